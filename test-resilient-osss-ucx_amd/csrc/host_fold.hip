// host_fold.hip -- the fold of a SMALL reduce-to-all call whose arrays live
// in host symmetric-heap memory, on the calling PE's own thread.
//
// The reference's whole algorithm for such a call is a CPU loop
// (src/reductions.c:79-111: copy the source into the target, barrier, pull
// every other PE's source with a blocking 64-element shmem_getmem and fold it
// through an indirect call per element, barrier).  For 1 Ki ints that loop
// takes 4-7 us; the GPU paths cannot come below a kernel launch whose
// completion the host sees (6.4 us for an empty kernel, DESIGN_HISTORY.md
// 10) plus the PCIe legs: the fused one-launch staged path takes 15-17 us.
// So while a PE pulls at most host_fold_max_bytes() from its peers
// (shmem_reduce.cpp run_host_fold) a host-heap call is folded here: one
// shmem_getmem per peer of its whole source, and a direct (inlined, not
// indirect) fold in the reference's per-PE order.
//
// The element ops are the SAME definitions the kernels use (elem_ops.hpp
// functors, x87.hpp soft-float for long double), compiled for the host: the
// results are bit-identical to the GPU paths' (tests/test_gpu_parity.py
// test_host_fold_matches_golden and tests/test_multiproc.py
// test_host_staged_processes check both against the golden vectors), not
// merely to the host compiler's view of the C operators.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "kernel_common.hpp"
#include "loc_host.hpp"
#include "wsum_host.hpp"
#include "x87.hpp"

#pragma clang fp contract(off)

namespace osgpu {
namespace {

template <typename T, int OP>
void fold_n(void *acc_v, const void *in_v, size_t n)
{
    T *acc = static_cast<T *>(acc_v);
    const T *in = static_cast<const T *>(in_v);
    for (size_t i = 0; i < n; i++) acc[i] = Elem<T, OP>::f(acc[i], in[i]);
}

// long double: 16-byte slots, value in bytes 0..9, padding written as zero
// (as longdouble.hip stores it)
template <int OP>
void fold_ld(void *acc_v, const void *in_v, size_t n)
{
    uint64_t *acc = static_cast<uint64_t *>(acc_v);
    const uint64_t *in = static_cast<const uint64_t *>(in_v);
    for (size_t i = 0; i < n; i++) {
        const x87::X80 a{acc[2 * i], (uint32_t) (acc[2 * i + 1] & 0xffffu)};
        const x87::X80 b{in[2 * i], (uint32_t) (in[2 * i + 1] & 0xffffu)};
        x87::X80 r;
        if (OP == OP_SUM) r = x87::add(a, b);
        else if (OP == OP_PROD) r = x87::mul(a, b);
        else if (OP == OP_MAX) r = x87::less(b, a) ? a : b;  // a > b ? a : b
        else r = x87::less(a, b) ? a : b;                     // a < b ? a : b
        acc[2 * i] = r.m;
        acc[2 * i + 1] = (uint64_t) (r.se & 0xffffu);
    }
}

typedef void (*FoldFn)(void *, const void *, size_t);

FoldFn fold_fn(int type, int op)
{
    if (type == T_LONGDOUBLE)
        return dispatch_ld_op(op, (FoldFn) nullptr,
                              [](auto o) -> FoldFn { return fold_ld<decltype(o)::value>; });
    return dispatch_type_op(type, op, (FoldFn) nullptr, [](auto t, auto o) -> FoldFn {
        return fold_n<typename decltype(t)::type, decltype(o)::value>;
    });
}

typedef void (*LocFoldFn)(void *, int32_t *, const void *, const int32_t *, int32_t, size_t);

// osgpu_reduce_loc's step (elem_ops.hpp LocStep) over loc_host.hpp's loop
template <typename T, int OP>
void fold_loc_n(void *v, int32_t *i, const void *b, const int32_t *ib, int32_t ib_const, size_t n)
{
    rt::loc_fold_n<LocStep<T, OP>, T>(static_cast<T *>(v), i, static_cast<const T *>(b), ib,
                                      ib_const, n);
}

LocFoldFn loc_fold_fn(int type, int op)
{
    return dispatch_type_op(type, op, (LocFoldFn) nullptr, [](auto t, auto o) -> LocFoldFn {
        using T = typename decltype(t)::type;
        constexpr int OP = decltype(o)::value;
        constexpr bool kOrdered = std::is_integral<T>::value || std::is_floating_point<T>::value ||
                                  is_f16<T>::value;
        if constexpr (kOrdered && (OP == OP_MAX || OP == OP_MIN)) return fold_loc_n<T, OP>;
        else return nullptr;
    });
}

}  // namespace

bool host_fold_loc_supported(int type, int op) { return loc_fold_fn(type, op) != nullptr; }

// (val[k], loc[k]) takes (in_val[k], in_loc ? in_loc[k] : in_const) for k < n
bool host_fold_loc(int type, int op, void *val, int *loc, const void *in_val, const int *in_loc,
                   int in_const, size_t n)
{
    const LocFoldFn f = loc_fold_fn(type, op);
    if (!f) return false;
    f(val, loc, in_val, in_loc, in_const, n);
    return true;
}

// osgpu_reduce_wsum's steps (elem_ops.hpp WsumStep) over wsum_host.hpp's loops
bool host_wsum_widen(int type, float *acc, const void *src, size_t n)
{
    if (type == T_HALF)
        rt::wsum_widen_n<WsumStep<half_t>>(acc, static_cast<const half_t *>(src), n);
    else if (type == T_BFLOAT16)
        rt::wsum_widen_n<WsumStep<bf16_t>>(acc, static_cast<const bf16_t *>(src), n);
    else return false;
    return true;
}

bool host_wsum_add(int type, float *acc, const void *in, size_t n)
{
    if (type == T_HALF) rt::wsum_add_n<WsumStep<half_t>>(acc, static_cast<const half_t *>(in), n);
    else if (type == T_BFLOAT16)
        rt::wsum_add_n<WsumStep<bf16_t>>(acc, static_cast<const bf16_t *>(in), n);
    else return false;
    return true;
}

bool host_wsum_narrow(int type, void *out, const float *acc, size_t n)
{
    if (type == T_HALF) rt::wsum_narrow_n<WsumStep<half_t>>(static_cast<half_t *>(out), acc, n);
    else if (type == T_BFLOAT16)
        rt::wsum_narrow_n<WsumStep<bf16_t>>(static_cast<bf16_t *>(out), acc, n);
    else return false;
    return true;
}

bool host_fold_supported(int type, int op) { return fold_fn(type, op) != nullptr; }

// acc[i] = op(acc[i], in[i]) for i < n, elements of `type`
bool host_fold(int type, int op, void *acc, const void *in, size_t n)
{
    const FoldFn f = fold_fn(type, op);
    if (!f) return false;
    f(acc, in, n);
    return true;
}

}  // namespace osgpu
