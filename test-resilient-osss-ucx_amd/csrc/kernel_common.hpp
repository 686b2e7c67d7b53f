// kernel_common.hpp -- the decisions every kernel file (.hip) shares; never
// included by the host .cpp layer.
//  * u32x4 / Vec16: the 16-byte vector a lane loads and stores;
//  * dispatch_type_op: which (type, op) pairs exist and the C++ type of each
//    type code; dispatch_members: the member counts a team kernel is built for;
//  * vec_split / edge_index: n elements at a 16-byte phase as a scalar head,
//    whole vectors and a scalar tail;
//  * for_each_tile_run: a call of more than max_launch_threads() threads as
//    several launches over runs of whole tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <type_traits>

#include "combine.hpp"
#include "elem_ops.hpp"

#pragma clang fp contract(off)

namespace osgpu {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
union Vec16 {
    u32x4 v;
    T e[16 / sizeof(T)];
};

// ------------------------------------------------------------ (type, op)
template <typename T>
struct type_tag {
    using type = T;
};
template <int OP>
using op_tag = std::integral_constant<int, OP>;

// f(type_tag<T>, op_tag<OP>) for the ops T admits -- integers all seven,
// real types (half_t and bf16_t among them) sum / prod / max / min, complex
// types sum / prod -- else fallback
template <typename T, typename R, typename F>
R dispatch_op(int op, R fallback, F &&f)
{
    constexpr bool kInt = std::is_integral<T>::value;
    constexpr bool kOrdered = kInt || std::is_floating_point<T>::value || is_f16<T>::value;
    switch (op) {
    case OP_SUM: return f(type_tag<T>{}, op_tag<OP_SUM>{});
    case OP_PROD: return f(type_tag<T>{}, op_tag<OP_PROD>{});
    case OP_AND: if constexpr (kInt) return f(type_tag<T>{}, op_tag<OP_AND>{}); break;
    case OP_OR: if constexpr (kInt) return f(type_tag<T>{}, op_tag<OP_OR>{}); break;
    case OP_XOR: if constexpr (kInt) return f(type_tag<T>{}, op_tag<OP_XOR>{}); break;
    case OP_MAX: if constexpr (kOrdered) return f(type_tag<T>{}, op_tag<OP_MAX>{}); break;
    case OP_MIN: if constexpr (kOrdered) return f(type_tag<T>{}, op_tag<OP_MIN>{}); break;
    }
    return fallback;
}

// f(type_tag<T>, op_tag<OP>) of a valid (type, op) pair; fallback for an
// invalid one and for T_LONGDOUBLE (x87 soft-float, no C++ type on the GPU:
// callers handle it themselves, see dispatch_ld_op)
template <typename R, typename F>
R dispatch_type_op(int type, int op, R fallback, F &&f)
{
    switch (type) {
    case T_SHORT: return dispatch_op<int16_t>(op, fallback, f);
    case T_INT: return dispatch_op<int32_t>(op, fallback, f);
    case T_LONG:
    case T_LONGLONG: return dispatch_op<int64_t>(op, fallback, f);
    case T_FLOAT: return dispatch_op<float>(op, fallback, f);
    case T_DOUBLE: return dispatch_op<double>(op, fallback, f);
    case T_COMPLEXF: return dispatch_op<cfloat>(op, fallback, f);
    case T_COMPLEXD: return dispatch_op<cdouble>(op, fallback, f);
    case T_HALF: return dispatch_op<half_t>(op, fallback, f);
    case T_BFLOAT16: return dispatch_op<bf16_t>(op, fallback, f);
    }
    return fallback;
}

// f(op_tag<OP>) for long double's ops (a real type's: sum / prod / max / min)
template <typename R, typename F>
R dispatch_ld_op(int op, R fallback, F &&f)
{
    return dispatch_op<long double>(op, fallback, [&](auto, auto o) { return f(o); });
}

// f(integral_constant<int, P>) for the member counts the team kernels are
// built for, 2 .. kMaxTeam; else fallback
template <typename R, typename F>
R dispatch_members(int P, R fallback, F &&f)
{
    static_assert(kMaxTeam == 8, "one case per member count");
    switch (P) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    }
    return fallback;
}

// ------------------------------------------------------------ vector split
// n elements whose arrays share one 16-byte phase: elements [0, head) up to
// the first 16-byte boundary, nvec whole vectors, then the tail from
// tail_start; nedge = head + tail elements, folded one per lane.
// vec false (and the rest 0): the element-granular kernel serves.
struct VecSplit {
    bool vec;
    size_t head, nvec, tail_start;
    int nedge;
};

// a[0 .. na) and b[0 .. nb): the pointers that must share a[0]'s phase
template <typename A, typename B>
VecSplit vec_split(size_t elem, size_t n, A *const *a, int na, B *const *b, int nb)
{
    const uintptr_t phase = (uintptr_t) a[0] & 15;
    bool same = elem <= 16 && (phase % elem) == 0;
    for (int i = 0; i < na; i++) same = same && ((uintptr_t) a[i] & 15) == phase;
    for (int i = 0; i < nb; i++) same = same && ((uintptr_t) b[i] & 15) == phase;
    if (!same) return VecSplit{false, 0, 0, 0, 0};
    size_t head = phase ? (16 - phase) / elem : 0;
    if (head > n) head = n;
    const size_t nvec = (n - head) / (16 / elem);
    const size_t tail_start = head + nvec * (16 / elem);
    return VecSplit{true, head, nvec, tail_start, (int) (head + (n - tail_start))};
}

// the edges: lanes [0, nedge) of workgroup 0 take one element each, the head
// elements first, then the tail's; this lane's
__device__ __forceinline__ size_t edge_index(size_t head, size_t tail_start)
{
    return threadIdx.x < head ? threadIdx.x : tail_start + (threadIdx.x - head);
}

// --------------------------------------------------------------- tile runs
// nvec vectors in tiles of V, one tile per workgroup of `threads`, at most
// max_launch_threads() per launch (combine.hpp): fn(t0, nt, nv) for every
// run of nt tiles from tile t0 holding nv vectors, until one fails.  Runs
// are whole multiples of m tiles (launch_team_tiles: tile t of a run is
// still member k's when t % m == k).  The first run (t0 == 0) carries the
// edges; the others take pointers shifted by t0 * V vectors.
template <typename Fn>
hipError_t for_each_tile_run(size_t nvec, size_t V, unsigned threads, size_t m, Fn &&fn)
{
    size_t tiles = (nvec + V - 1) / V;
    if (tiles == 0) tiles = 1;
    const size_t lim = max_launch_threads() / threads;
    const size_t run = (lim ? lim : 1) * m;
    for (size_t t0 = 0; t0 < tiles; t0 += run) {
        const size_t nt = tiles - t0 < run ? tiles - t0 : run;
        const size_t nv = nvec - t0 * V < nt * V ? nvec - t0 * V : nt * V;
        const hipError_t e = fn(t0, nt, nv);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace osgpu
