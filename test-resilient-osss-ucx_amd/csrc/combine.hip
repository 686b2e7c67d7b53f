// combine.hip -- the reduce-to-all combine as gfx950 streaming kernels.
//
// out[i] = op(...op(op(in[0][i], in[1][i]), in[2][i])..., in[K-1][i])
//
// This is the element-wise fold of src/reductions.c:79-111 (copy source,
// then fold every peer's source in PE order) with the 64-element pWrk bounce
// and the per-element indirect call removed: every input is streamed once
// from HBM (local or a peer GPU's over xGMI), the accumulator never leaves
// registers, and the target is written once.  HBM bytes per element:
// (K + 1) * sizeof(T) -- the roofline quantity reported by bench.py.
//
// Shape (MI355X: 256 CUs, 64-wide waves, 16-B global_load_dwordx4):
//  * one 16-byte vector per lane per load; a 256-thread workgroup covers
//    256*U consecutive vectors of every input, so each wave-instruction is a
//    fully coalesced 1 KiB access;
//  * all K*U loads of a lane are issued before the fold, so a lane keeps
//    K*U*16 B in flight (K=2, U=4: 128 B/lane, 32 KiB per workgroup);
//  * the result is stored nontemporal (it is not re-read by this kernel);
//  * the head/tail elements that do not fill a 16-B vector (unaligned start,
//    ragged n) are folded by the first lanes of workgroup 0, so one launch
//    covers any n.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stddef.h>

#include <vector>

#include "kernel_common.hpp"
#include "many_host.hpp"

#pragma clang fp contract(off)

namespace osgpu {

template <typename T, int K>
struct Inputs {
    const T *p[K];
};

constexpr int kBlock = 256;

// above 6 inputs: vectors per input in flight per round (U = kUK8 in all);
// G = U keeps every load of the tile in flight at once (G = 2 and 1 were
// measured no faster: tools/combine_variants.py)
constexpr int kCombineG8 = kUK8;

// lanes per vector-tile unroll: keep K*U*4 VGPRs of payload modest
template <int K>
struct Unroll {
    static constexpr int value = K <= 2 ? kUK2 : (K <= 4 ? kUK4 : kUK8);
};

template <typename T, int OP, int K>
__device__ __forceinline__ T fold_scalar(const Inputs<T, K> &in, size_t i)
{
    T x[K];
#pragma unroll
    for (int k = 0; k < K; k++) x[k] = in.p[k][i];
    T acc = x[0];
#pragma unroll
    for (int k = 1; k < K; k++) acc = Elem<T, OP>::f(acc, x[k]);
    return acc;
}

// the branch-free fold (elem_ops.hpp Fast), redone with the exact one only
// for a vector whose result holds a NaN part: no branch per element
template <typename T, int OP, int K>
__device__ __forceinline__ void fold_vec(Vec16<T> (&x)[K], Vec16<T> &out)
{
    constexpr int W = 16 / sizeof(T);
    using F = Fast<T, OP>;
    bool bad = false;
#pragma unroll
    for (int w = 0; w < W; w++) {
        T acc = x[0].e[w];
#pragma unroll
        for (int k = 1; k < K; k++) acc = F::f(acc, x[k].e[w]);
        out.e[w] = acc;
        bad = bad || F::bad(acc);
    }
    if (F::kChecked && __builtin_expect(bad, 0)) {
#pragma unroll
        for (int w = 0; w < W; w++) {
            T acc = x[0].e[w];
#pragma unroll
            for (int k = 1; k < K; k++) acc = Elem<T, OP>::f(acc, x[k].e[w]);
            out.e[w] = acc;
        }
    }
}

// Vector body over [head, head + nvec*W) plus the scalar edges.
template <typename T, int OP, int K>
__global__ __launch_bounds__(kBlock) void combine_vec_kernel(
    T *out, Inputs<T, K> in, size_t nvec, size_t head, size_t tail_start,
    int nedge)
{
    constexpr int U = Unroll<K>::value;
    constexpr int W = 16 / sizeof(T);
    const size_t tid = (size_t) blockIdx.x * (kBlock * U) + threadIdx.x;

    // edges: head elements [0, head) and tail [tail_start, tail_start + ...)
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        out[e] = fold_scalar<T, OP, K>(in, e);
    }

    const u32x4 *src[K];
#pragma unroll
    for (int k = 0; k < K; k++) src[k] = reinterpret_cast<const u32x4 *>(in.p[k] + head);
    u32x4 *dst = reinterpret_cast<u32x4 *>(out + head);
    (void) W;

    if (tid + (size_t) (U - 1) * kBlock < nvec) {
        // the loads of G vectors of every input in flight before their folds
        // (G = U: all K*U of them; above 6 inputs kCombineG8)
        constexpr int G = K <= 6 ? U : kCombineG8;
        static_assert(G >= 1 && G <= U && U % G == 0, "kCombineG8 must divide U");
#pragma unroll
        for (int g = 0; g < U; g += G) {
            Vec16<T> x[G][K];
#pragma unroll
            for (int u = 0; u < G; u++)
#pragma unroll
                for (int k = 0; k < K; k++)
                    x[u][k].v = __builtin_nontemporal_load(&src[k][tid + (size_t) (g + u) * kBlock]);
#pragma unroll
            for (int u = 0; u < G; u++) {
                Vec16<T> r;
                fold_vec<T, OP, K>(x[u], r);
                __builtin_nontemporal_store(r.v, &dst[tid + (size_t) (g + u) * kBlock]);
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t j = tid + (size_t) u * kBlock;
            if (j < nvec) {
                Vec16<T> x[K], r;
#pragma unroll
                for (int k = 0; k < K; k++) x[k].v = __builtin_nontemporal_load(&src[k][j]);
                fold_vec<T, OP, K>(x, r);
                __builtin_nontemporal_store(r.v, &dst[j]);
            }
        }
    }
}

// LDS-staged form (2 <= K <= kCombineLdsMaxK): K
// waves per workgroup, a tile of 64*U 16-B vectors of every input.  Wave k
// streams input k's tile into LDS (one read stream per wave, like the copy
// kernel and team_lds_kernel); after the barrier the K waves fold the tile
// from LDS in input order and store it, each a contiguous 1 KiB per
// instruction.  HBM bytes as combine_vec_kernel.  Timed against it in one
// process on the same fresh arrays (tools/combine_inproc_ab.py, 6
// allocations each, profiles/r05_combine_lds_ab.jsonl): double sum K = 2
// 1.04x with U = 2 (0.824 against 0.792 of 8 TB/s median; 1.02x with
// U = 4), K = 3 and 4 1.02x with U = 4 (U = 2: 1.01x, 0.98x); float / int
// sum 1.02x / 1.04x, long xor 1.01x, double max 1.00x at K = 2; K = 5 and
// 8 (32 Mi doubles) 1.04x and 1.07x with U = 4 (U = 2: 1.01x, 1.05x); at
// 8 / 64 / 128 Mi doubles, K = 2: 1.07x / 1.04x / 1.04x.
constexpr int kCombineLdsMaxK = 8;
#ifndef OSGPU_COMBINE_LDS_U2
#define OSGPU_COMBINE_LDS_U2 2  // vectors per lane per input at K = 2 (the headline kernel)
#endif
constexpr int kCombineLdsU = 4;  // ... at K = 3 .. 8
// (Round 6, in one process on the same arrays, 6 allocations each,
// profiles/r06_combine_glds_ab.jsonl: the tile staged by LDS-DMA --
// global_load_lds_dwordx4, no VGPR round trip -- 1.005x at U = 2 (min
// 0.997x), 0.985x at U = 4, 0.975x at U = 8; register staging at U = 4
// 0.979x.  Within noise at best: the register staging ships.  Several
// tiles per workgroup, the next tile's loads in flight during this one's
// fold (profiles/r06_combine_tpw_ab.jsonl): 2 tiles 0.979x, 4 tiles 0.912x,
// 4 strided tiles 0.922x, 4 tiles of U = 1 0.993x -- one tile per
// workgroup, a one-shot grid, ships.)

template <typename T, int OP, int K, int U>
__global__ __launch_bounds__(64 * K) void combine_lds_kernel(T *out, Inputs<T, K> in, size_t nvec,
                                                              size_t head, size_t tail_start,
                                                              int nedge)
{
    constexpr int V = 64 * U;  // vectors per input per tile
    __shared__ u32x4 tile[K][V];
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        out[e] = fold_scalar<T, OP, K>(in, e);
    }
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63);
    const size_t base = (size_t) blockIdx.x * V;
    const bool whole = base + V <= nvec;
    const T *pw = in.p[0];
#pragma unroll
    for (int k = 1; k < K; k++)
        if (w == k) pw = in.p[k];
    const u32x4 *src = reinterpret_cast<const u32x4 *>(pw + head);
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++)
        if (whole || base + u * 64 + lane < nvec)
            v[u] = __builtin_nontemporal_load(src + base + u * 64 + lane);
#pragma unroll
    for (int u = 0; u < U; u++) tile[w][u * 64 + lane] = v[u];
    __syncthreads();
    u32x4 *dst = reinterpret_cast<u32x4 *>(out + head);
    for (int j = (int) threadIdx.x; j < V; j += 64 * K) {
        if (!whole && base + j >= nvec) continue;
        Vec16<T> x[K], r;
#pragma unroll
        for (int k = 0; k < K; k++) x[k].v = tile[k][j];
        fold_vec<T, OP, K>(x, r);
        __builtin_nontemporal_store(r.v, dst + base + j);
    }
}

// Shifted form of combine_lds_kernel (launch_combine_shifted): every pointer
// at its own 16-byte phase, each a multiple of sizeof(T) -- block m of a
// symmetric source against a target at its own address (the reduce-scatter).
// The target's 16-byte vectors tile the call as above.  Input k's bytes of
// target vector j start sh_k = (in_k + head) & 15 bytes into ITS aligned
// vector j, so wave k streams the tile's V aligned vectors of input k plus,
// when sh_k != 0, the one after them (the halo: 16 B per input per tile)
// into its LDS row of V + 1 slots; the fold reads input k at byte 16 j + sh_k
// of row k.  Every global access of the body is an aligned 16-byte one.
// The launcher keeps every aligned vector inside [in_k, in_k + n): a first
// or last target vector whose cover would start before an input or end past
// it goes to the element-wise edges.
//
// The read at the shift: slots j and j + 1 as two aligned 16-byte reads, the
// 16 bytes picked out of the 32 in registers (sh_k is wave-uniform: one of
// four static dword selections, v_alignbyte for the 2-byte types).  A
// 16-byte LDS read off its alignment is not an option: it is replayed at 64
// cycles per wave-instruction.  Reads at the element's own alignment (two
// 8-byte, four 4-byte, five 4-byte + v_alignbyte) timed the same within
// 0.5 % and are gone (tools/rscatter_rate.py, profiles/rscatter_rate.md:
// U = 2 is 4 % ahead of U = 4 and 6 % ahead of U = 1).  An input at shift 0
// (the fed-back target of a second chunk always is) takes one aligned read.
#ifndef OSGPU_SHIFT_U
#define OSGPU_SHIFT_U 2  // vectors per lane per input, every K
#endif

// bytes [sh, sh + 16) of lo:hi; sh wave-uniform, a multiple of E = sizeof(T)
template <int E>
__device__ __forceinline__ u32x4 shift_pair(u32x4 lo, u32x4 hi, unsigned sh)
{
    const unsigned x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    u32x4 r;
    if constexpr (E == 8) {  // sh is 0 or 8
        r = sh ? u32x4{x[2], x[3], x[4], x[5]} : lo;
    } else if constexpr (E == 4) {
        switch (sh >> 2) {
        case 1: r = u32x4{x[1], x[2], x[3], x[4]}; break;
        case 2: r = u32x4{x[2], x[3], x[4], x[5]}; break;
        case 3: r = u32x4{x[3], x[4], x[5], x[6]}; break;
        default: r = lo; break;
        }
    } else {
        const unsigned b = sh & 3;
#define OSGPU_AB(i) __builtin_amdgcn_alignbyte(x[(i) + 1], x[i], b)
        switch (sh >> 2) {
        case 0: r = u32x4{OSGPU_AB(0), OSGPU_AB(1), OSGPU_AB(2), OSGPU_AB(3)}; break;
        case 1: r = u32x4{OSGPU_AB(1), OSGPU_AB(2), OSGPU_AB(3), OSGPU_AB(4)}; break;
        case 2: r = u32x4{OSGPU_AB(2), OSGPU_AB(3), OSGPU_AB(4), OSGPU_AB(5)}; break;
        default: r = u32x4{OSGPU_AB(3), OSGPU_AB(4), OSGPU_AB(5), OSGPU_AB(6)}; break;
        }
#undef OSGPU_AB
    }
    return r;
}

// the 16 bytes at byte 16 j + sh of an LDS row
template <typename T>
__device__ __forceinline__ u32x4 read_shifted(const u32x4 *row, int j, unsigned sh)
{
    if (sh == 0) return row[j];
    return shift_pair<(int) sizeof(T)>(row[j], row[j + 1], sh);
}

template <typename T, int OP, int K, int U>
__global__ __launch_bounds__(64 * K) void combine_shift_kernel(T *out, Inputs<T, K> in, size_t nvec,
                                                                size_t head, size_t tail_start,
                                                                int nedge)
{
    constexpr int V = 64 * U;  // target vectors per tile
    __shared__ u32x4 tile[K][V + 1];
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        out[e] = fold_scalar<T, OP, K>(in, e);
    }
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63);
    const size_t base = (size_t) blockIdx.x * V;
    const bool whole = base + V <= nvec;
    const int cnt = whole ? V : (base < nvec ? (int) (nvec - base) : 0);  // this tile's vectors
    const T *pw = in.p[0];
#pragma unroll
    for (int k = 1; k < K; k++)
        if (w == k) pw = in.p[k];
    const uintptr_t at = reinterpret_cast<uintptr_t>(pw + head);
    const u32x4 *src = reinterpret_cast<const u32x4 *>(at - (at & 15)) + base;
    const bool halo = (at & 15) != 0 && lane == 0 && cnt > 0;
    u32x4 v[U], h = {};
#pragma unroll
    for (int u = 0; u < U; u++)
        if (u * 64 + lane < cnt) v[u] = __builtin_nontemporal_load(src + u * 64 + lane);
    if (halo) h = __builtin_nontemporal_load(src + cnt);
#pragma unroll
    for (int u = 0; u < U; u++)
        if (u * 64 + lane < cnt) tile[w][u * 64 + lane] = v[u];
    if (halo) tile[w][cnt] = h;
    __syncthreads();
    unsigned sh[K];
#pragma unroll
    for (int k = 0; k < K; k++)
        sh[k] = (unsigned) (reinterpret_cast<uintptr_t>(in.p[k] + head) & 15);
    u32x4 *dst = reinterpret_cast<u32x4 *>(out + head);
    for (int j = (int) threadIdx.x; j < cnt; j += 64 * K) {
        Vec16<T> x[K], r;
#pragma unroll
        for (int k = 0; k < K; k++) x[k].v = read_shifted<T>(tile[k], j, sh[k]);
        fold_vec<T, OP, K>(x, r);
        __builtin_nontemporal_store(r.v, dst + base + j);
    }
}

// Batched form of combine_lds_kernel (launch_combine_many): one grid over a
// table of up to kManySegs independent arrays, each a segment with its own
// pointers, vector split and run of workgroups.  The table travels by value
// in the kernel arguments (K = 8: 104 bytes a segment, 1664 in all), so no
// copy to the device sits on the latency path.  A workgroup finds its segment
// by counting the segments that start at or before it (unused ones start at
// ~0u); the index is wave-uniform and kept in an SGPR, so the segment's
// fields -- wave k's input pointer among them -- are scalar loads from the
// kernel argument segment.  Within the segment the workgroup is
// combine_lds_kernel's: wave k streams input k's tile, the tile is folded in
// input order, the segment's first workgroup folds its edges.
// U = 2 (V = 128 vectors), the shift kernel's shape: not measured against
// U = 1 and 4.
#ifndef OSGPU_MANY_U
#define OSGPU_MANY_U 2  // vectors per lane per input, every K
#endif

template <typename T, int K>
struct ManySeg {
    T *out;
    const T *in[K];
    size_t nvec, head, tail_start;
    int nedge;
    unsigned first;  // the segment's first workgroup of the launch
};

template <typename T, int K>
struct ManyTable {
    ManySeg<T, K> seg[kManySegs];
};

template <typename T, int OP, int K, int U>
__global__ __launch_bounds__(64 * K) void combine_many_kernel(ManyTable<T, K> tab)
{
    constexpr int V = 64 * U;  // vectors per input per tile
    __shared__ u32x4 tile[K][V];
    int si = 0;
#pragma unroll
    for (int i = 1; i < kManySegs; i++) si += blockIdx.x >= tab.seg[i].first ? 1 : 0;
    si = __builtin_amdgcn_readfirstlane(si);
    const ManySeg<T, K> &g = tab.seg[si];
    const unsigned blk = blockIdx.x - g.first;
    T *out = g.out;
    const size_t nvec = g.nvec, head = g.head;
    if (blk == 0 && (int) threadIdx.x < g.nedge) {
        Inputs<T, K> in;
#pragma unroll
        for (int k = 0; k < K; k++) in.p[k] = g.in[k];
        const size_t e = edge_index(head, g.tail_start);
        out[e] = fold_scalar<T, OP, K>(in, e);
    }
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63);
    const size_t base = (size_t) blk * V;
    const bool whole = base + V <= nvec;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(g.in[w] + head);
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++)
        if (whole || base + u * 64 + lane < nvec)
            v[u] = __builtin_nontemporal_load(src + base + u * 64 + lane);
#pragma unroll
    for (int u = 0; u < U; u++) tile[w][u * 64 + lane] = v[u];
    __syncthreads();
    u32x4 *dst = reinterpret_cast<u32x4 *>(out + head);
    for (int j = (int) threadIdx.x; j < V; j += 64 * K) {
        if (!whole && base + j >= nvec) continue;
        Vec16<T> x[K], r;
#pragma unroll
        for (int k = 0; k < K; k++) x[k].v = tile[k][j];
        fold_vec<T, OP, K>(x, r);
        __builtin_nontemporal_store(r.v, dst + base + j);
    }
}

// Element-granular fallback for inputs whose 16-byte phases differ.
template <typename T, int OP, int K>
__global__ __launch_bounds__(kBlock) void combine_scalar_kernel(T *out, Inputs<T, K> in,
                                                                size_t n)
{
    const size_t stride = (size_t) gridDim.x * kBlock;
    for (size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        out[i] = fold_scalar<T, OP, K>(in, i);
}

// ------------------------------------------------------------------ launch

static std::atomic<size_t> g_launch_threads{kMaxLaunchThreads};
size_t max_launch_threads() { return g_launch_threads.load(std::memory_order_relaxed); }
void set_max_launch_threads(size_t n) { g_launch_threads.store(n, std::memory_order_relaxed); }

template <typename T, int OP, int K>
static hipError_t launch_k(T *out, const T *const *srcs, size_t n, hipStream_t s)
{
    Inputs<T, K> in;
    for (int k = 0; k < K; k++) in.p[k] = srcs[k];
    const VecSplit vs = vec_split(sizeof(T), n, &out, 1, srcs, K);
    if (!vs.vec) {
        size_t blocks = (n + kBlock - 1) / kBlock;
        if (blocks > 8192) blocks = 8192;
        if (blocks == 0) blocks = 1;
        hipLaunchKernelGGL((combine_scalar_kernel<T, OP, K>), dim3((unsigned) blocks),
                           dim3(kBlock), 0, s, out, in, n);
        return hipGetLastError();
    }
    constexpr int W = 16 / sizeof(T);
    constexpr int U = Unroll<K>::value;
    // tiles of V vectors, one per workgroup of `threads`: the first launch
    // takes the edges, the others the next runs of tiles through shifted
    // pointers (for_each_tile_run)
    auto launch = [&](size_t V, unsigned threads, auto kernel) -> hipError_t {
        return for_each_tile_run(vs.nvec, V, threads, 1, [&](size_t t0, size_t nt, size_t nv) {
            if (t0 == 0) {
                hipLaunchKernelGGL(kernel, dim3((unsigned) nt), dim3(threads), 0, s, out, in, nv,
                                   vs.head, vs.tail_start, vs.nedge);
            } else {
                const size_t off = vs.head + t0 * V * W;
                Inputs<T, K> ic;
                for (int k = 0; k < K; k++) ic.p[k] = in.p[k] + off;
                hipLaunchKernelGGL(kernel, dim3((unsigned) nt), dim3(threads), 0, s, out + off, ic, nv,
                                   (size_t) 0, (size_t) 0, 0);
            }
            return hipGetLastError();
        });
    };
    if constexpr (K >= 2 && K <= kCombineLdsMaxK) {
        constexpr int UL = K == 2 ? OSGPU_COMBINE_LDS_U2 : kCombineLdsU;
        return launch((size_t) 64 * UL, 64 * K, combine_lds_kernel<T, OP, K, UL>);
    }
    return launch((size_t) kBlock * U, kBlock, combine_vec_kernel<T, OP, K>);
}

// launch_combine_shifted's choice for one chunk: the kernels above when all
// phases agree (and for one input, a copy, and for 16-byte elements, which
// always share a phase), combine_shift_kernel when every pointer is aligned
// to its element, combine_scalar_kernel (through launch_k) otherwise.
// What launch_shift_k chose, per process (shift_route_counts; tests and
// tools/rscatter_rate.py): chunks handed to launch_k's own choice, chunks on
// combine_shift_kernel, chunks off their element alignment, and the
// launches of combine_shift_kernel.
static std::atomic<unsigned long long> g_shift_routes[4];

template <typename T, int OP, int K>
static hipError_t launch_shift_k(T *out, const T *const *srcs, size_t n, hipStream_t s)
{
    if constexpr (K < 2 || K > kCombineLdsMaxK || sizeof(T) >= 16) {
        g_shift_routes[0]++;
        return launch_k<T, OP, K>(out, srcs, n, s);
    } else {
        constexpr size_t E = sizeof(T);
        constexpr size_t W = 16 / E;
        bool same = true, elem = (uintptr_t) out % E == 0;
        for (int k = 0; k < K; k++) {
            same = same && (((uintptr_t) srcs[k] ^ (uintptr_t) out) & 15) == 0;
            elem = elem && (uintptr_t) srcs[k] % E == 0;
        }
        if (same || !elem) {
            g_shift_routes[elem ? 0 : 2]++;
            return launch_k<T, OP, K>(out, srcs, n, s);
        }
        g_shift_routes[1]++;
        // the split of the target alone; then the vector body gives up its
        // first / last vector to the edges where an input's aligned vectors
        // covering it would start before that input or end past it
        const VecSplit vs = vec_split(E, n, &out, 1, srcs, 0);
        size_t head = vs.head, nvec = vs.nvec;
        const size_t tail_bytes = (n - vs.tail_start) * E;
        bool cut_first = false, cut_last = false;
        for (int k = 0; k < K; k++) {
            const size_t sh = (uintptr_t) (srcs[k] + head) & 15;
            cut_first = cut_first || (sh != 0 && head * E < sh);
            cut_last = cut_last || (sh != 0 && tail_bytes < 16 - sh);
        }
        if (cut_first && nvec > 0) head += W, nvec--;
        if (cut_last && nvec > 0) nvec--;
        const size_t tail_start = head + nvec * W;
        const int nedge = (int) (head + (n - tail_start));  // < 4 W <= 32 lanes
        Inputs<T, K> in;
        for (int k = 0; k < K; k++) in.p[k] = srcs[k];
        constexpr size_t V = (size_t) 64 * OSGPU_SHIFT_U;
        return for_each_tile_run(nvec, V, 64 * K, 1, [&](size_t t0, size_t nt, size_t nv) {
            auto kernel = combine_shift_kernel<T, OP, K, OSGPU_SHIFT_U>;
            g_shift_routes[3]++;
            if (t0 == 0) {
                hipLaunchKernelGGL(kernel, dim3((unsigned) nt), dim3(64 * K), 0, s, out, in, nv, head,
                                   tail_start, nedge);
            } else {
                // a later run: a non-last run's halo is the next run's first vector
                const size_t off = head + t0 * V * W;
                Inputs<T, K> ic;
                for (int k = 0; k < K; k++) ic.p[k] = in.p[k] + off;
                hipLaunchKernelGGL(kernel, dim3((unsigned) nt), dim3(64 * K), 0, s, out + off, ic, nv,
                                   (size_t) 0, (size_t) 0, 0);
            }
            return hipGetLastError();
        });
    }
}

constexpr int kMaxK = 8;

template <typename T, int OP, int K, bool SHIFT>
static hipError_t launch_chunk(T *out, const T *const *srcs, size_t n, hipStream_t s)
{
    if constexpr (SHIFT) return launch_shift_k<T, OP, K>(out, srcs, n, s);
    else return launch_k<T, OP, K>(out, srcs, n, s);
}

template <typename T, int OP, bool SHIFT = false>
static hipError_t launch_op(void *out_, const void *const *srcs_, int k, size_t n,
                            hipStream_t s)
{
    T *out = static_cast<T *>(out_);
    const T *const *srcs = reinterpret_cast<const T *const *>(srcs_);
    // fold in chunks of at most kMaxK inputs: out = fold(srcs[0..7]), then
    // out = fold(out, srcs[8..14]), ... -- left-to-right order is preserved
    const T *chunk[kMaxK];
    int done = 0;
    hipError_t err = hipSuccess;
    while (done < k && err == hipSuccess) {
        int m = 0;
        if (done > 0) chunk[m++] = out;
        while (m < kMaxK && done < k) chunk[m++] = srcs[done++];
        switch (m) {
        case 1: err = launch_chunk<T, OP, 1, SHIFT>(out, chunk, n, s); break;
        case 2: err = launch_chunk<T, OP, 2, SHIFT>(out, chunk, n, s); break;
        case 3: err = launch_chunk<T, OP, 3, SHIFT>(out, chunk, n, s); break;
        case 4: err = launch_chunk<T, OP, 4, SHIFT>(out, chunk, n, s); break;
        case 5: err = launch_chunk<T, OP, 5, SHIFT>(out, chunk, n, s); break;
        case 6: err = launch_chunk<T, OP, 6, SHIFT>(out, chunk, n, s); break;
        case 7: err = launch_chunk<T, OP, 7, SHIFT>(out, chunk, n, s); break;
        default: err = launch_chunk<T, OP, 8, SHIFT>(out, chunk, n, s); break;
        }
    }
    return err;
}

hipError_t launch_combine(int type, int op, void *out, const void *const *srcs, int k,
                          size_t n, hipStream_t s)
{
    if (k < 1 || out == nullptr) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (type == T_LONGDOUBLE) return launch_longdouble(op, out, srcs, k, n, s);
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        return launch_op<typename decltype(t)::type, decltype(o)::value>(out, srcs, k, n, s);
    });
}

void shift_route_counts(unsigned long long out[4], int *u)
{
    for (int i = 0; i < 4; i++) out[i] = g_shift_routes[i].load();
    *u = OSGPU_SHIFT_U;
}

// launch_combine with every pointer at its own 16-byte phase (the feedback of
// `out` as input 0 of a second chunk is why every input has its own shift)
hipError_t launch_combine_shifted(int type, int op, void *out, const void *const *srcs, int k,
                                  size_t n, hipStream_t s)
{
    if (k < 1 || out == nullptr) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (type == T_LONGDOUBLE) return launch_longdouble(op, out, srcs, k, n, s);
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        return launch_op<typename decltype(t)::type, decltype(o)::value, true>(out, srcs, k, n, s);
    });
}

// ------------------------------------------------------- batched combine
// What launch_combine_many chose, per process (many_route_counts): [0]
// segments on combine_many_kernel (continuations included), entries sent to
// [1] launch_combine_shifted, [2] launch_longdouble, [3] launch_combine's
// chunks of 8, [4] the one-input copy, [5] launches of combine_many_kernel,
// [6] continuations (segments that carry on an entry split between launches).
static std::atomic<unsigned long long> g_many_routes[7];

// one launch: the pieces' segments of the table, `blocks` workgroups
template <typename T, int OP, int K>
static hipError_t launch_many_k(const rt::ManyPiece *pc, int np, size_t blocks,
                                void *const *targets, const void *const *const *srcs,
                                const size_t *nelems, hipStream_t s)
{
    constexpr size_t W = 16 / sizeof(T), V = (size_t) 64 * OSGPU_MANY_U;
    ManyTable<T, K> tab;
    for (int i = 0; i < kManySegs; i++) {
        tab.seg[i] = ManySeg<T, K>{};
        tab.seg[i].first = ~0u;
    }
    for (int i = 0; i < np; i++) {
        const int e = pc[i].entry;
        T *out = static_cast<T *>(targets[e]);
        const T *const *in = reinterpret_cast<const T *const *>(srcs[e]);
        const VecSplit vs = vec_split(sizeof(T), nelems[e], &out, 1, in, K);
        if (!vs.vec) return hipErrorInvalidValue;  // many_route said MANY_BATCH
        ManySeg<T, K> &g = tab.seg[i];
        const size_t t0 = pc[i].tile0;
        const size_t left = vs.nvec > t0 * V ? vs.nvec - t0 * V : 0;
        g.nvec = left < pc[i].ntiles * V ? left : pc[i].ntiles * V;
        g.first = pc[i].first;
        if (t0 == 0) {
            g.out = out;
            for (int k = 0; k < K; k++) g.in[k] = in[k];
            g.head = vs.head;
            g.tail_start = vs.tail_start;
            g.nedge = vs.nedge;
        } else {
            // a continuation: no edges, pointers at its first tile (for_each_tile_run's rule)
            const size_t off = vs.head + t0 * V * W;
            g.out = out + off;
            for (int k = 0; k < K; k++) g.in[k] = in[k] + off;
            g_many_routes[6]++;
        }
    }
    g_many_routes[0] += (unsigned long long) np;
    g_many_routes[5]++;
    hipLaunchKernelGGL((combine_many_kernel<T, OP, K, OSGPU_MANY_U>), dim3((unsigned) blocks),
                       dim3(64 * K), 0, s, tab);
    return hipGetLastError();
}

template <typename T, int OP>
static hipError_t launch_many_op(int count, void *const *targets, const void *const *const *srcs,
                                 int nsrc, const size_t *nelems, hipStream_t s)
{
    constexpr size_t V = (size_t) 64 * OSGPU_MANY_U;
    // entries of the batch kernel: their workgroups; the others are launched
    // here, each on its own (independent arrays: the order is free)
    std::vector<size_t> tiles((size_t) count, 0);
    std::vector<uintptr_t> at((size_t) nsrc);
    for (int i = 0; i < count; i++) {
        if (nelems[i] == 0) continue;
        if (!targets[i] || !srcs[i]) return hipErrorInvalidValue;
        for (int k = 0; k < nsrc; k++) at[(size_t) k] = (uintptr_t) srcs[i][k];
        const rt::ManyRoute r = rt::many_route(sizeof(T), false, nsrc, nelems[i],
                                               (uintptr_t) targets[i], at.data());
        hipError_t e = hipSuccess;
        if (r == rt::MANY_BATCH) {
            T *out = static_cast<T *>(targets[i]);
            const VecSplit vs = vec_split(sizeof(T), nelems[i], &out, 1,
                                          reinterpret_cast<const T *const *>(srcs[i]), nsrc);
            tiles[(size_t) i] = rt::many_tiles(vs.nvec, V);
        } else if (r == rt::MANY_SHIFTED) {
            g_many_routes[1]++;
            e = launch_op<T, OP, true>(targets[i], srcs[i], nsrc, nelems[i], s);
        } else {
            g_many_routes[r == rt::MANY_COPY ? 4 : 3]++;
            e = launch_op<T, OP>(targets[i], srcs[i], nsrc, nelems[i], s);
        }
        if (e != hipSuccess) return e;
    }
    if (nsrc < 2 || nsrc > kMaxK) return hipSuccess;
    hipError_t err = hipSuccess;
    auto pack = [&](auto k) {
        constexpr int K = decltype(k)::value;
        rt::many_pack(tiles.data(), count, max_launch_threads() / (64 * K),
                      [&](const rt::ManyPiece *pc, int np, size_t blocks) {
                          err = launch_many_k<T, OP, K>(pc, np, blocks, targets, srcs, nelems, s);
                          return err == hipSuccess;
                      });
    };
    switch (nsrc) {
    case 2: pack(std::integral_constant<int, 2>{}); break;
    case 3: pack(std::integral_constant<int, 3>{}); break;
    case 4: pack(std::integral_constant<int, 4>{}); break;
    case 5: pack(std::integral_constant<int, 5>{}); break;
    case 6: pack(std::integral_constant<int, 6>{}); break;
    case 7: pack(std::integral_constant<int, 7>{}); break;
    default: pack(std::integral_constant<int, 8>{}); break;
    }
    return err;
}

hipError_t launch_combine_many(int type, int op, int count, void *const *targets,
                               const void *const *const *srcs, int nsrc, const size_t *nelems,
                               hipStream_t s)
{
    if (count < 0 || nsrc < 1 || (count > 0 && (!targets || !srcs || !nelems)))
        return hipErrorInvalidValue;
    if (type == T_LONGDOUBLE) {
        for (int i = 0; i < count; i++) {
            if (nelems[i] == 0) continue;
            if (!targets[i] || !srcs[i]) return hipErrorInvalidValue;
            g_many_routes[2]++;
            const hipError_t e = launch_longdouble(op, targets[i], srcs[i], nsrc, nelems[i], s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        return launch_many_op<typename decltype(t)::type, decltype(o)::value>(count, targets, srcs,
                                                                              nsrc, nelems, s);
    });
}

void many_route_counts(unsigned long long out[7])
{
    for (int i = 0; i < 7; i++) out[i] = g_many_routes[i].load();
}

}  // namespace osgpu
