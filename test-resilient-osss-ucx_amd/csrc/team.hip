// team.hip -- owner-computes reduce-to-all for a whole active set.
//
// The reference makes every PE pull every other PE's whole source
// (src/reductions.c:84-111): P*(P-1)*N elements cross the PE boundary and
// every PE reads P*N.  Here PE g (index g of the active set) owns the element
// shard [lo_g, hi_g) of ALL targets (targets are symmetric objects in
// OpenSHMEM 1.4): it reads shard g of the P sources once, computes the P
// per-PE results -- each in that PE's own fold order, op(op(x_q, x_0), x_1)
// ... skipping q (src/reductions.c:79-111) -- and writes shard g of every
// PE's target.  Per call the team moves 2*P*N*s bytes instead of
// P*(P+1)*N*s; across GPUs each PE exchanges (P-1)/P * N * s each way, the
// traffic of a reduce-scatter + all-gather, and the result stays bit-exact.
//
// Order-independent ops (every integer op) fold once and store P copies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <type_traits>

#include "kernel_common.hpp"
#include "loc_host.hpp"
#include "scan_host.hpp"
#include "wsum_host.hpp"

#pragma clang fp contract(off)

namespace osgpu {

template <typename T, int P>
struct TeamPtrs {
    const T *src[P];
    T *dst[P];
};

constexpr int kTeamBlock = 256;

// ---------------------------------------------------------------- shapes
// Tuning constants of the launch shapes.  Each was chosen by an in-process
// A/B on the same allocations (tools/team_inproc_ab.py); the records are
// cited here and in DESIGN_HISTORY.md.  The four left overridable with -D
// (tools/build_ab.sh) are the ones a round-6 A/B still builds.
//
// Above 4 members: U vectors per input per lane, G of them in flight per
// round.  U = 4 in two rounds of G = 2 (16 vectors of 16 B in flight per lane
// at 8 members) beat one round of U = G = 2 at P = 8 for every type: float
// 0.715 -> 0.786, complexf 0.723 -> 0.790 of 8 TB/s
// (profiles/r03_team_variants_interleaved.jsonl); U = G = 4 spills the
// 8-input complexf fold (0.45).
constexpr int kTeamU8 = 4;
constexpr int kTeamG8 = 2;  // complex sum; every type when members are remote
// ... for the real (non-complex) types on one GPU: one round of all U = 4
// vectors, 1.006x over 7 (type, op) pairs at 5-8 members
// (profiles/r05_team_p8_tile_ab.jsonl).  Not measured across GPUs (xGMI):
// calls with remote members keep G = kTeamG8 (TeamShape REMOTE).
#ifndef OSGPU_TEAM_G8R
#define OSGPU_TEAM_G8R 4
#endif
// the register-heavy folds above 4 members (complex products: 4-6 VALU
// temporaries per element per output) take rounds of kTeamGH vectors
constexpr int kTeamGH = 2;
// Above 4 members integer folds issue round r+1's loads before round r's
// folds and stores (two round buffers): +0.5-1 %; for floating-point folds
// the two buffers cost 0.2-0.4 of the rate in round 4 and 2-3 % once inlined
// (profiles/r04_team_type_op_sweep.jsonl, r05_team_p8_tile_ab.jsonl), so
// only integers pipeline.  Ordered folds above 4 members fold, check and
// store one output at a time (only one output vector live).
// Vectors per input per lane for 2 and for 3-4 members in the register form
// (all loaded before the first fold): U = 2 at 2 members ran 0.71-0.75
// against 0.77 with U = 4.
constexpr int kTeamU2 = 4;
constexpr int kTeamU4 = 4;
// The LDS-staged kernel (team_lds_kernel, one wave per member) serves
// OSGPU_TEAM_LDS_MIN_P .. OSGPU_TEAM_LDS_MAX_P members.  2 members: 1.03x
// over the register form for double sum, 1.00-1.07x for every (type, op)
// probed (profiles/r05_team_p2_ab.jsonl); 3-4 members ahead or equal on
// every box; 5-8 members: the register form's best (0.81 of 8 TB/s at 8) is
// above the LDS form's (0.75) (r04_team_place_3/4.jsonl).  Calls with
// remote members keep the round-4 range, 3-4 (TeamShape REMOTE): the 2-member
// A/B ran on one GPU only.
#ifndef OSGPU_TEAM_LDS_MIN_P
#define OSGPU_TEAM_LDS_MIN_P 2
#endif
#ifndef OSGPU_TEAM_LDS_MAX_P
#define OSGPU_TEAM_LDS_MAX_P 4
#endif
// 16-B vectors per lane per LDS tile: U = 1 (1 KiB per member per workgroup,
// round 6).  In one process on the same allocations against U = 2
// (tools/team_inproc_ab.py, profiles/r06_lds_u1_confirm_ab.jsonl: 6 (type,
// op) pairs x 2-4 members x 4 allocations) every pair's median was faster:
// 1.025x / 1.026x / 1.070x at 2 / 3 / 4 members overall (int xor and float
// prod 1.09x at 4, complex double prod 1.05-1.09x), lifting the 4-member
// kernel from 0.963 to 1.021 of the same-mix copy
// (profiles/r06_team_lds_u1_ab.jsonl: 1.04x / 1.00x / 1.09x for double
// sum).  Above 4 members it wins at 5, 6 and 8 for real types other than
// FP max/min (TeamShape kLds below) and loses at 7 and for complex types
// (0.72x for complex double prod at 8): those keep the register form.  (Round 5 had U = 2 over U = 4, 1.02-1.04x,
// r05_team_p34_ab.jsonl; LDS-DMA staging at 4 members 0.967-0.998x,
// r06_team_p4_ab.jsonl.)  The combine keeps U = 2: U = 1 there ran 0.966x.
#ifndef OSGPU_TEAM_LDS_U
#define OSGPU_TEAM_LDS_U 1
#endif

// Launch shape per (T, OP, P): U vectors per input per lane in rounds of G.
// REMOTE: some member's arrays live in another GPU's HBM (xGMI): the shapes
// last measured across GPUs (round 4) -- the register form at 2 members and
// rounds of kTeamG8 above 4.
template <typename T, int OP, int P, bool REMOTE = false>
struct TeamShape {
    static constexpr bool kComplex = std::is_same<T, cfloat>::value || std::is_same<T, cdouble>::value;
    static constexpr bool kHeavy = kComplex && OP == OP_PROD;
    static constexpr int U = P <= 2 ? kTeamU2 : (P <= 4 ? kTeamU4 : kTeamU8);
    static constexpr int G = P <= 4 ? U
                             : (kHeavy ? kTeamGH : ((kComplex || REMOTE) ? kTeamG8 : OSGPU_TEAM_G8R));
    static constexpr bool kPipe = P > 4 && U / G > 1 && std::is_integral<T>::value;
    static constexpr bool kPerOutput = P > 4;
    // the LDS form also at 5, 6 and 8 members for real types other than FP
    // max/min: in one process on the same allocations, 9 (type, op) cases x
    // 5 allocations, at 8 members every case ran faster (double sum 1.012x,
    // float sum 1.043x, int sum 1.085x, long xor 1.068x, short min 1.060x,
    // float prod 1.042x, double prod 1.110x, int max 1.090x, long sum
    // 1.042x; profiles/r06_team_lds8_ab.jsonl), at 5 and 6 members 1.058x
    // overall (cases 0.989-1.110x; r06_team_lds56_ab.jsonl); complex types
    // and FP max/min lost (0.72-0.98x, r06_team_lds_p58_ab.jsonl), and so
    // did every case at 7 members (7-wave workgroups, 0.78-0.99x).
    static constexpr bool kFpMinMax = (std::is_floating_point<T>::value || is_f16<T>::value) &&
                                      (OP == OP_MAX || OP == OP_MIN);
    // half_t / bf16_t: the LDS form at every member count above 4 too, for
    // every op, local and remote.  Eight elements per vector make the register
    // form's P outputs of one lane too large there (bf16_t max at 8 members:
    // 238 VGPRs, 2 waves per SIMD; sum at 7: the fold loop is not unrolled
    // and its arrays go to scratch), while a wave of the LDS form folds one
    // output.  The register form serves them at 2 remote members only.
    static constexpr bool kLds = is_f16<T>::value
                                     ? (REMOTE ? P >= 3 : P >= OSGPU_TEAM_LDS_MIN_P)
                                 : REMOTE ? (P >= 3 && P <= 4)
                                          : ((P >= OSGPU_TEAM_LDS_MIN_P && P <= OSGPU_TEAM_LDS_MAX_P) ||
                                             ((P == 5 || P == 6 || P == 8) && !kComplex && !kFpMinMax));
    static constexpr int kLdsU = OSGPU_TEAM_LDS_U;
    // the rounds g = 0, G, 2G, ... must tile [0, U) exactly, or the last
    // round reads and writes past the tile (and past nvec)
    static_assert(G >= 1 && G <= U && U % G == 0, "the round size must divide U");
};

// the remote shape differs from the local one (else the local kernel serves)
template <typename T, int OP, int P>
constexpr bool kRemoteDiffers = TeamShape<T, OP, P, true>::kLds != TeamShape<T, OP, P, false>::kLds ||
                                TeamShape<T, OP, P, true>::G != TeamShape<T, OP, P, false>::G;

// f(integral_constant<int, I>) for I = 0 .. N-1, unrolled by construction
// (a #pragma unroll on the round loop is dropped for the largest bodies)
template <int I, int N>
struct Rounds {
    template <typename F>
    __device__ __forceinline__ static void run(F &&f)
    {
        if constexpr (I < N) {
            f(std::integral_constant<int, I>{});
            Rounds<I + 1, N>::run(f);
        }
    }
};

// (An XCD-aware workgroup -> tile map -- XCD x streaming one contiguous run of
// tiles instead of tiles x, x + 8, ... -- ran slower at every member count
// over ten layouts, 0.853-0.954 against 0.886-0.978 of the same-mix copy,
// profiles/r05_team_layouts.jsonl: the identity map ships.)

// E: Elem<T, OP> (exact) or Fast<T, OP> (branch-free, elem_ops.hpp)
template <typename T, int OP, int P, bool ORDERED, typename E = Elem<T, OP>>
__device__ __forceinline__ void team_fold(const T (&x)[P], T (&r)[P])
{
    if (ORDERED) {
#pragma unroll
        for (int q = 0; q < P; q++) {
            T acc = x[q];
#pragma unroll
            for (int j = 0; j < P; j++)
                if (j != q) acc = E::f(acc, x[j]);
            r[q] = acc;
        }
    } else {
        T acc = x[0];
#pragma unroll
        for (int j = 1; j < P; j++) acc = E::f(acc, x[j]);
#pragma unroll
        for (int q = 0; q < P; q++) r[q] = acc;
    }
}

template <typename T, int OP, int P, bool ORDERED, bool REMOTE>
__global__ __launch_bounds__(kTeamBlock) void team_vec_kernel(TeamPtrs<T, P> a, size_t nvec,
                                                              size_t head, size_t tail_start,
                                                              int nedge, unsigned tm, unsigned tk)
{
    constexpr int W = 16 / sizeof(T);
    using S = TeamShape<T, OP, P, REMOTE>;
    constexpr int U = S::U;
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        T x[P], r[P];
#pragma unroll
        for (int p = 0; p < P; p++) x[p] = a.src[p][e];
        team_fold<T, OP, P, ORDERED>(x, r);
#pragma unroll
        for (int p = 0; p < P; p++) a.dst[p][e] = r[p];
    }
    // tile blockIdx.x * tm + tk (launch_team_tiles; tm = 1, tk = 0: tile blockIdx.x)
    const size_t t0 = ((size_t) blockIdx.x * tm + tk) * (kTeamBlock * U) + threadIdx.x;
    // fold one vector of every input into one vector of every output: the
    // branch-free fold first, the exact one only for a vector whose results
    // hold a NaN part (rare; elem_ops.hpp Fast) -- no branch per element, so
    // the tile's loads stay in flight ahead of the folds
    using F = Fast<T, OP>;
    auto fold_store = [&](Vec16<T> (&in)[P], size_t j) __attribute__((always_inline)) {
        if constexpr (ORDERED && S::kPerOutput) {
            // one output at a time: fold, check, store -- only one output
            // vector live beside the inputs
            Rounds<0, P>::run([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                Vec16<T> out;
                bool bad = false;
#pragma unroll
                for (int w = 0; w < W; w++) {
                    T acc = in[q].e[w];
#pragma unroll
                    for (int k = 0; k < P; k++)
                        if (k != q) acc = F::f(acc, in[k].e[w]);
                    out.e[w] = acc;
                    bad = bad || F::bad(acc);
                }
                if (F::kChecked && __builtin_expect(bad, 0)) {
#pragma unroll
                    for (int w = 0; w < W; w++) {
                        T acc = in[q].e[w];
#pragma unroll
                        for (int k = 0; k < P; k++)
                            if (k != q) acc = Elem<T, OP>::f(acc, in[k].e[w]);
                        out.e[w] = acc;
                    }
                }
                __builtin_nontemporal_store(out.v, reinterpret_cast<u32x4 *>(a.dst[q] + head) + j);
            });
            return;
        }
        Vec16<T> out[P];
        bool bad = false;
#pragma unroll
        for (int w = 0; w < W; w++) {
            T x[P], r[P];
#pragma unroll
            for (int p = 0; p < P; p++) x[p] = in[p].e[w];
            team_fold<T, OP, P, ORDERED, F>(x, r);
#pragma unroll
            for (int p = 0; p < P; p++) {
                out[p].e[w] = r[p];
                bad = bad || F::bad(r[p]);
            }
        }
        if (F::kChecked && __builtin_expect(bad, 0)) {
#pragma unroll
            for (int w = 0; w < W; w++) {
                T x[P], r[P];
#pragma unroll
                for (int p = 0; p < P; p++) x[p] = in[p].e[w];
                team_fold<T, OP, P, ORDERED>(x, r);
#pragma unroll
                for (int p = 0; p < P; p++) out[p].e[w] = r[p];
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++)
            __builtin_nontemporal_store(out[p].v, reinterpret_cast<u32x4 *>(a.dst[p] + head) + j);
    };
    if (t0 + (size_t) (U - 1) * kTeamBlock < nvec) {
        // whole tile: the loads of G vectors of every input are in flight
        // before the first fold, as in combine_vec_kernel -- P*G*16 B per
        // lane, not P*16 B per round trip.  G = U up to 4 inputs; above,
        // TeamShape's G (all 4*P at once spills the 8-input complex sum)
        constexpr int G = S::G;
        constexpr int R = U / G;
        auto load_round = [&](Vec16<T> (&in)[G][P], int g) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < G; u++)
#pragma unroll
                for (int p = 0; p < P; p++)
                    in[u][p].v = __builtin_nontemporal_load(
                        reinterpret_cast<const u32x4 *>(a.src[p] + head) + t0 +
                        (size_t) (g * G + u) * kTeamBlock);
        };
        if constexpr (S::kPipe) {
            // round r+1's loads go out before round r's stores
            Vec16<T> b0[G][P], b1[G][P];
            load_round(b0, 0);
            Rounds<0, R>::run([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                auto &cur = (r % 2 == 0) ? b0 : b1;
                auto &nxt = (r % 2 == 0) ? b1 : b0;
                if constexpr (r + 1 < R) load_round(nxt, r + 1);
#pragma unroll
                for (int u = 0; u < G; u++) fold_store(cur[u], t0 + (size_t) (r * G + u) * kTeamBlock);
            });
        } else {
            Rounds<0, R>::run([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                Vec16<T> in[G][P];
                load_round(in, r);
#pragma unroll
                for (int u = 0; u < G; u++) fold_store(in[u], t0 + (size_t) (r * G + u) * kTeamBlock);
            });
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t j = t0 + (size_t) u * kTeamBlock;
        if (j < nvec) {
            Vec16<T> in[P];
#pragma unroll
            for (int p = 0; p < P; p++)
                in[p].v = __builtin_nontemporal_load(
                    reinterpret_cast<const u32x4 *>(a.src[p] + head) + j);
            fold_store(in, j);
        }
    }
}

// x[k] of a compile-time-sized array at a wave-uniform runtime index
template <typename X, int P>
__device__ __forceinline__ X pick(const X (&x)[P], int k)
{
    X r = x[0];
#pragma unroll
    for (int p = 1; p < P; p++)
        if (k == p) r = x[p];
    return r;
}

// LDS-staged form: P waves per workgroup, a tile of 64*U 16-B vectors of
// every member.  Wave p streams member p's source tile into LDS (one read
// stream per wave, as the copy kernel); after the barrier wave q folds the
// tile of all P inputs from LDS in member q's order and streams member q's
// target tile (one write stream per wave).  HBM bytes as the register form
// (2*P*s per element); the LDS carries P reads of every staged byte.  (A
// persistent grid walking the tiles with two LDS buffers, the next tile's
// loads in flight during this one's folds, ran 2-17 % slower at 3-8
// members: profiles/r04_team_sweep_4.jsonl; two or four members per wave,
// fewer waves per workgroup, no faster: r04_team_place_3.jsonl.)
template <typename T, int OP, int P, bool ORDERED, int U>
__global__ __launch_bounds__(64 * P) void team_lds_kernel(TeamPtrs<T, P> a, size_t nvec,
                                                          size_t head, size_t tail_start,
                                                          int nedge, unsigned tm, unsigned tk)
{
    constexpr int W = 16 / sizeof(T);
    constexpr int V = 64 * U;  // vectors per member per tile
    __shared__ u32x4 tile[P][V];
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        T x[P], r[P];
#pragma unroll
        for (int p = 0; p < P; p++) x[p] = a.src[p][e];
        team_fold<T, OP, P, ORDERED>(x, r);
#pragma unroll
        for (int p = 0; p < P; p++) a.dst[p][e] = r[p];
    }
    // the member this wave stages and writes
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63);
    const u32x4 *src = reinterpret_cast<const u32x4 *>(pick(a.src, w) + head);
    u32x4 *dst = reinterpret_cast<u32x4 *>(pick(a.dst, w) + head);
    u32x4 v[U];
    auto load = [&](size_t t) {
        const size_t base = t * V;
        const bool whole = base + V <= nvec;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (whole || base + u * 64 + lane < nvec)
                v[u] = __builtin_nontemporal_load(src + base + u * 64 + lane);
    };
    using F = Fast<T, OP>;
    // member q's fold of element e: x[q] first, then the others ascending
    // (order-independent integer ops: ascending for every q)
    // the vectors [u0, u1) of the tile
    auto fold_store = [&](size_t t, int u0, int u1) {
        const size_t base = t * V;
        const bool whole = base + V <= nvec;
        Rounds<0, P>::run([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if (w != q) return;
#pragma unroll
            for (int u = u0; u < u1; u++) {
                if (!whole && base + u * 64 + lane >= nvec) continue;
                Vec16<T> in[P], out;
#pragma unroll
                for (int p = 0; p < P; p++) in[p].v = tile[p][u * 64 + lane];
                bool bad = false;
#pragma unroll
                for (int e = 0; e < W; e++) {
                    T acc = in[ORDERED ? q : 0].e[e];
#pragma unroll
                    for (int k = 0; k < P; k++)
                        if (k != (ORDERED ? q : 0)) acc = F::f(acc, in[k].e[e]);
                    out.e[e] = acc;
                    bad = bad || F::bad(acc);
                }
                if (F::kChecked && __builtin_expect(bad, 0)) {
#pragma unroll
                    for (int e = 0; e < W; e++) {
                        T acc = in[q].e[e];
#pragma unroll
                        for (int k = 0; k < P; k++)
                            if (k != q) acc = Elem<T, OP>::f(acc, in[k].e[e]);
                        out.e[e] = acc;
                    }
                }
                __builtin_nontemporal_store(out.v, dst + base + u * 64 + lane);
            }
        });
    };
    const size_t t = (size_t) blockIdx.x * tm + tk;
    load(t);
#pragma unroll
    for (int u = 0; u < U; u++) tile[w][u * 64 + lane] = v[u];
    __syncthreads();
    fold_store(t, 0, U);
}

template <typename T, int OP, int P, bool ORDERED>
__global__ __launch_bounds__(kTeamBlock) void team_scalar_kernel(TeamPtrs<T, P> a, size_t n,
                                                                 unsigned tm, unsigned tk)
{
    // tiles of kTeamBlock elements: blockIdx.x * tm + tk, then gridDim.x * tm further
    const size_t stride = (size_t) gridDim.x * tm * kTeamBlock;
    for (size_t i = ((size_t) blockIdx.x * tm + tk) * kTeamBlock + threadIdx.x; i < n;
         i += stride) {
        T x[P], r[P];
#pragma unroll
        for (int p = 0; p < P; p++) x[p] = a.src[p][i];
        team_fold<T, OP, P, ORDERED>(x, r);
#pragma unroll
        for (int p = 0; p < P; p++) a.dst[p][i] = r[p];
    }
}

// tiles of m members, this one k-th (launch_team_tiles)
struct Tiles {
    unsigned m, k;
    bool remote;  // some member's arrays are in another GPU's HBM
    // of `total` tiles, the ones this member folds (at least one block)
    size_t blocks(size_t total) const
    {
        const size_t b = total > k ? (total - k + m - 1) / m : 0;
        return b ? b : 1;
    }
};

// the callers' first np members, `off` elements in, as a table of N (the rest null)
template <typename T, int N>
static TeamPtrs<T, N> team_table(void *const *dsts, const void *const *srcs, int np, size_t off)
{
    TeamPtrs<T, N> a;
    for (int p = 0; p < N; p++) {
        a.src[p] = p < np ? static_cast<const T *>(srcs[p]) + off : nullptr;
        a.dst[p] = p < np ? static_cast<T *>(dsts[p]) + off : nullptr;
    }
    return a;
}

// `kernel` (a, nvec, head, tail_start, nedge, tail...) over the vectors of
// vs in tiles of V, this member's every tl.m-th one, one per workgroup of
// `threads`, in runs that are whole multiples of tl.m (for_each_tile_run):
// the first launch takes head, tail_start and the edges (member 0's first
// workgroup folds them), the others zeros and pointers shifted to their
// first tile.
template <typename T, int P, typename Kernel, typename... Tail>
static hipError_t launch_tile_runs(Kernel kernel, size_t V, unsigned threads, Tiles tl,
                                   void *const *dsts, const void *const *srcs, const VecSplit &vs,
                                   hipStream_t s, Tail... tail)
{
    constexpr int W = 16 / sizeof(T);
    return for_each_tile_run(vs.nvec, V, threads, tl.m, [&](size_t t0, size_t nt, size_t nv) {
        const bool first = t0 == 0;
        const TeamPtrs<T, P> a = team_table<T, P>(dsts, srcs, P, first ? 0 : vs.head + t0 * V * W);
        hipLaunchKernelGGL(kernel, dim3((unsigned) tl.blocks(nt)), dim3(threads), 0, s, a, nv,
                           first ? vs.head : (size_t) 0, first ? vs.tail_start : (size_t) 0,
                           first && tl.k == 0 ? vs.nedge : 0, tail...);
        return hipGetLastError();
    });
}
// the scan and the uniform reduce: every tile is this member's
constexpr Tiles kAllTiles{1, 0, false};

// `kernel` (a, np, n, tail...), element-granular over a table sized for
// kMaxTeam (pointers whose 16-byte phases differ)
template <typename T, typename Kernel, typename... Tail>
static hipError_t launch_elem_table(Kernel kernel, int P, void *const *dsts,
                                    const void *const *srcs, size_t n, hipStream_t s, Tail... tail)
{
    size_t blocks = (n + kTeamBlock - 1) / kTeamBlock;
    blocks = blocks > 8192 ? 8192 : blocks;
    hipLaunchKernelGGL(kernel, dim3((unsigned) blocks), dim3(kTeamBlock), 0, s,
                       (team_table<T, kMaxTeam>(dsts, srcs, P, 0)), P, n, tail...);
    return hipGetLastError();
}

template <typename T, int OP, int P, bool REMOTE>
static hipError_t team_launch_p(void *const *dsts, const void *const *srcs, size_t n,
                                Tiles tl, hipStream_t s)
{
    using S = TeamShape<T, OP, P, REMOTE>;
    // integer ops are order-independent (wrapping ring / lattice ops); every
    // floating-point op, min/max included (NaN, signed zero), is not
    constexpr bool ORDERED = !std::is_integral<T>::value;
    const VecSplit vs = vec_split(sizeof(T), n, srcs, P, dsts, P);
    if (!vs.vec) {
        size_t blocks = tl.blocks((n + kTeamBlock - 1) / kTeamBlock);
        blocks = blocks > 8192 ? 8192 : blocks;
        hipLaunchKernelGGL((team_scalar_kernel<T, OP, P, ORDERED>), dim3((unsigned) blocks),
                           dim3(kTeamBlock), 0, s, (team_table<T, P>(dsts, srcs, P, 0)), n, tl.m,
                           tl.k);
        return hipGetLastError();
    }
    if constexpr (S::kLds) {
        constexpr int UL = S::kLdsU;
        return launch_tile_runs<T, P>(team_lds_kernel<T, OP, P, ORDERED, UL>, (size_t) 64 * UL,
                                      64 * P, tl, dsts, srcs, vs, s, tl.m, tl.k);
    } else {  // (not instantiated where the LDS form is used)
        return launch_tile_runs<T, P>(team_vec_kernel<T, OP, P, ORDERED, REMOTE>,
                                      (size_t) kTeamBlock * S::U, kTeamBlock, tl, dsts, srcs, vs,
                                      s, tl.m, tl.k);
    }
}

// the remote shape only where it differs from the local one
template <typename T, int OP, int P>
static hipError_t team_launch_pr(void *const *d, const void *const *sr, size_t n, Tiles tl,
                                 hipStream_t s)
{
    if constexpr (kRemoteDiffers<T, OP, P>)
        if (tl.remote) return team_launch_p<T, OP, P, true>(d, sr, n, tl, s);
    return team_launch_p<T, OP, P, false>(d, sr, n, tl, s);
}

template <typename T, int OP>
static hipError_t team_launch_op(int P, void *const *d, const void *const *sr, size_t n,
                                 Tiles tl, hipStream_t s)
{
    return dispatch_members(P, hipErrorInvalidValue, [&](auto pc) {
        return team_launch_pr<T, OP, decltype(pc)::value>(d, sr, n, tl, s);
    });
}

hipError_t launch_team_tiles(int type, int op, int P, void *const *dsts, const void *const *srcs,
                             size_t n, int m, int k, hipStream_t s, bool remote)
{
    if (P < 2 || P > kMaxTeam || m < 1 || k < 0 || k >= m) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const Tiles tl{(unsigned) m, (unsigned) k, remote};
    if (type == T_LONGDOUBLE)
        return m == 1 ? launch_team_longdouble(op, P, dsts, srcs, n, s) : hipErrorNotSupported;
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        return team_launch_op<typename decltype(t)::type, decltype(o)::value>(P, dsts, srcs, n, tl, s);
    });
}

hipError_t launch_team(int type, int op, int P, void *const *dsts, const void *const *srcs,
                       size_t n, hipStream_t s, bool remote)
{
    return launch_team_tiles(type, op, P, dsts, srcs, n, 1, 0, s, remote);
}

// ------------------------------------------------------------ prefix scan
// osgpu_scan: member q of the set receives the fold of members 0..q
// (inclusive) or 0..q-1 (exclusive), ascending for every member.  The same
// owner-computes shape as above -- this member reads its shard of every
// source once and writes that shard of every target -- but one running fold
// serves every output: P - 1 operations per element, where the ordered team
// fold takes P (P - 1).  `excl` (0 / 1) is a kernel argument: wave-uniform,
// one instantiation serves both modes.  `ident`: the op's identity in every
// element of a vector (scan_host.hpp), stored to member 0 by an exclusive
// scan and never an operand.

// The scan of one element: x[q] of the first np members in, store(q, value)
// out, by the exact element ops.  N is the array's size; np <= N.
template <typename T, int OP, int N, typename St>
__device__ __forceinline__ void scan_elem(const T (&x)[N], int np, int excl, T ident, St &&store)
{
    T acc = x[0];
    store(0, excl ? ident : acc);
#pragma unroll
    for (int q = 1; q < N; q++) {
        if (q >= np) break;
        const T inc = Elem<T, OP>::f(acc, x[q]);
        store(q, excl ? acc : inc);
        acc = inc;
    }
}

// LDS-staged form, the shape of team_lds_kernel: P waves per workgroup, a
// tile of 64*U 16-B vectors per member.  Wave p streams member p's source
// tile into LDS; after the barrier wave q folds inputs 0 .. q - excl from LDS
// ascending and streams member q's target tile.  No input: the identity
// vector; one: a copy.  HBM bytes as the team kernel (2*P*s per element).
template <typename T, int OP, int P, int U>
__global__ __launch_bounds__(64 * P) void team_scan_lds_kernel(TeamPtrs<T, P> a, size_t nvec,
                                                               size_t head, size_t tail_start,
                                                               int nedge, int excl, u32x4 ident)
{
    constexpr int W = 16 / sizeof(T);
    constexpr int V = 64 * U;  // vectors per member per tile
    __shared__ u32x4 tile[P][V];
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        T x[P];
#pragma unroll
        for (int p = 0; p < P; p++) x[p] = a.src[p][e];
        Vec16<T> id;
        id.v = ident;
        scan_elem<T, OP>(x, P, excl, id.e[0], [&](int q, T r) { a.dst[q][e] = r; });
    }
    // the member this wave stages and writes
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63);
    const u32x4 *src = reinterpret_cast<const u32x4 *>(pick(a.src, w) + head);
    u32x4 *dst = reinterpret_cast<u32x4 *>(pick(a.dst, w) + head);
    const size_t base = (size_t) blockIdx.x * V;
    const bool whole = base + V <= nvec;
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        v[u] = u32x4{0, 0, 0, 0};
        if (whole || base + u * 64 + lane < nvec)
            v[u] = __builtin_nontemporal_load(src + base + u * 64 + lane);
    }
#pragma unroll
    for (int u = 0; u < U; u++) tile[w][u * 64 + lane] = v[u];
    __syncthreads();
    using F = Fast<T, OP>;
    const int nin = w + 1 - excl;  // inputs of this wave's output: 0 .. P
    Rounds<0, P + 1>::run([&](auto nc) {
        constexpr int N = decltype(nc)::value;
        if (nin != N) return;
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!whole && base + u * 64 + lane >= nvec) continue;
            Vec16<T> out;
            if constexpr (N == 0) {
                out.v = ident;
            } else if constexpr (N == 1) {
                out.v = tile[0][u * 64 + lane];
            } else {
                Vec16<T> in[N];
#pragma unroll
                for (int p = 0; p < N; p++) in[p].v = tile[p][u * 64 + lane];
                // the branch-free fold first, the exact one only for a vector
                // whose result holds a NaN part (elem_ops.hpp Fast)
                bool bad = false;
#pragma unroll
                for (int e = 0; e < W; e++) {
                    T acc = in[0].e[e];
#pragma unroll
                    for (int k = 1; k < N; k++) acc = F::f(acc, in[k].e[e]);
                    out.e[e] = acc;
                    bad = bad || F::bad(acc);
                }
                if (F::kChecked && __builtin_expect(bad, 0)) {
#pragma unroll
                    for (int e = 0; e < W; e++) {
                        T acc = in[0].e[e];
#pragma unroll
                        for (int k = 1; k < N; k++) acc = Elem<T, OP>::f(acc, in[k].e[e]);
                        out.e[e] = acc;
                    }
                }
            }
            __builtin_nontemporal_store(out.v, dst + base + u * 64 + lane);
        }
    });
}

// element-granular form (pointers whose 16-byte phases differ): np members
// of a table sized for kMaxTeam, so one instantiation serves every P
template <typename T, int OP>
__global__ __launch_bounds__(kTeamBlock) void team_scan_scalar_kernel(TeamPtrs<T, kMaxTeam> a,
                                                                      int np, size_t n, int excl,
                                                                      u32x4 ident)
{
    Vec16<T> id;
    id.v = ident;
    const size_t stride = (size_t) gridDim.x * kTeamBlock;
    for (size_t i = (size_t) blockIdx.x * kTeamBlock + threadIdx.x; i < n; i += stride) {
        T x[kMaxTeam];
#pragma unroll
        for (int p = 0; p < kMaxTeam; p++)
            if (p < np) x[p] = a.src[p][i];
        scan_elem<T, OP>(x, np, excl, id.e[0], [&](int q, T r) { a.dst[q][i] = r; });
    }
}

// byte k % s (s = 2, 4, 8 or 16) of a 16-byte pattern, without indexing registers
__device__ __forceinline__ unsigned pattern_byte(u32x4 pat, size_t k, unsigned s)
{
    const unsigned i = (unsigned) (k % s), wd = i >> 2;
    const unsigned word = wd == 0 ? pat.x : (wd == 1 ? pat.y : (wd == 2 ? pat.z : pat.w));
    return (word >> (8 * (i & 3))) & 0xffu;
}

// The identity fill: nbytes from dst, byte k = elem's byte k % s.  Bytes
// [0, head) up to the first 16-byte boundary and the bytes behind the last
// whole vector go one per lane of workgroup 0 (fewer than 32); the nvec
// vectors between are 16-byte stores of `vec`, the pattern as it falls on a
// 16-byte boundary.
__global__ __launch_bounds__(kTeamBlock) void scan_fill_kernel(unsigned char *dst, size_t nbytes,
                                                               size_t head, size_t nvec, u32x4 vec,
                                                               u32x4 elem, unsigned s)
{
    const size_t tail_start = head + nvec * 16;
    const size_t nedge = head + (nbytes - tail_start);
    if (blockIdx.x == 0 && threadIdx.x < nedge) {
        const size_t k = edge_index(head, tail_start);
        dst[k] = (unsigned char) pattern_byte(elem, k, s);
    }
    const size_t stride = (size_t) gridDim.x * kTeamBlock;
    u32x4 *out = reinterpret_cast<u32x4 *>(dst + head);
    for (size_t j = (size_t) blockIdx.x * kTeamBlock + threadIdx.x; j < nvec; j += stride)
        __builtin_nontemporal_store(vec, out + j);
}

// 16 bytes of the pattern of period s starting at its byte `at`
static u32x4 pattern_vec(const unsigned char *elem, size_t s, size_t at)
{
    unsigned char b[16];
    for (size_t i = 0; i < 16; i++) b[i] = elem[(at + i) % s];
    u32x4 v;
    memcpy(&v, b, 16);
    return v;
}

hipError_t launch_scan_fill(int type, int op, void *dst, size_t n, hipStream_t s)
{
    unsigned char id[16];
    const size_t es = rt::scan_identity(type, op, id);
    if (!es) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const size_t nbytes = n * es, phase = (uintptr_t) dst & 15;
    size_t head = phase ? 16 - phase : 0;
    if (head > nbytes) head = nbytes;
    const size_t nvec = (nbytes - head) / 16;
    size_t blocks = (nvec + kTeamBlock - 1) / kTeamBlock;
    blocks = blocks > 8192 ? 8192 : (blocks ? blocks : 1);
    hipLaunchKernelGGL(scan_fill_kernel, dim3((unsigned) blocks), dim3(kTeamBlock), 0, s,
                       static_cast<unsigned char *>(dst), nbytes, head, nvec,
                       pattern_vec(id, es, head), pattern_vec(id, es, 0), (unsigned) es);
    return hipGetLastError();
}

template <typename T, int OP>
static hipError_t scan_launch_op(int P, void *const *d, const void *const *sr, size_t n, int excl,
                                 u32x4 ident, hipStream_t s)
{
    const VecSplit vs = vec_split(sizeof(T), n, sr, P, d, P);
    if (!vs.vec)
        return launch_elem_table<T>(team_scan_scalar_kernel<T, OP>, P, d, sr, n, s, excl, ident);
    return dispatch_members(P, hipErrorInvalidValue, [&](auto pc) {
        constexpr int PP = decltype(pc)::value;
        constexpr int UL = OSGPU_TEAM_LDS_U;
        return launch_tile_runs<T, PP>(team_scan_lds_kernel<T, OP, PP, UL>, (size_t) 64 * UL,
                                       64 * PP, kAllTiles, d, sr, vs, s, excl, ident);
    });
}

hipError_t launch_team_scan(int type, int op, int exclusive, int P, void *const *dsts,
                            const void *const *srcs, size_t n, hipStream_t s)
{
    if (P < 2 || P > kMaxTeam || exclusive < 0 || exclusive > 1) return hipErrorInvalidValue;
    if (type == T_LONGDOUBLE) return hipErrorNotSupported;
    unsigned char id[16];
    const size_t es = rt::scan_identity(type, op, id);
    if (!es) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const u32x4 ident = pattern_vec(id, es, 0);
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        return scan_launch_op<typename decltype(t)::type, decltype(o)::value>(P, dsts, srcs, n,
                                                                              exclusive, ident, s);
    });
}

// ----------------------------------------------------- uniform reduce-to-all
// osgpu_reduce_uniform: every member receives the ONE ascending fold
// srcs[0] op srcs[1] op ... op srcs[P-1] -- the last member's inclusive scan,
// member 0's reduce-to-all -- so all P targets hold the same bytes.  The same
// owner-computes shape and the same 2*P*s HBM bytes per element as above.
//
// The scan kernel lets wave q refold inputs 0..q from LDS: P (P - 1) / 2
// wave-level folds per 64 vectors (VALU issue is per wave whatever the lane
// mask).  Here a tile is P sub-tiles of 64 vectors per member and each
// sub-tile is folded ONCE:
//   stage  wave p streams member p's P*64 vectors into LDS, its P loads in
//          flight before the first LDS write (one read stream per wave);
//   fold   wave w folds sub-tile w, one vector per lane, the P inputs read
//          from LDS ascending; the result overwrites row 0 of sub-tile w,
//          which no other wave reads;
//   write  wave w streams the tile's P*64 result vectors (row 0) to member
//          w's target (one write stream per wave).
// LDS: P * P * 64 * 16 B = P^2 KiB a workgroup, 64 KiB at 8 members.  Every
// wave reaches both barriers whatever part of the tile lies beyond nvec: a
// last tile of 65 vectors leaves waves 2..P-1 nothing to fold, yet they have
// targets to write.

// the one ascending fold of an element by the exact ops
template <typename T, int OP, int P>
__device__ __forceinline__ T uniform_elem(const T (&x)[P])
{
    T acc = x[0];
#pragma unroll
    for (int p = 1; p < P; p++) acc = Elem<T, OP>::f(acc, x[p]);
    return acc;
}

constexpr int kUniformSub = 64;  // vectors per sub-tile: one per lane of the folding wave

template <typename T, int OP, int P>
__global__ __launch_bounds__(64 * P) void team_uniform_lds_kernel(TeamPtrs<T, P> a, size_t nvec,
                                                                  size_t head, size_t tail_start,
                                                                  int nedge)
{
    constexpr int W = 16 / sizeof(T);
    constexpr int V = kUniformSub * P;  // vectors per member per tile
    __shared__ u32x4 tile[P][V];
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        T x[P];
#pragma unroll
        for (int p = 0; p < P; p++) x[p] = a.src[p][e];
        const T r = uniform_elem<T, OP, P>(x);
#pragma unroll
        for (int p = 0; p < P; p++) a.dst[p][e] = r;
    }
    // the member this wave stages and writes, the sub-tile it folds
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63);
    const u32x4 *src = reinterpret_cast<const u32x4 *>(pick(a.src, w) + head);
    u32x4 *dst = reinterpret_cast<u32x4 *>(pick(a.dst, w) + head);
    const size_t base = (size_t) blockIdx.x * V;
    const bool whole = base + V <= nvec;
    // (a branch per load would merge the P vectors at every join: 229 VGPRs
    // at 8 members.)  A partial tile loads vector min(j, nvec - 1) in place of
    // a vector j beyond nvec -- inside the array, never folded -- so its P
    // loads are unconditional too; no tile starts at or beyond nvec but the
    // one of a call without whole vectors, which loads nothing.
    if (whole || base < nvec) {
        const size_t last = nvec - 1 - base;  // of this tile's vectors, when partial
        u32x4 v[P];
#pragma unroll
        for (int u = 0; u < P; u++) {
            const size_t j = (size_t) (u * kUniformSub + lane);
            v[u] = __builtin_nontemporal_load(src + base + (whole || j < last ? j : last));
        }
#pragma unroll
        for (int u = 0; u < P; u++) tile[w][u * kUniformSub + lane] = v[u];
    }
    __syncthreads();
    const int mine = w * kUniformSub + lane;
    if (whole || base + mine < nvec) {
        using F = Fast<T, OP>;
        Vec16<T> in[P], out;
#pragma unroll
        for (int p = 0; p < P; p++) in[p].v = tile[p][mine];
        // the branch-free fold first, the exact one only for a vector whose
        // result holds a NaN part (elem_ops.hpp Fast)
        bool bad = false;
#pragma unroll
        for (int e = 0; e < W; e++) {
            T acc = in[0].e[e];
#pragma unroll
            for (int k = 1; k < P; k++) acc = F::f(acc, in[k].e[e]);
            out.e[e] = acc;
            bad = bad || F::bad(acc);
        }
        if (F::kChecked && __builtin_expect(bad, 0)) {
#pragma unroll
            for (int e = 0; e < W; e++) {
                T acc = in[0].e[e];
#pragma unroll
                for (int k = 1; k < P; k++) acc = Elem<T, OP>::f(acc, in[k].e[e]);
                out.e[e] = acc;
            }
        }
        tile[0][mine] = out.v;
    }
    __syncthreads();
    if (whole) {
        u32x4 r[P];
#pragma unroll
        for (int u = 0; u < P; u++) r[u] = tile[0][u * kUniformSub + lane];
#pragma unroll
        for (int u = 0; u < P; u++)
            __builtin_nontemporal_store(r[u], dst + base + u * kUniformSub + lane);
        return;
    }
#pragma unroll
    for (int u = 0; u < P; u++)
        if (base + u * kUniformSub + lane < nvec)
            __builtin_nontemporal_store(tile[0][u * kUniformSub + lane],
                                        dst + base + u * kUniformSub + lane);
}

// element-granular form (pointers whose 16-byte phases differ): np members
// of a table sized for kMaxTeam, so one instantiation serves every P
template <typename T, int OP>
__global__ __launch_bounds__(kTeamBlock) void team_uniform_scalar_kernel(TeamPtrs<T, kMaxTeam> a,
                                                                         int np, size_t n)
{
    const size_t stride = (size_t) gridDim.x * kTeamBlock;
    for (size_t i = (size_t) blockIdx.x * kTeamBlock + threadIdx.x; i < n; i += stride) {
        T acc = a.src[0][i];
#pragma unroll
        for (int p = 1; p < kMaxTeam; p++)
            if (p < np) acc = Elem<T, OP>::f(acc, a.src[p][i]);
#pragma unroll
        for (int q = 0; q < kMaxTeam; q++)
            if (q < np) a.dst[q][i] = acc;
    }
}

template <typename T, int OP>
static hipError_t uniform_launch_op(int P, void *const *d, const void *const *sr, size_t n,
                                    hipStream_t s)
{
    const VecSplit vs = vec_split(sizeof(T), n, sr, P, d, P);
    if (!vs.vec) return launch_elem_table<T>(team_uniform_scalar_kernel<T, OP>, P, d, sr, n, s);
    return dispatch_members(P, hipErrorInvalidValue, [&](auto pc) {
        constexpr int PP = decltype(pc)::value;
        return launch_tile_runs<T, PP>(team_uniform_lds_kernel<T, OP, PP>,
                                       (size_t) kUniformSub * PP, 64 * PP, kAllTiles, d, sr, vs, s);
    });
}

hipError_t launch_team_uniform(int type, int op, int P, void *const *dsts, const void *const *srcs,
                               size_t n, hipStream_t s)
{
    if (P < 2 || P > kMaxTeam) return hipErrorInvalidValue;
    if (type == T_LONGDOUBLE) return launch_uniform_longdouble(op, P, dsts, srcs, n, s);
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        if (n == 0) return hipSuccess;
        return uniform_launch_op<typename decltype(t)::type, decltype(o)::value>(P, dsts, srcs, n,
                                                                                 s);
    });
}

// ------------------------------------------- max / min with location
// osgpu_reduce_loc: the uniform reduce's ONE ascending fold carrying a second
// stream -- every element is a pair (value, 32-bit index), folded by
// elem_ops.hpp LocStep, and both results go to ndst targets (all P members'
// in the owner-computes form, the caller's alone in the pull form).  The
// kernel reads P value streams and up to P index streams whose elements
// differ in size, so a lane step is a GROUP of G = max(16 / sizeof(T), 4)
// elements: whole 16-byte vectors of both streams (loc_host.hpp loc_group).
//
// Register form, no LDS and no barrier: the fold of a group needs nothing
// from another lane, and the LDS tile of team_uniform_lds_kernel costs it
// 3-16 % on HBM-bound types.  A lane issues the
// P * (NV + NI) loads of its group -- 24 at 8 members -- before the first
// use, folds G elements (a compare pair and two selects per member), and
// stores ndst * (NV + NI) vectors.  One group per lane and ONE bounds test
// around the whole body: a lane beyond the last group leaves, so no load is
// conditional and nothing merges at a join (the uniform kernel's clamped
// index is not needed: at most 76 VGPRs at 8 members, 6 waves per SIMD or
// more, no scratch).
// Index sources are a template parameter: kLocConst reads no index stream at
// all (every element of member p carries a.member[p]); kLocFeedback reads
// input 0's only (the pull form's chunks after the first, whose input 0 is
// the pair folded so far).
constexpr int kLocBlock = 256;  // groups per tile: one per lane
enum LocMode { kLocConst = 0, kLocStreams = 1, kLocFeedback = 2 };

template <typename T, int P>
struct LocPtrs {
    const T *vsrc[P];
    const int32_t *lsrc[P];
    T *vdst[P];
    int32_t *ldst[P];
    int32_t member[P];
};

template <int MODE>
__device__ __forceinline__ constexpr bool loc_streamed(int p)
{
    return MODE == kLocStreams || (MODE == kLocFeedback && p == 0);
}

template <typename T, int OP, int P, int MODE>
__global__ __launch_bounds__(kLocBlock) void team_loc_vec_kernel(LocPtrs<T, P> a, int ndst,
                                                                 size_t ngroups, size_t head,
                                                                 size_t tail_start, int nedge)
{
    constexpr int G = sizeof(T) == 2 ? 8 : 4;  // elements per group
    constexpr int W = 16 / sizeof(T);          // values per vector
    constexpr int NV = G / W, NI = G / 4;      // vectors per group and stream
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        T v = a.vsrc[0][e];
        int32_t i = loc_streamed<MODE>(0) ? a.lsrc[0][e] : a.member[0];
#pragma unroll
        for (int p = 1; p < P; p++)
            LocStep<T, OP>::f(v, i, a.vsrc[p][e], loc_streamed<MODE>(p) ? a.lsrc[p][e] : a.member[p]);
#pragma unroll
        for (int q = 0; q < P; q++)
            if (q < ndst) {
                a.vdst[q][e] = v;
                a.ldst[q][e] = i;
            }
    }
    const size_t j = (size_t) blockIdx.x * kLocBlock + threadIdx.x;
    if (j >= ngroups) return;
    Vec16<T> val[P][NV];
    Vec16<int32_t> loc[P][NI];
#pragma unroll
    for (int p = 0; p < P; p++) {
#pragma unroll
        for (int u = 0; u < NV; u++)
            val[p][u].v = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4 *>(a.vsrc[p] + head) + j * NV + u);
        if (loc_streamed<MODE>(p)) {
#pragma unroll
            for (int u = 0; u < NI; u++)
                loc[p][u].v = __builtin_nontemporal_load(
                    reinterpret_cast<const u32x4 *>(a.lsrc[p] + head) + j * NI + u);
        }
    }
    Vec16<T> rv[NV];
    Vec16<int32_t> ri[NI];
#pragma unroll
    for (int e = 0; e < G; e++) {
        T v = val[0][e / W].e[e % W];
        int32_t i = loc_streamed<MODE>(0) ? loc[0][e / 4].e[e % 4] : a.member[0];
#pragma unroll
        for (int p = 1; p < P; p++)
            LocStep<T, OP>::f(v, i, val[p][e / W].e[e % W],
                              loc_streamed<MODE>(p) ? loc[p][e / 4].e[e % 4] : a.member[p]);
        rv[e / W].e[e % W] = v;
        ri[e / 4].e[e % 4] = i;
    }
#pragma unroll
    for (int q = 0; q < P; q++) {
        if (q >= ndst) break;
#pragma unroll
        for (int u = 0; u < NV; u++)
            __builtin_nontemporal_store(rv[u].v,
                                        reinterpret_cast<u32x4 *>(a.vdst[q] + head) + j * NV + u);
#pragma unroll
        for (int u = 0; u < NI; u++)
            __builtin_nontemporal_store(ri[u].v,
                                        reinterpret_cast<u32x4 *>(a.ldst[q] + head) + j * NI + u);
    }
}

// element-granular form (no common head aligns every pointer): np members of
// a table sized for kMaxTeam, so one instantiation per mode serves every P
template <typename T, int OP, int MODE>
__global__ __launch_bounds__(kTeamBlock) void team_loc_scalar_kernel(LocPtrs<T, kMaxTeam> a, int np,
                                                                     int ndst, size_t n)
{
    const size_t stride = (size_t) gridDim.x * kTeamBlock;
    for (size_t k = (size_t) blockIdx.x * kTeamBlock + threadIdx.x; k < n; k += stride) {
        T v = a.vsrc[0][k];
        int32_t i = loc_streamed<MODE>(0) ? a.lsrc[0][k] : a.member[0];
#pragma unroll
        for (int p = 1; p < kMaxTeam; p++)
            if (p < np)
                LocStep<T, OP>::f(v, i, a.vsrc[p][k],
                                  loc_streamed<MODE>(p) ? a.lsrc[p][k] : a.member[p]);
#pragma unroll
        for (int q = 0; q < kMaxTeam; q++)
            if (q < ndst) {
                a.vdst[q][k] = v;
                a.ldst[q][k] = i;
            }
    }
}

template <typename T, int P>
static LocPtrs<T, P> loc_ptrs(int np, int ndst, void *const *vd, int *const *ld,
                              const void *const *vs, const int *const *ls, const int *member,
                              int mode, size_t off)
{
    LocPtrs<T, P> a;
    for (int p = 0; p < P; p++) {
        const bool streamed = mode == kLocStreams || (mode == kLocFeedback && p == 0);
        a.vsrc[p] = p < np ? static_cast<const T *>(vs[p]) + off : nullptr;
        a.lsrc[p] = p < np && streamed ? ls[p] + off : nullptr;
        a.vdst[p] = p < ndst ? static_cast<T *>(vd[p]) + off : nullptr;
        a.ldst[p] = p < ndst ? ld[p] + off : nullptr;
        a.member[p] = p < np && !streamed ? member[p] : 0;
    }
    return a;
}

template <typename T, int OP, int MODE>
static hipError_t loc_launch_mode(int P, int ndst, void *const *vd, int *const *ld,
                                  const void *const *vs, const int *const *ls, const int *member,
                                  size_t n, hipStream_t s)
{
    const void *vals[2 * kMaxTeam], *locs[2 * kMaxTeam];
    int nv = 0, nl = 0;
    for (int p = 0; p < P; p++) vals[nv++] = vs[p];
    for (int q = 0; q < ndst; q++) vals[nv++] = vd[q], locs[nl++] = ld[q];
    for (int p = 0; p < P; p++)
        if (MODE == kLocStreams || (MODE == kLocFeedback && p == 0)) locs[nl++] = ls[p];
    const rt::LocSplit sp = rt::loc_split(sizeof(T), n, vals, nv, locs, nl);
    if (!sp.vec) {
        size_t blocks = (n + kTeamBlock - 1) / kTeamBlock;
        blocks = blocks > 8192 ? 8192 : blocks;
        hipLaunchKernelGGL((team_loc_scalar_kernel<T, OP, MODE>), dim3((unsigned) blocks),
                           dim3(kTeamBlock), 0, s,
                           loc_ptrs<T, kMaxTeam>(P, ndst, vd, ld, vs, ls, member, MODE, 0), P, ndst,
                           n);
        return hipGetLastError();
    }
    constexpr size_t G = sizeof(T) == 2 ? 8 : 4;
    auto run = [&](auto pc) {
        constexpr int PP = decltype(pc)::value;
        // one tile of kLocBlock groups per workgroup, in runs below the launch
        // limit: the first launch takes the edges, the others shifted pointers
        return for_each_tile_run(sp.ngroups, kLocBlock, kLocBlock, 1,
                                 [&](size_t t0, size_t nt, size_t ng) {
            const size_t off = t0 == 0 ? 0 : sp.head + t0 * kLocBlock * G;
            hipLaunchKernelGGL((team_loc_vec_kernel<T, OP, PP, MODE>), dim3((unsigned) nt),
                               dim3(kLocBlock), 0, s,
                               loc_ptrs<T, PP>(PP, ndst, vd, ld, vs, ls, member, MODE, off), ndst,
                               ng, t0 == 0 ? sp.head : (size_t) 0,
                               t0 == 0 ? sp.tail_start : (size_t) 0, t0 == 0 ? sp.nedge : 0);
            return hipGetLastError();
        });
    };
    if (P == 1) return run(std::integral_constant<int, 1>{});
    return dispatch_members(P, hipErrorInvalidValue, run);
}

hipError_t launch_team_loc(int type, int op, int P, int ndst, void *const *val_dsts,
                           int *const *loc_dsts, const void *const *val_srcs,
                           const int *const *loc_srcs, const int *member_locs, size_t n,
                           hipStream_t s)
{
    if (P < 1 || P > kMaxTeam || (ndst != 1 && ndst != P)) return hipErrorInvalidValue;
    if (op != OP_MAX && op != OP_MIN) return hipErrorInvalidValue;
    if (!val_dsts || !loc_dsts || !val_srcs || (!loc_srcs && !member_locs))
        return hipErrorInvalidValue;
    int mode = kLocConst;
    if (loc_srcs && loc_srcs[0]) mode = P == 1 || loc_srcs[1] ? kLocStreams : kLocFeedback;
    if (mode == kLocFeedback && !member_locs) return hipErrorInvalidValue;
    return dispatch_type_op(type, op, hipErrorInvalidValue, [&](auto t, auto o) {
        using T = typename decltype(t)::type;
        constexpr int OP = decltype(o)::value;
        constexpr bool kOrdered = std::is_integral<T>::value || std::is_floating_point<T>::value ||
                                  is_f16<T>::value;
        if constexpr (kOrdered && (OP == OP_MAX || OP == OP_MIN)) {
            if (n == 0) return hipSuccess;
            switch (mode) {
            case kLocConst:
                return loc_launch_mode<T, OP, kLocConst>(P, ndst, val_dsts, loc_dsts, val_srcs,
                                                         loc_srcs, member_locs, n, s);
            case kLocStreams:
                return loc_launch_mode<T, OP, kLocStreams>(P, ndst, val_dsts, loc_dsts, val_srcs,
                                                           loc_srcs, member_locs, n, s);
            default:
                return loc_launch_mode<T, OP, kLocFeedback>(P, ndst, val_dsts, loc_dsts, val_srcs,
                                                            loc_srcs, member_locs, n, s);
            }
        } else {
            return hipErrorInvalidValue;
        }
    });
}

// ------------------------------------------- float-accumulated 16-bit sum
// osgpu_reduce_wsum: the uniform reduce's ONE ascending fold of half_t /
// bf16_t sources in a FLOAT accumulator, narrowed once (elem_ops.hpp
// WsumStep), stored to ndst targets of the source's type or of float.  The
// shape of team_loc_vec_kernel: a register form, no LDS and no barrier, one
// GROUP of 8 elements per lane -- one 16-byte vector of every 16-bit stream,
// two of every float stream (the carry, float targets) -- and ONE bounds test
// around the body, so no load is conditional.  A lane issues its P (+ 2)
// loads before the first use, widens (v_cvt_f32_f16 / a shift), folds with
// P - 1 (+ 1) float adds per element, narrows once and stores ndst * (1 or 2)
// vectors.
// The NaN rule stays off the streaming path: a NaN, once met or made, stays
// through every later add, so the accumulator is a NaN at the end exactly when
// some step met one; each element's final accumulator is tested once and only
// such an element is refolded by the exact steps.
// CARRY: the accumulator starts at a float array's element (an earlier
// chunk's result) and srcs[0] takes an add like every other member.  With a
// float target and ndst = 1 the target may be the carry itself: a lane reads
// its group before it stores it.
constexpr int kWsumBlock = 256;  // groups per tile: one per lane

template <typename T, typename OUT, int P>
struct WsumPtrs {
    const T *src[P];
    OUT *dst[P];
    const float *carry;
};

// one element by the exact steps
template <typename T, typename OUT, int P, bool CARRY>
__device__ __forceinline__ OUT wsum_elem(const T (&x)[P], int np, float c)
{
    using S = WsumStep<T>;
    float acc = CARRY ? S::add(c, x[0]) : S::widen(x[0]);
#pragma unroll
    for (int p = 1; p < P; p++)
        if (p < np) acc = S::add(acc, x[p]);
    OUT r;
    S::out(acc, r);
    return r;
}

template <typename T, typename OUT, int P, bool CARRY>
__global__ __launch_bounds__(kWsumBlock) void team_wsum_vec_kernel(WsumPtrs<T, OUT, P> a, int ndst,
                                                                   size_t ngroups, size_t head,
                                                                   size_t tail_start, int nedge)
{
    constexpr int G = 8;                  // elements per group
    constexpr int NO = G * sizeof(OUT) / 16;  // vectors per group of a target: 1 or 2
    constexpr int WO = 16 / sizeof(OUT);
    using S = WsumStep<T>;
    if (blockIdx.x == 0 && (int) threadIdx.x < nedge) {
        const size_t e = edge_index(head, tail_start);
        T x[P];
#pragma unroll
        for (int p = 0; p < P; p++) x[p] = a.src[p][e];
        const OUT r = wsum_elem<T, OUT, P, CARRY>(x, P, CARRY ? a.carry[e] : 0.0f);
#pragma unroll
        for (int q = 0; q < P; q++)
            if (q < ndst) a.dst[q][e] = r;
    }
    const size_t j = (size_t) blockIdx.x * kWsumBlock + threadIdx.x;
    if (j >= ngroups) return;
    Vec16<T> in[P];
    Vec16<float> cv[2];
#pragma unroll
    for (int p = 0; p < P; p++)
        in[p].v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a.src[p] + head) + j);
    if (CARRY) {
#pragma unroll
        for (int u = 0; u < 2; u++)
            cv[u].v = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4 *>(a.carry + head) + j * 2 + u);
    }
    Vec16<OUT> out[NO];
#pragma unroll
    for (int e = 0; e < G; e++) {
        float acc = S::widen_fast(in[0].e[e]);
        if (CARRY) acc = cv[e / 4].e[e % 4] + acc;
#pragma unroll
        for (int p = 1; p < P; p++) acc = acc + S::widen_fast(in[p].e[e]);
        if (__builtin_expect(acc != acc, 0)) {
            T x[P];
#pragma unroll
            for (int p = 0; p < P; p++) x[p] = in[p].e[e];
            out[e / WO].e[e % WO] =
                wsum_elem<T, OUT, P, CARRY>(x, P, CARRY ? cv[e / 4].e[e % 4] : 0.0f);
        } else {
            S::out(acc, out[e / WO].e[e % WO]);
        }
    }
#pragma unroll
    for (int q = 0; q < P; q++) {
        if (q >= ndst) break;
#pragma unroll
        for (int u = 0; u < NO; u++)
            __builtin_nontemporal_store(out[u].v,
                                        reinterpret_cast<u32x4 *>(a.dst[q] + head) + j * NO + u);
    }
}

// element-granular form (no common head aligns every pointer): np sources of
// a table sized for kMaxTeam, so one instantiation serves every P
template <typename T, typename OUT, bool CARRY>
__global__ __launch_bounds__(kTeamBlock) void team_wsum_scalar_kernel(WsumPtrs<T, OUT, kMaxTeam> a,
                                                                      int np, int ndst, size_t n)
{
    const size_t stride = (size_t) gridDim.x * kTeamBlock;
    for (size_t k = (size_t) blockIdx.x * kTeamBlock + threadIdx.x; k < n; k += stride) {
        T x[kMaxTeam];
#pragma unroll
        for (int p = 0; p < kMaxTeam; p++) x[p] = p < np ? a.src[p][k] : T{0};
        const OUT r = wsum_elem<T, OUT, kMaxTeam, CARRY>(x, np, CARRY ? a.carry[k] : 0.0f);
#pragma unroll
        for (int q = 0; q < kMaxTeam; q++)
            if (q < ndst) a.dst[q][k] = r;
    }
}

template <typename T, typename OUT, int P>
static WsumPtrs<T, OUT, P> wsum_ptrs(int np, int ndst, void *const *dsts, const void *const *srcs,
                                     const float *carry, size_t off)
{
    WsumPtrs<T, OUT, P> a;
    for (int p = 0; p < P; p++) {
        a.src[p] = p < np ? static_cast<const T *>(srcs[p]) + off : nullptr;
        a.dst[p] = p < ndst ? static_cast<OUT *>(dsts[p]) + off : nullptr;
    }
    a.carry = carry ? carry + off : nullptr;
    return a;
}

template <typename T, typename OUT, bool CARRY>
static hipError_t wsum_launch(int P, int ndst, void *const *dsts, const void *const *srcs,
                              const float *carry, size_t n, hipStream_t s)
{
    // the 16-bit pointers, and the float ones (loc_split's 4-byte stream)
    const void *half[2 * kMaxTeam], *wide[kMaxTeam + 1];
    int nh = 0, nw = 0;
    for (int p = 0; p < P; p++) half[nh++] = srcs[p];
    for (int q = 0; q < ndst; q++) {
        if (sizeof(OUT) == 2) half[nh++] = dsts[q];
        else wide[nw++] = dsts[q];
    }
    if (CARRY) wide[nw++] = carry;
    const rt::LocSplit sp = rt::loc_split(sizeof(T), n, half, nh, wide, nw);
    if (!sp.vec) {
        size_t blocks = (n + kTeamBlock - 1) / kTeamBlock;
        blocks = blocks > 8192 ? 8192 : blocks;
        hipLaunchKernelGGL((team_wsum_scalar_kernel<T, OUT, CARRY>), dim3((unsigned) blocks),
                           dim3(kTeamBlock), 0, s,
                           wsum_ptrs<T, OUT, kMaxTeam>(P, ndst, dsts, srcs, carry, 0), P, ndst, n);
        return hipGetLastError();
    }
    auto run = [&](auto pc) {
        constexpr int PP = decltype(pc)::value;
        // one tile of kWsumBlock groups per workgroup, in runs below the launch
        // limit: the first launch takes the edges, the others shifted pointers
        return for_each_tile_run(sp.ngroups, kWsumBlock, kWsumBlock, 1,
                                 [&](size_t t0, size_t nt, size_t ng) {
            const size_t off = t0 == 0 ? 0 : sp.head + t0 * kWsumBlock * rt::kWsumGroup;
            hipLaunchKernelGGL((team_wsum_vec_kernel<T, OUT, PP, CARRY>), dim3((unsigned) nt),
                               dim3(kWsumBlock), 0, s,
                               wsum_ptrs<T, OUT, PP>(PP, ndst, dsts, srcs, carry, off), ndst, ng,
                               t0 == 0 ? sp.head : (size_t) 0,
                               t0 == 0 ? sp.tail_start : (size_t) 0, t0 == 0 ? sp.nedge : 0);
            return hipGetLastError();
        });
    };
    if (P == 1) return run(std::integral_constant<int, 1>{});
    return dispatch_members(P, hipErrorInvalidValue, run);
}

template <typename T>
static hipError_t wsum_launch_type(bool wide_out, int P, int ndst, void *const *dsts,
                                   const void *const *srcs, const float *carry, size_t n,
                                   hipStream_t s)
{
    if (wide_out)
        return carry ? wsum_launch<T, float, true>(P, ndst, dsts, srcs, carry, n, s)
                     : wsum_launch<T, float, false>(P, ndst, dsts, srcs, carry, n, s);
    return carry ? wsum_launch<T, T, true>(P, ndst, dsts, srcs, carry, n, s)
                 : wsum_launch<T, T, false>(P, ndst, dsts, srcs, carry, n, s);
}

hipError_t launch_team_wsum(int type, int out_type, int P, int ndst, void *const *dsts,
                            const void *const *srcs, const float *carry, size_t n, hipStream_t s)
{
    if (!rt::wsum_pair(type, out_type) || !dsts || !srcs) return hipErrorInvalidValue;
    if (P < 1 || P > kMaxTeam || !(ndst == 1 || (ndst == P && P >= 2))) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const bool wide_out = out_type == T_FLOAT;
    if (type == T_HALF) return wsum_launch_type<half_t>(wide_out, P, ndst, dsts, srcs, carry, n, s);
    return wsum_launch_type<bf16_t>(wide_out, P, ndst, dsts, srcs, carry, n, s);
}

}  // namespace osgpu
