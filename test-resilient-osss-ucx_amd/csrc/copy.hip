// copy.hip -- the data-movement kernel of the broadcast / collect / fcollect /
// alltoall collectives (shmem_collect.cpp): up to kMaxCopySegs independent
// byte ranges (src -> dst), each source in local HBM or in a peer GPU's HBM
// mapped into this process, copied by ONE launch.
//
// The reference moves these bytes with shmemc_put / shmemc_get over UCX
// (src/shmemc/fcollect.c:32-38, src/shmemc/collect.c:52-64,
// src/shmemc/broadcast.c:39-41).  Here the owner of every target pulls all
// its pieces with 16-byte streaming loads: HBM-bound on one GPU, xGMI-bound
// across GPUs; 2 bytes of traffic (read + write) per byte copied.
//
// Layout of a launch: each segment gets ceil(body / (256 * U)) workgroups of
// 256 lanes, each lane U 16-byte vectors (all loads issued before the first
// store, non-temporal both ways -- the shape tools/tune_combine.hip found
// fastest for the combine).  The segments' tiles are dealt round-robin
// (workgroup b -> segment b % m, for as many rounds as the smallest segment
// has tiles; the rest of the larger segments follow, segment by segment):
// dispatch runs workgroups roughly in order, so with segments one after
// another the ~2 K workgroups resident at any moment would all stream ONE
// segment -- over xGMI one peer link at a time while the others idle.
// Round-robin keeps every segment (every peer's link) streaming at once.  Vectors are aligned on the DESTINATION; the
// source may sit at any 4-byte phase (gfx950 serves dword-aligned
// global_load_dwordx4), so a 32-bit collect whose block offsets are not
// 16-byte multiples stays on the vector path.  The first workgroup of a
// segment also copies the unaligned head (< 16 B) and tail (< 16 B) bytes.
// A segment whose source and destination differ in byte phase (impossible for
// 32/64-bit elements at natural alignment) takes the byte kernel.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "kernel_common.hpp"

namespace osgpu {
namespace {

typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // dword-aligned 16-B load

constexpr int kThreads = 256;
constexpr int kU = 4;  // 16-B vectors per lane
constexpr size_t kBlockBytes = (size_t) kThreads * kU * 16;

struct SegTable {
    const char *src[kMaxCopySegs];
    char *dst[kMaxCopySegs];
    size_t bytes[kMaxCopySegs];
    unsigned first_block[kMaxCopySegs + 1];  // of the blocked part (tiles past `rounds`)
    unsigned rounds;                          // round-robin rounds (vector kernel)
    int n;
};

__device__ __forceinline__ int find_seg(const SegTable &t, unsigned b)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxCopySegs; i++)
        if (i < t.n && b >= t.first_block[i]) k = i;
    return k;
}

__global__ __launch_bounds__(kThreads) void copy_vec_kernel(SegTable t)
{
    // round-robin part first: block b -> segment b % n, tile b / n; then
    // every segment's tiles from `rounds` on, segment after segment
    const unsigned inter = t.rounds * (unsigned) t.n;
    int k;
    unsigned lb;
    if (blockIdx.x < inter) {
        k = (int) (blockIdx.x % (unsigned) t.n);
        lb = blockIdx.x / (unsigned) t.n;
    } else {
        const unsigned b = blockIdx.x - inter;
        k = find_seg(t, b);
        lb = t.rounds + (b - t.first_block[k]);
    }
    const char *s = t.src[k];
    char *d = t.dst[k];
    const size_t bytes = t.bytes[k];
    size_t head = (size_t) ((0 - (uintptr_t) d) & 15);
    if (head > bytes) head = bytes;
    const size_t nvec = (bytes - head) / 16;
    const size_t tail0 = head + nvec * 16;
    if (lb == 0) {
        const unsigned x = threadIdx.x;
        if (x < head) d[x] = s[x];
        if (x < bytes - tail0) d[tail0 + x] = s[tail0 + x];
    }
    const u32x4_a4 *sv = reinterpret_cast<const u32x4_a4 *>(s + head);
    u32x4 *dv = reinterpret_cast<u32x4 *>(d + head);
    const size_t base = (size_t) lb * kThreads * kU + threadIdx.x;
    u32x4 v[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) {
        const size_t i = base + (size_t) u * kThreads;
        if (i < nvec) v[u] = __builtin_nontemporal_load(sv + i);
    }
#pragma unroll
    for (int u = 0; u < kU; u++) {
        const size_t i = base + (size_t) u * kThreads;
        if (i < nvec) __builtin_nontemporal_store(v[u], dv + i);
    }
}

__global__ __launch_bounds__(kThreads) void copy_byte_kernel(SegTable t)
{
    const int k = find_seg(t, blockIdx.x);
    const size_t per_block = (size_t) kThreads * 16;
    const size_t lo = (size_t) (blockIdx.x - t.first_block[k]) * per_block;
    for (size_t i = lo + threadIdx.x; i < t.bytes[k] && i < lo + per_block; i += kThreads)
        t.dst[k][i] = t.src[k][i];
}

// plain (cached) 8-byte loads, one word per lane: the preflight's owner-side
// read, which first leaves the lines in this GPU's L2 and later re-reads
// them after peers wrote them remotely (heap.cpp, remote-write leg)
__global__ __launch_bounds__(kThreads) void probe_load_kernel(const unsigned long long *src,
                                                              unsigned long long *dst,
                                                              unsigned words)
{
    if (threadIdx.x < words) dst[threadIdx.x] = src[threadIdx.x];
}

// One range across PCIe, device <-> pinned host memory mapped into the GPU
// (the STAGED path's legs, shmem_reduce.cpp run_staged).  A fixed grid of
// kHostGrid workgroups walks the range in tiles of kThreads * kU vectors,
// every lane's kU loads in flight before its stores.  Why a kernel and not
// the DMA engine: the engine's device-to-host rate follows the GPU's power
// state -- 28.4-29.5 GB/s for the first second of an idle box and again at
// random later, 56.6 once the state is up -- while this kernel's writes
// hold 53.9-54.0 GB/s in both states, and a DMA read beside it 41.8-42.0
// each way (tools/d2h_timeline.hip, profiles/r05_dma_state_timeline.jsonl).
// Vectors are aligned on the destination; block 0 copies the head and the
// tail bytes.
__global__ __launch_bounds__(kThreads) void host_copy_kernel(const char *__restrict__ s,
                                                             char *__restrict__ d, size_t bytes)
{
    size_t head = (size_t) ((0 - (uintptr_t) d) & 15);
    if (head > bytes) head = bytes;
    const size_t nvec = (bytes - head) / 16;
    const size_t tail0 = head + nvec * 16;
    if (blockIdx.x == 0) {
        const unsigned x = threadIdx.x;
        if (x < head) d[x] = s[x];
        if (x < bytes - tail0) d[tail0 + x] = s[tail0 + x];
    }
    const u32x4_a4 *sv = reinterpret_cast<const u32x4_a4 *>(s + head);
    u32x4 *dv = reinterpret_cast<u32x4 *>(d + head);
    const size_t stride = (size_t) gridDim.x * kThreads * kU;
    for (size_t base = (size_t) blockIdx.x * kThreads * kU + threadIdx.x; base < nvec;
         base += stride) {
        u32x4 v[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const size_t i = base + (size_t) u * kThreads;
            if (i < nvec) v[u] = __builtin_nontemporal_load(sv + i);
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const size_t i = base + (size_t) u * kThreads;
            if (i < nvec) dv[i] = v[u];
        }
    }
}

// ------------------------------------------------------------------ strided
// alltoalls' data movement: dst[k * dst_stride] = src[k * sst] over elements
// of 4 or 8 bytes, strides in elements (the reference issues one UCX get per
// element, src/putget.h:185-207).  Three forms, chosen per segment on the
// host, one launch per form; `unit` is what a lane moves per step:
//   gather   dst_stride == 1: unit = a 16-byte vector of the destination,
//            built from 4 (32-bit) or 2 (64-bit) strided element loads and
//            written by one 16-byte non-temporal store;
//   scatter  sst == 1: unit = a 16-byte vector of the source, one
//            non-temporal load, then 4 or 2 strided element stores;
//   both     unit = one element.
// Vectors are aligned on the contiguous side, whatever its dword phase; the
// first workgroup of a segment moves the elements before the first and after
// the last whole vector (vec_split).  Consecutive lanes take consecutive
// units, so one instruction of a wave touches the fewest lines of the strided
// side, and a lane issues all its U units' loads before its first store.
// Tiles of kThreads * U units are dealt round-robin over the segments like
// copy_vec_kernel's.  Every offset is size_t / ptrdiff_t: k * stride *
// elem_bytes passes 2^32 at small k.
enum { F_GATHER = 0, F_SCATTER = 1, F_BOTH = 2, F_NFORMS = 3 };

// Shipped shape per form (U units in flight per lane; NT = non-temporal
// accesses on the STRIDED side -- the contiguous side is always
// non-temporal, as in copy_vec_kernel).  Chosen by tools/strided_rate.py's
// in-process A/B over U in {2, 4, 8} x {plain, nt} (256 MiB useful per case,
// strides 2 / 3 / 17, both widths, 1 and 8 segments; geometric-mean us per
// launch over a form's cases, profiles/strided_rate.md):
//   gather   U2 278, U4 287, U8 295; nt 310-327 -- nt loads bypass L1, which
//            serves the 2-4 lanes sharing a line at 32 bits (+45 % at stride
//            2); at 64 bits nt is 3-7 % ahead, not enough to split the form;
//   scatter  U2 563, U4 569, U8 575; nt 1028-1069 -- nt element stores cost
//            1.6-3.5x at strides 2 and 3;
//   both     U2nt 633, U4nt 648, U8nt 661; plain 689-709.
// U moves a form by 3-6 %; the smallest measured is ahead in all three.
constexpr int kStridedU[F_NFORMS] = {2, 2, 2};
constexpr bool kStridedNT[F_NFORMS] = {false, false, true};

struct StridedTable {
    const char *src[kMaxCopySegs];
    char *dst[kMaxCopySegs];
    size_t n[kMaxCopySegs];      // elements
    size_t head[kMaxCopySegs];   // gather / scatter: elements before the first whole vector
    size_t units[kMaxCopySegs];  // whole vectors (gather / scatter) or elements (both)
    ptrdiff_t sst[kMaxCopySegs], dstr[kMaxCopySegs];  // in elements
    unsigned first_block[kMaxCopySegs + 1];  // of the blocked part (tiles past `rounds`)
    unsigned rounds;
    int nseg;
};

template <int ES> struct StridedElem;
template <> struct StridedElem<4> { using type = uint32_t; };
template <> struct StridedElem<8> { using type = unsigned long long; };

template <bool NT, typename T>
__device__ __forceinline__ T strided_ld(const T *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

template <bool NT, typename T>
__device__ __forceinline__ void strided_st(T v, T *p)
{
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int ES, int FORM, int U, bool NT>
__global__ __launch_bounds__(kThreads) void strided_kernel(StridedTable t)
{
    using T = typename StridedElem<ES>::type;
    constexpr size_t E = 16 / ES;
    const unsigned inter = t.rounds * (unsigned) t.nseg;
    int k = 0;
    unsigned lb;
    if (blockIdx.x < inter) {
        k = (int) (blockIdx.x % (unsigned) t.nseg);
        lb = blockIdx.x / (unsigned) t.nseg;
    } else {
        const unsigned b = blockIdx.x - inter;
#pragma unroll
        for (int i = 1; i < kMaxCopySegs; i++)
            if (i < t.nseg && b >= t.first_block[i]) k = i;
        lb = t.rounds + (b - t.first_block[k]);
    }
    const T *s = reinterpret_cast<const T *>(t.src[k]);
    T *d = reinterpret_cast<T *>(t.dst[k]);
    const size_t n = t.n[k], units = t.units[k];
    const ptrdiff_t ss = t.sst[k], ds = t.dstr[k];
    const size_t base = (size_t) lb * kThreads * U + threadIdx.x;
    if constexpr (FORM == F_BOTH) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t i = base + (size_t) u * kThreads;
            if (i < units) v[u] = strided_ld<NT>(s + (ptrdiff_t) i * ss);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t i = base + (size_t) u * kThreads;
            if (i < units) strided_st<NT>(v[u], d + (ptrdiff_t) i * ds);
        }
    } else {
        const size_t head = t.head[k], tail0 = head + units * E;
        if (lb == 0 && threadIdx.x < head + (n - tail0)) {
            const ptrdiff_t i = (ptrdiff_t) edge_index(head, tail0);
            d[i * ds] = s[i * ss];
        }
        Vec16<T> v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t i = base + (size_t) u * kThreads;
            if (i < units) {
                if constexpr (FORM == F_GATHER) {
                    const T *p = s + (ptrdiff_t) (head + i * E) * ss;
#pragma unroll
                    for (size_t e = 0; e < E; e++) v[u].e[e] = strided_ld<NT>(p + (ptrdiff_t) e * ss);
                } else {
                    v[u].v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s + head) + i);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t i = base + (size_t) u * kThreads;
            if (i < units) {
                if constexpr (FORM == F_GATHER) {
                    __builtin_nontemporal_store(v[u].v, reinterpret_cast<u32x4 *>(d + head) + i);
                } else {
                    T *p = d + (ptrdiff_t) (head + i * E) * ds;
#pragma unroll
                    for (size_t e = 0; e < E; e++) strided_st<NT>(v[u].e[e], p + (ptrdiff_t) e * ds);
                }
            }
        }
    }
}

std::atomic<int> g_strided_u[F_NFORMS] = {{kStridedU[0]}, {kStridedU[1]}, {kStridedU[2]}};
std::atomic<int> g_strided_nt[F_NFORMS] = {{kStridedNT[0]}, {kStridedNT[1]}, {kStridedNT[2]}};

template <int ES, int FORM, int U>
hipError_t launch_strided_shape(bool nt, const StridedTable &t, unsigned blocks, hipStream_t stream)
{
    if (nt)
        hipLaunchKernelGGL((strided_kernel<ES, FORM, U, true>), dim3(blocks), dim3(kThreads), 0,
                           stream, t);
    else
        hipLaunchKernelGGL((strided_kernel<ES, FORM, U, false>), dim3(blocks), dim3(kThreads), 0,
                           stream, t);
    return hipGetLastError();
}

template <int ES, int FORM>
hipError_t launch_strided_form(int U, bool nt, const StridedTable &t, unsigned blocks,
                               hipStream_t stream)
{
    switch (U) {
    case 2: return launch_strided_shape<ES, FORM, 2>(nt, t, blocks, stream);
    case 4: return launch_strided_shape<ES, FORM, 4>(nt, t, blocks, stream);
    case 8: return launch_strided_shape<ES, FORM, 8>(nt, t, blocks, stream);
    }
    return hipErrorInvalidValue;
}

template <int ES>
hipError_t launch_strided(const StridedSeg *segs, int nseg, hipStream_t stream)
{
    StridedTable tab[F_NFORMS] = {};
    unsigned blocks[F_NFORMS] = {0, 0, 0};
    int U[F_NFORMS];
    for (int f = 0; f < F_NFORMS; f++) U[f] = g_strided_u[f].load(std::memory_order_relaxed);
    for (int i = 0; i < nseg; i++) {
        const StridedSeg &g = segs[i];
        if (g.nelems == 0) continue;
        if (g.sst < 1 || g.dst_stride < 1 || ((uintptr_t) g.src | (uintptr_t) g.dst) % ES)
            return hipErrorInvalidValue;
        const int f = g.dst_stride == 1 ? F_GATHER : g.sst == 1 ? F_SCATTER : F_BOTH;
        StridedTable &t = tab[f];
        if (t.nseg == kMaxCopySegs) return hipErrorInvalidValue;  // callers batch
        size_t head = 0, units = g.nelems;
        if (f != F_BOTH) {  // vectors on the contiguous side
            const void *c = f == F_GATHER ? g.dst : g.src;
            const VecSplit sp = vec_split((size_t) ES, g.nelems, &c, 1, &c, 0);
            head = sp.head;
            units = sp.nvec;
        }
        const size_t per = (size_t) kThreads * U[f];
        size_t tiles = (units + per - 1) / per;
        if (tiles == 0) tiles = 1;  // edges only
        if (tiles > 0x7fffffffu - blocks[f]) return hipErrorInvalidValue;
        t.src[t.nseg] = (const char *) g.src;
        t.dst[t.nseg] = (char *) g.dst;
        t.n[t.nseg] = g.nelems;
        t.head[t.nseg] = head;
        t.units[t.nseg] = units;
        t.sst[t.nseg] = g.sst;
        t.dstr[t.nseg] = g.dst_stride;
        t.first_block[t.nseg] = blocks[f];
        t.nseg++;
        blocks[f] += (unsigned) tiles;
    }
    for (int f = 0; f < F_NFORMS; f++) {
        StridedTable &t = tab[f];
        if (!t.nseg) continue;
        // round-robin rounds = the smallest segment's tile count; the blocked
        // table then holds only each segment's tiles beyond them (launch_copy)
        unsigned rounds = ~0u;
        for (int i = 0; i < t.nseg; i++) {
            const unsigned next = i + 1 < t.nseg ? t.first_block[i + 1] : blocks[f];
            rounds = next - t.first_block[i] < rounds ? next - t.first_block[i] : rounds;
        }
        unsigned nb = 0;
        for (int i = 0; i < t.nseg; i++) {
            const unsigned next = i + 1 < t.nseg ? t.first_block[i + 1] : blocks[f];
            const unsigned tiles = next - t.first_block[i];
            t.first_block[i] = nb;
            nb += tiles - rounds;
        }
        t.first_block[t.nseg] = nb;
        t.rounds = rounds;
        const bool nt = g_strided_nt[f].load(std::memory_order_relaxed) != 0;
        hipError_t e = hipErrorInvalidValue;
        switch (f) {
        case F_GATHER: e = launch_strided_form<ES, F_GATHER>(U[f], nt, t, blocks[f], stream); break;
        case F_SCATTER: e = launch_strided_form<ES, F_SCATTER>(U[f], nt, t, blocks[f], stream); break;
        case F_BOTH: e = launch_strided_form<ES, F_BOTH>(U[f], nt, t, blocks[f], stream); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

bool set_strided_shape(int form, int u, int nt)
{
    if (form < -1 || form >= F_NFORMS || (u > 0 && u != 2 && u != 4 && u != 8)) return false;
    for (int f = 0; f < F_NFORMS; f++) {
        if (form != -1 && form != f) continue;
        g_strided_u[f].store(u > 0 ? u : kStridedU[f], std::memory_order_relaxed);
        g_strided_nt[f].store(u > 0 ? nt != 0 : (int) kStridedNT[f], std::memory_order_relaxed);
    }
    return true;
}

hipError_t launch_strided_copy(int elem_bytes, const StridedSeg *segs, int nseg, hipStream_t stream)
{
    if (nseg < 0 || (nseg > 0 && !segs)) return hipErrorInvalidValue;
    if (elem_bytes == 4) return launch_strided<4>(segs, nseg, stream);
    if (elem_bytes == 8) return launch_strided<8>(segs, nseg, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_host_copy(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    static const unsigned grid = [] {
        const char *e = getenv("OSGPU_HOST_COPY_GRID");
        const long v = e ? atol(e) : 256;
        return (unsigned) (v < 1 ? 1 : (v > 4096 ? 4096 : v));
    }();
    if (bytes == 0) return hipSuccess;
    if (((uintptr_t) src ^ (uintptr_t) dst) & 3) {  // byte phases differ: the byte kernel
        CopySeg g = {src, dst, bytes};
        return launch_copy(&g, 1, stream);
    }
    const size_t tiles = (bytes + kBlockBytes - 1) / kBlockBytes;
    hipLaunchKernelGGL(host_copy_kernel, dim3((unsigned) (tiles < grid ? tiles : grid)),
                       dim3(kThreads), 0, stream, static_cast<const char *>(src),
                       static_cast<char *>(dst), bytes);
    return hipGetLastError();
}

hipError_t launch_probe_load(const void *src, void *dst, size_t bytes, hipStream_t stream)
{
    static_assert(kProbeLoadBytes == (size_t) kThreads * 8, "one word per lane");
    if (bytes % 8 || bytes > kProbeLoadBytes || ((uintptr_t) src | (uintptr_t) dst) & 7)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_load_kernel, dim3(1), dim3(kThreads), 0, stream,
                       static_cast<const unsigned long long *>(src),
                       static_cast<unsigned long long *>(dst), (unsigned) (bytes / 8));
    return hipGetLastError();
}

hipError_t launch_copy(const CopySeg *segs, int nseg, hipStream_t stream)
{
    SegTable vt{}, bt{};
    unsigned vblocks = 0, bblocks = 0;
    for (int i = 0; i < nseg; i++) {
        const CopySeg &g = segs[i];
        if (g.bytes == 0) continue;
        const uintptr_t phase = (uintptr_t) g.src ^ (uintptr_t) g.dst;
        SegTable &t = (phase & 3) ? bt : vt;
        unsigned &nb = (phase & 3) ? bblocks : vblocks;
        const size_t per = (phase & 3) ? (size_t) kThreads * 16 : kBlockBytes;
        const size_t blocks = (g.bytes + per - 1) / per;
        if (blocks > 0x7fffffffu - nb) return hipErrorInvalidValue;
        if (t.n == kMaxCopySegs) return hipErrorInvalidValue;  // callers batch
        t.src[t.n] = (const char *) g.src;
        t.dst[t.n] = (char *) g.dst;
        t.bytes[t.n] = g.bytes;
        t.first_block[t.n] = nb;
        t.n++;
        nb += (unsigned) blocks;
    }
    if (vt.n) {
        // round-robin rounds = the smallest segment's tile count; the
        // blocked table then holds only each segment's tiles beyond them
        unsigned rounds = ~0u;
        for (int i = 0; i < vt.n; i++) {
            const unsigned next = i + 1 < vt.n ? vt.first_block[i + 1] : vblocks;
            rounds = next - vt.first_block[i] < rounds ? next - vt.first_block[i] : rounds;
        }
        unsigned nb = 0;
        for (int i = 0; i < vt.n; i++) {
            const unsigned next = i + 1 < vt.n ? vt.first_block[i + 1] : vblocks;
            const unsigned tiles = next - vt.first_block[i];
            vt.first_block[i] = nb;
            nb += tiles - rounds;
        }
        vt.first_block[vt.n] = nb;
        vt.rounds = rounds;
        hipLaunchKernelGGL(copy_vec_kernel, dim3(vblocks), dim3(kThreads), 0, stream, vt);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (bt.n) {
        bt.first_block[bt.n] = bblocks;
        hipLaunchKernelGGL(copy_byte_kernel, dim3(bblocks), dim3(kThreads), 0, stream, bt);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace osgpu
