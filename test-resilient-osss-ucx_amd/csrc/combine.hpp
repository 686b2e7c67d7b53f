// combine.hpp -- internal interface between the C-ABI layer and the kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace osgpu {

// 16-byte vectors in flight per lane per input of the register-form combine
// for <= 2, <= 4 and <= 8 inputs (register budget vs bytes in flight;
// tools/tune_combine.hip)
constexpr int kUK2 = 4, kUK4 = 4, kUK8 = 4;

// type codes (same numbering as include/osgpu_reduce.h OSGPU_T_*); T_HALF
// and T_BFLOAT16 are the extension types (16-bit patterns, elem_ops.hpp)
enum TypeCode {
    T_SHORT = 0, T_INT, T_LONG, T_LONGLONG, T_FLOAT, T_DOUBLE, T_LONGDOUBLE,
    T_COMPLEXF, T_COMPLEXD, T_HALF, T_BFLOAT16, T_NTYPES
};

// out[i] = fold(op, srcs[0][i], srcs[1][i], ..., srcs[k-1][i]) for i < n,
// enqueued on stream s.  All pointers are device-accessible (local HBM or a
// peer GPU's HBM mapped into this process).  `out` may alias srcs[0].
hipError_t launch_combine(int type, int op, void *out, const void *const *srcs, int k,
                          size_t n, hipStream_t s);
// The same where the pointers' 16-byte phases may differ (the reduce-scatter:
// block m of every source into a target at its own address): while every
// pointer is aligned to its element, 2..8 inputs per chunk stream as aligned
// 16-byte vectors through combine_shift_kernel (combine.hip); equal phases
// take launch_combine's kernels, pointers off their element alignment the
// element-granular one.
hipError_t launch_combine_shifted(int type, int op, void *out, const void *const *srcs, int k,
                                  size_t n, hipStream_t s);
// Its choices so far in this process (osgpu_test_shift_routes): out[0] chunks
// handed to launch_combine's kernels (equal phases, one input, 16-byte
// elements), out[1] chunks on combine_shift_kernel, out[2] chunks with a
// pointer off its element alignment (the element-granular kernel), out[3]
// launches of combine_shift_kernel; *u: the build's OSGPU_SHIFT_U.
void shift_route_counts(unsigned long long out[4], int *u);
// launch_combine over a table of `count` independent arrays (the batched
// reduce-to-all): targets[i] = fold of srcs[i][0 .. nsrc) over nelems[i]
// elements, empty entries skipped.  An entry of 2..8 inputs whose pointers
// share one 16-byte phase (entries may differ from each other) becomes a
// segment of combine_many_kernel (combine.hip), up to kManySegs
// (many_host.hpp) segments and max_launch_threads() threads a launch, an
// entry that does not fit split at a tile boundary; any other entry is
// launched on its own on the same stream -- launch_combine_shifted for a
// phase mismatch or a pointer off its element, launch_longdouble, and
// launch_combine for more than 8 inputs or one.  The host tables are read
// before the call returns.
hipError_t launch_combine_many(int type, int op, int count, void *const *targets,
                               const void *const *const *srcs, int nsrc, const size_t *nelems,
                               hipStream_t s);
// Its choices so far in this process (osgpu_test_many_routes): out[0]
// segments on combine_many_kernel (continuations included), entries sent to
// out[1] launch_combine_shifted, out[2] launch_longdouble, out[3]
// launch_combine's chunks of 8, out[4] the one-input copy, out[5] launches of
// combine_many_kernel, out[6] continuations of entries split between launches.
void many_route_counts(unsigned long long out[7]);

// Owner-computes team combine over an active set of P PEs (2 <= P <= 8):
// for i < n, dsts[q][i] = fold of srcs[*][i] in PE q's order (q first, then
// ascending, skipping q).  srcs/dsts indexed by position in the active set
// and already offset to this PE's shard.
// remote: some member's arrays live in another GPU's HBM (xGMI) -- the team
// kernel then takes the shapes last measured across GPUs (team.hip TeamShape)
constexpr int kMaxTeam = 8;

// Threads per launch of the one-tile-per-workgroup kernels (combine_lds,
// combine_vec, team_lds, team_vec): a grid's thread count must stay below
// 2^32 (HIP refuses larger grids: an 8-member team call of 1 Gi doubles,
// config 4's shape, needs 2^32 threads in the LDS form), so a larger call
// runs as several launches over consecutive runs of tiles.
constexpr size_t kMaxLaunchThreads = (size_t) 1 << 31;
// the limit in force: kMaxLaunchThreads, or a smaller one a test set
// (osgpu_test_max_launch_threads) to run the multi-launch path at small sizes
size_t max_launch_threads();
void set_max_launch_threads(size_t n);
hipError_t launch_team(int type, int op, int P, void *const *dsts, const void *const *srcs,
                       size_t n, hipStream_t s, bool remote = false);
hipError_t launch_team_longdouble(int op, int P, void *const *dsts, const void *const *srcs,
                                  size_t n, hipStream_t s);
// The same over [0, n) split by tiles instead of contiguous shards: of m
// members sharing one GPU, member k folds the tiles k, k + m, k + 2m, ...
// (a tile = one workgroup's vectors), so their concurrent grids stream the
// same address range together (run_team).  m = 1, k = 0: launch_team.
// hipErrorNotSupported for long double (contiguous shards only).
hipError_t launch_team_tiles(int type, int op, int P, void *const *dsts, const void *const *srcs,
                             size_t n, int m, int k, hipStream_t s, bool remote = false);
// Owner-computes prefix scan over an active set of P PEs (2 <= P <= 8,
// team.hip): for i < n, dsts[q][i] = srcs[0][i] op ... op srcs[q][i]
// (exclusive = 0) or ... op srcs[q-1][i] (exclusive = 1; dsts[0][i] = the
// op's identity), ascending for every q, one running fold per element.
// srcs/dsts as launch_team's; they must not overlap.  Multi-launch above
// max_launch_threads().  hipErrorNotSupported for long double.
hipError_t launch_team_scan(int type, int op, int exclusive, int P, void *const *dsts,
                            const void *const *srcs, size_t n, hipStream_t s);
// Owner-computes uniform reduce-to-all over an active set of P PEs
// (2 <= P <= 8, team.hip): for i < n and every q < P,
// dsts[q][i] = srcs[0][i] op ... op srcs[P-1][i], ONE ascending fold per
// element stored to all P targets.  srcs/dsts as launch_team's; they must not
// overlap.  Multi-launch above max_launch_threads().  Long double:
// launch_uniform_longdouble (longdouble.hip; pointers 8-byte aligned).
hipError_t launch_team_uniform(int type, int op, int P, void *const *dsts,
                               const void *const *srcs, size_t n, hipStream_t s);
hipError_t launch_uniform_longdouble(int op, int P, void *const *dsts, const void *const *srcs,
                                     size_t n, hipStream_t s);
// Max / min with location (team.hip): for i < n and every q < ndst,
// (val_dsts[q][i], loc_dsts[q][i]) = the ascending fold of the P pairs
// (val_srcs[p][i], loc_srcs[p][i]) by elem_ops.hpp LocStep; op OP_MAX or
// OP_MIN, the ordered types but long double.  1 <= P <= 8; ndst is 1 or P.
// loc_srcs null: member p's elements all carry member_locs[p] (a host array,
// passed to the kernel by value).  loc_srcs[0] set and loc_srcs[1] null
// (P > 1): input 0 alone has an index stream, the others member_locs[p] --
// a later chunk of a fold over more than 8 inputs, whose input 0 is the pair
// folded so far; a destination may then be input 0 itself (every element is
// read and written by one lane).  Otherwise targets must not overlap sources.
// Multi-launch above max_launch_threads().
hipError_t launch_team_loc(int type, int op, int P, int ndst, void *const *val_dsts,
                           int *const *loc_dsts, const void *const *val_srcs,
                           const int *const *loc_srcs, const int *member_locs, size_t n,
                           hipStream_t s);
// Float-accumulated sum of half / bfloat16 sources (team.hip): for i < n and
// every q < ndst, dsts[q][i] = out(widen(srcs[0][i]) + ... + widen(srcs[P-1][i])),
// ONE float add per source, ascending, by elem_ops.hpp WsumStep; out narrows
// once to `type` (out_type == type) or keeps the float (out_type == T_FLOAT).
// 1 <= P <= 8; ndst is 1, or P with P >= 2.  carry (device floats, or null):
// its element starts the accumulator and srcs[0] takes an add like the rest
// -- a later chunk of a fold over more than 8 members; with a float target
// and ndst = 1, dsts[0] may be the carry itself (every element is read and
// written by one lane).  Otherwise targets must not overlap sources.
// Multi-launch above max_launch_threads().
hipError_t launch_team_wsum(int type, int out_type, int P, int ndst, void *const *dsts,
                            const void *const *srcs, const float *carry, size_t n, hipStream_t s);
// n elements of the identity of (type, op) (scan_host.hpp scan_identity) at
// dst, any alignment; long double's padding bytes zero (team.hip)
hipError_t launch_scan_fill(int type, int op, void *dst, size_t n, hipStream_t s);

// Byte copy of up to kMaxCopySegs independent ranges in one launch (copy.hip):
// the data movement of broadcast / collect / fcollect / alltoall.  Sources may
// be peer HBM.  Zero-length segments are skipped; more than kMaxCopySegs
// non-empty segments is an error (callers batch).
constexpr int kMaxCopySegs = 8;
struct CopySeg {
    const void *src;
    void *dst;
    size_t bytes;
};
hipError_t launch_copy(const CopySeg *segs, int nseg, hipStream_t s);
// Strided element copy of up to kMaxCopySegs independent segments in one
// launch per form (copy.hip): the data movement of alltoalls.  For k < nelems,
//   dst[k * dst_stride] = src[k * sst]     (elements of elem_bytes = 4 or 8;
// strides in elements, >= 1; pointers aligned to elem_bytes; sources may be
// peer HBM).  Nothing between the strided elements is written.  Empty
// segments are skipped; more than kMaxCopySegs is an error (callers batch).
struct StridedSeg {
    const void *src;
    void *dst;
    size_t nelems;
    ptrdiff_t sst, dst_stride;
};
hipError_t launch_strided_copy(int elem_bytes, const StridedSeg *segs, int nseg, hipStream_t s);
// Launch shape of one form of the strided kernel (0 gather, 1 scatter, 2
// both strided; -1 all): u elements / vectors in flight per lane (2, 4 or
// 8), nt = 1 non-temporal accesses on the strided side.  u <= 0 restores
// the shipped shape.  For tools/strided_rate.py's in-process A/B only
// (osgpu_test_strided_shape); false for a shape that is not compiled.
bool set_strided_shape(int form, int u, int nt);
// Host fold of small host-heap calls (host_fold.hip): acc[i] = op(acc[i],
// in[i]) for i < n with the kernels' element ops compiled for the host
bool host_fold_supported(int type, int op);
bool host_fold(int type, int op, void *acc, const void *in, size_t n);
// The same for osgpu_reduce_loc: (val[k], loc[k]) takes (in_val[k], in_loc ?
// in_loc[k] : in_const) by elem_ops.hpp LocStep; max / min of the ordered
// types but long double
bool host_fold_loc_supported(int type, int op);
bool host_fold_loc(int type, int op, void *val, int *loc, const void *in_val, const int *in_loc,
                   int in_const, size_t n);
// The same for osgpu_reduce_wsum (elem_ops.hpp WsumStep over wsum_host.hpp's
// loops; type half or bfloat16): acc[k] = widen(src[k]); acc[k] += widen(in[k])
// by one float add; out[k] = narrow(acc[k])
bool host_wsum_widen(int type, float *acc, const void *src, size_t n);
bool host_wsum_add(int type, float *acc, const void *in, size_t n);
bool host_wsum_narrow(int type, void *out, const float *acc, size_t n);
// One range between HBM and pinned host memory mapped into the GPU (either
// side may be the host's device view): a fixed grid (OSGPU_HOST_COPY_GRID,
// default 256 workgroups) sized for one PCIe link, not for HBM (copy.hip)
hipError_t launch_host_copy(void *dst, const void *src, size_t bytes, hipStream_t s);
// <= kProbeLoadBytes of 8-byte words read with plain (L2-cached) loads into dst
constexpr size_t kProbeLoadBytes = 2048;
hipError_t launch_probe_load(const void *src, void *dst, size_t bytes, hipStream_t s);

// One-launch reduce-to-all for small calls (fused.hip): the call's two
// barriers run inside the kernel as epoch flags in every member's flag area
// (uncached device memory, mapped into every member).  Word layout of a
// flag area (unsigned long long):
constexpr int kFlagArrive = 0;    // [0, 8): arrive[member]
constexpr int kFlagDone = 8;      // [8, 16): done[member]
constexpr int kFlagTicket = 16;   // last-workgroup tickets (u32): completion,
constexpr int kFlagTicketIn = 17;  //   staged copy-in,
constexpr int kFlagTicketOut = 18; //   staged copy-out
constexpr int kFlagCount = 20;    // [20, 28): count[member] (collect: tag << 40 | source bytes)
constexpr int kFlagGateIn = 28;   // entry gate: (epoch << 20 | attempt << 1 | go), my grid's
constexpr int kFlagGateOut = 29;  //   verdict on the entry / exit wait (one decider per grid)
constexpr int kCountBits = 40;
constexpr int kFlagWords = 32;
// fused grids: at most one workgroup of 256 lanes per CU of the GPU (256 on
// MI355X), split between the members sharing it (one member per GPU: all)
constexpr int kFusedBlocksPerGpu = 256;
struct FusedArgs {
    const void *src[kMaxTeam];            // every member's source, active-set order
    void *dst[kMaxTeam];                  // outputs: team form every member's target, pull form mine
    int q[kMaxTeam];                      // active-set index whose fold order dst[d] uses
    unsigned long long *flags[kMaxTeam];  // every member's flag area
    unsigned long long *mine;             // my flag area
    int *err;                             // host-mapped: 1 arrive / 2 done not passed in time
    unsigned long long *done_host;        // host-mapped: epoch, written once the call is complete
    unsigned long long epoch, timeout;    // timeout: one wait slice, in wall-clock ticks
    int resume;                           // 0 first launch, 1 continue at the entry barrier,
                                          //   2 continue at the exit barrier
    unsigned attempt;                     // launches of this call so far (gate keys)
    size_t n;                             // elements from src[p] / dst[d]
    size_t nvec, head, tail_start;        // filled by launch_fused
    int nedge, P, D, me;                  // me: my active-set index
    int max_blocks;                       // grid cap (co-residency on a shared GPU)
    unsigned long long *trace;            // optional host-mapped phase clock (8 words)
    // staged form (host memory): null host_in = device form
    const void *host_in;                  // my host source (device-accessible)
    void *host_out;                       // my host target (device-accessible)
    void *stage_mine;                     // my input staging slot (= src[me])
    const void *stage_result;             // my result staging slot (= one of dst[])
    size_t host_bytes;
    // copy form (launch_fused_copy): nseg segments src[d] -> dst[d]
    size_t seg_bytes[kMaxTeam];
    int nseg;
    // collect form (launch_fused_collect): src[i] every member's source,
    // dst[0] my output; contributions differ per member and are exchanged
    // in the flag areas at arrival
    size_t my_count;                      // bytes of my source (< 2^kCountBits)
    unsigned long long count_tag;         // the set's collect sequence number
    size_t src_avail[kMaxTeam];           // bytes mapped from src[i] (bounds)
    size_t copy_limit;                    // copy in the launch iff the total fits
    unsigned long long *counts_host;      // host-mapped: every member's count, then
                                          //   counts_host[kMaxTeam] = 1 if copied
};
bool fused_supported(int type);
hipError_t launch_fused_copy(const FusedArgs &a, hipStream_t s);
hipError_t launch_fused_collect(const FusedArgs &a, hipStream_t s);
hipError_t launch_fused(int type, int op, const FusedArgs &a, hipStream_t s);

// Full-size parity checks on the GPU (verify.hip).  Checksum of n elements
// of elem_bytes (2, 4, 8, 16) into *out (device memory, zeroed by the
// caller): CK_SUM adds the zero-extended elements mod 2^64, CK_XOR xors
// them, CK_HASH adds a position-weighted mix of each element's bits.
// Compare: out[0] += differing 16-B vectors (bytes when unaligned), out[1]
// = min(out[1], byte offset of the first difference); out[1] preset to ~0.
enum { CK_SUM = 0, CK_XOR = 1, CK_HASH = 2 };
hipError_t launch_checksum(int elem_bytes, int mode, const void *p, size_t n,
                           unsigned long long *out, hipStream_t s);
hipError_t launch_compare(const void *a, const void *b, size_t nbytes, unsigned long long *out,
                          hipStream_t s);

// x87 80-bit extended combine (soft-float on the GPU), longdouble.hip
hipError_t launch_longdouble(int op, void *out, const void *const *srcs, int k, size_t n,
                             hipStream_t s);

}  // namespace osgpu
