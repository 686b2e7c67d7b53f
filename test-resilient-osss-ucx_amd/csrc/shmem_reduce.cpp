// shmem_reduce.cpp -- C-ABI layer of libosgpu_reduce.so.
//
// Replaces the reduce-to-all entry points of the reference
// (SHMEM_REDUCE_TYPE_OP, src/reductions.c:139-154, instantiated at :248-297)
// with the same 44 signatures.  Where the reference walks its peers with a
// blocking 64-element shmem_getmem per chunk and folds through a function
// pointer per element (udr_<T>_to_all, src/reductions.c:32-120), this layer
// picks one of these MI355X paths:
//
//   TEAM    device-resident, source and target symmetric in registered
//           heaps, 2..8 PEs: owner-computes kernel (team.hip) -- PE g folds
//           shard g of every PE's target, each in that PE's own fold order,
//           reading every source once over HBM/xGMI (bit-exact);
//   PULL    device-resident, source symmetric: the reference's pull
//           schedule as ONE combine kernel streaming all PE_size sources in
//           the PE's fold order (bit-exact);
//   RCCL    device-resident, one process per GPU with an RCCL communicator:
//           ncclAllReduce over xGMI (FP within tolerance);
//   STAGED  host symmetric-heap arguments: H2D own source -> TEAM over
//           IPC-mapped device staging -> D2H, pipelined (bit-exact);
//   GETMEM  host arguments when staging cannot be mapped by every PE: peers'
//           sources pulled with the runtime's shmem_getmem, H2D, combine, D2H.
//
// The two shmem_barrier calls of the reference (:82, :113) keep their roles
// (every source ready / every reader or writer done) on every non-RCCL path.
// The per-call scaffolding shared with shmem_collect.cpp is call_common.hpp.
//
// The other front doors (reduce-scatter, batched, scan, uniform, max/min with
// location, float-accumulated 16-bit sum) have no forms of their own above the kernels: they share the
// reduce-to-all's prologue (begin_call, arrays_kind), its host route
// (host_route_fold), its GETMEM chunk loop (getmem_chunks), its pull schedule
// (symmetric_ptrs, fold_sources, run_pull) and its caller-first host fold
// (host_fold_table), and pass what differs -- the members to read, a byte
// offset, the launcher, an overlap verdict -- as arguments.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/osgpu_reduce.h"
#include "call_common.hpp"
#include "combine.hpp"
#include "loc_host.hpp"
#include "many_host.hpp"
#include "rscatter_host.hpp"
#include "runtime.hpp"
#include "scan_host.hpp"
#include "wsum_host.hpp"

namespace {

using namespace osgpu::rt;

thread_local int t_last_path = OSGPU_RAN_NONE;

// ------------------------------------------------------------- the paths

// one reduce-to-all call: the active set (Coll) plus the arrays
struct Call : Coll {
    int type = 0, op = 0;
    void *target = nullptr, *source = nullptr;
    int nreduce = 0;
    size_t nbytes = 0;
};

// ----------------------------------------------------------- the prologue

// What every front door starts with: the active set (make_coll's checks) and
// the arrays.  `empty`: nothing to combine -- the collective still syncs, and
// the door returns.  false then.
bool begin_call(Call &c, const char *name, int type, int op, void *target, const void *source,
                int nreduce, int PE_start, int logPE_stride, int PE_size, long *pSync, bool empty)
{
    static_cast<Coll &>(c) = make_coll(name, PE_start, logPE_stride, PE_size, pSync);
    c.type = type;
    c.op = op;
    c.target = target;
    c.source = const_cast<void *>(source);
    c.nreduce = nreduce;
    if (!empty) return true;
    t_last_path = OSGPU_RAN_BARRIER_ONLY;
    sync_only(c);
    return false;
}

bool is_reduction(int type, int op) { return has_op(type, op) || has_ext_op(type, op); }

// `has`: the osgpu_has_* query that answers for the call
void require_reduction(const char *name, int type, int op, const char *has)
{
    if (!is_reduction(type, op))
        fatal(name, "type %d op %d is not a reduction of this library (%s)", type, op, has);
}

// The arrays of a call are all device or all host memory: the kind, and the
// first array's device.  heap_first (the batched call's long tables): an
// array after the first inside my registered device heap needs no pointer
// query.
struct Array {
    const void *p;
    size_t bytes;
};
MemKind arrays_kind(const Coll &c, const Array *arrays, size_t count, int *dev,
                    bool heap_first = false)
{
    const MemKind kind = mem_kind(arrays[0].p, dev);
    for (size_t i = 1; i < count; i++) {
        int seg = -1, d = -1;
        size_t off = 0;
        const bool in_heap =
            heap_first && heap_locate(c.me, arrays[i].p, arrays[i].bytes, &seg, &off);
        if ((in_heap ? MEM_DEVICE : mem_kind(arrays[i].p, &d)) != kind)
            fatal(c.name, "the arrays must all be device or all be host memory");
    }
    return kind;
}

// Host heaps: the host fold (true), or the forms that cross the GPU.  The
// fold serves small calls under OSGPU_HOST_AUTO (hp: host_path()):
// `pulled_bound` is a size every member shares, so all of them take the same
// path.  `no_staged`: what to call a collective without a STAGED form in the
// trace (null: it has one).
bool host_route_fold(const Call &c, int hp, size_t pulled_bound, bool fold_supported,
                     const char *no_staged)
{
    require_host_heaps(c);
    const size_t fold_lim = host_fold_max_bytes();  // 0: off
    if (hp == OSGPU_HOST_AUTO && fold_lim > 0 && pulled_bound <= fold_lim && fold_supported)
        return true;
    if (no_staged && hp == OSGPU_HOST_STAGED)
        DBG("%s PE %d: no STAGED form of %s, taking GETMEM", c.name, c.me, no_staged);
    return false;
}

// --------------------------------------------------- symmetric pointers

// [p, p + nbytes) in my registered heap: every member's copy of it, in
// active-set order.  *remote: one of them is another GPU's memory.
template <class Ptr>  // char *, void *, const void *: what the launcher at hand takes
bool symmetric_ptrs(const Coll &c, const void *p, size_t nbytes, std::vector<Ptr> &out,
                    bool *remote = nullptr)
{
    int seg = -1;
    size_t off = 0;
    if (!heap_locate(c.me, p, nbytes, &seg, &off)) return false;
    out.resize(c.PE_size);
    for (int i = 0; i < c.PE_size; i++) {
        char *q = nullptr;
        bool far = false;
        if (!heap_peer(c.pe_at(i), seg, off, nbytes, &q, &far)) return false;
        out[i] = q;
        if (remote && far) *remote = true;
    }
    return true;
}

// the one wording of the pull forms that have no other path
[[noreturn]] void no_device_heap(const Coll &c, const char *what, size_t nbytes)
{
    fatal(c.name, "device-resident arguments need every active PE's device heap registered "
                  "(osgpu_heap_create / osgpu_heap_register) and the whole %zu-byte %s inside it",
          nbytes, what);
}

// Owner-computes team path (team.hip): needs both source and target inside
// every active PE's registered heap at the same offsets (symmetric), no
// overlap between them, and 2 <= PE_size <= 8.  Fills srcs/dsts in active-set
// order and returns this PE's index, or -1.
int team_ptrs(const Call &c, std::vector<const void *> &srcs, std::vector<void *> &dsts,
              bool *remote = nullptr)
{
    if (c.PE_size < 2 || c.PE_size > osgpu::kMaxTeam) return -1;
    if (ranges_overlap(c.target, c.nbytes, c.source, c.nbytes)) return -1;
    bool far = false;
    if (!symmetric_ptrs(c, c.source, c.nbytes, srcs, &far) ||
        !symmetric_ptrs(c, c.target, c.nbytes, dsts, &far))
        return -1;
    if (remote) *remote = far;
    return c.index_of(c.me);
}

// Members of one active set that are threads of THIS process on the same
// GPU (threads-as-PEs; mixed topologies): each registers its call here
// before the entry barrier, so after it every local member is known, and a
// run of consecutive local members [first, last] folds the union of their
// shards split by TILES (launch_team_tiles: member k of m takes the tiles k,
// k + m, ...) instead of one contiguous shard each.  Their grids share the
// GPU; with contiguous shards the two concurrent half-grids of a 2-PE call
// streamed two distant ranges and ended ~16 us apart, the whole call taking
// ~6 % longer than one full grid (profiles/r04_call_overhead_1..4.jsonl).
// Calls on a set are matched by a sequence number kept per (set, device,
// PE) in this process -- not per OS thread, so a PE whose calls move
// between threads (a thread pool) keeps its count: OpenSHMEM members call
// a set's collectives in the same order.
// OSGPU_TEAM_LOCAL: merge (the default: the run's first member launches one
// grid over the whole run, the others only wait in the barriers) | shards
// (contiguous shards always) | tiles.  A 2-PE 64 Mi-double call: merged
// 379-384 us, 376.5-376.8 with OSGPU_SYNC=word, shards 377-391, tiles
// 401-409 (profiles/r04_call_overhead_6.jsonl); merged + word in the bench
// 0.726 of 8 TB/s (r04_bench_merge_word.log) against 0.68-0.71.
struct LocalCall {
    unsigned mask = 0;  // active-set indices of the local members
    int left = 0;       // registered members not yet done
};
std::mutex g_local_mu;
std::map<std::tuple<int, int, int, int, unsigned long long>, LocalCall> g_local;
std::map<std::tuple<int, int, int, int, int>, unsigned long long> g_local_seq;  // + PE

enum { LOCAL_SHARDS = 0, LOCAL_TILES, LOCAL_MERGE };
int local_mode()
{
    static const int m = [] {
        const char *e = getenv("OSGPU_TEAM_LOCAL");
        if (e && !strcmp(e, "tiles")) return (int) LOCAL_TILES;
        if (e && !strcmp(e, "shards")) return (int) LOCAL_SHARDS;
        return (int) LOCAL_MERGE;
    }();
    return m;
}

void run_team(const Call &c, const std::vector<const void *> &srcs,
              const std::vector<void *> &dsts, int idx, bool remote)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const size_t s = type_size(c.type);
    const int mode = local_mode();
    // (long double: contiguous shards or merged runs, no tiles)
    const bool tiles = mode == LOCAL_MERGE || (mode == LOCAL_TILES && c.type != osgpu::T_LONGDOUBLE);
    std::tuple<int, int, int, int, unsigned long long> key;
    if (tiles) {
        int dev = 0;
        HIPCHK(c.name, hipGetDevice(&dev));
        const auto set = std::make_tuple(c.PE_start, c.step, c.PE_size, dev);
        std::lock_guard<std::mutex> lk(g_local_mu);
        const unsigned long long seq = ++g_local_seq[std::tuple_cat(set, std::make_tuple(c.me))];
        key = std::tuple_cat(set, std::make_tuple(seq));
        LocalCall &L = g_local[key];
        L.mask |= 1u << idx;
        L.left++;
    }
    t_last_path = OSGPU_RAN_TEAM;
    call_trace(c.me, 0, "start");
    entry_sync(c.name, st);
    call_trace(c.me, 1, "entry_sync");
    barrier(c);  // src/reductions.c:82 -- sources ready, every target writable
    call_trace(c.me, 2, "barrier1");
    // the run of consecutive local members I belong to (just me without tiles)
    int first = idx, last = idx;
    if (tiles) {
        unsigned mask;
        {
            std::lock_guard<std::mutex> lk(g_local_mu);
            mask = g_local[key].mask;
        }
        while (first > 0 && (mask >> (first - 1) & 1u)) first--;
        while (last + 1 < c.PE_size && (mask >> (last + 1) & 1u)) last++;
    }
    long long lo = 0, hi = 0, t = 0;
    shard_of(c.nreduce, c.PE_size, first, s, &lo, &t);
    shard_of(c.nreduce, c.PE_size, last, s, &t, &hi);
    std::vector<const void *> sp(c.PE_size);
    std::vector<void *> dp(c.PE_size);
    for (int i = 0; i < c.PE_size; i++) {
        sp[i] = (const char *) srcs[i] + (size_t) lo * s;
        dp[i] = (char *) dsts[i] + (size_t) lo * s;
    }
    DBG("%s PE %d: team path, [%lld, %lld) of %d, tiles %d of %d, P=%d", c.name, c.me, lo, hi,
        c.nreduce, idx - first, last - first + 1, c.PE_size);
    int m = last - first + 1, k = idx - first;
    if (mode == LOCAL_MERGE) {
        if (k > 0) hi = lo;  // the run's first member launches for all of it
        m = 1;
        k = 0;
    }
    if (hi > lo)
        launched(c.name, "team combine launch",
                 osgpu::launch_team_tiles(c.type, c.op, c.PE_size, dp.data(), sp.data(),
                                          (size_t) (hi - lo), m, k, st, remote));
    call_trace(c.me, 3, "launch");
    DBG("%s PE %d: team kernel launched", c.name, c.me);
    stream_wait(c.name, st);
    call_trace(c.me, 4, "wait");
    DBG("%s PE %d: team kernel done", c.name, c.me);
    barrier(c);  // src/reductions.c:113 -- every shard of my target is written
    call_trace(c.me, 5, "barrier2");
    call_trace(c.me, 6, "end");
    if (tiles) {
        std::lock_guard<std::mutex> lk(g_local_mu);
        auto it = g_local.find(key);
        if (it != g_local.end() && --it->second.left == 0) g_local.erase(it);
    }
}

// Push form of the team exchange (osgpu_set_team_exchange(1)): every byte
// crosses the fabric as a remote WRITE.  Per chunk of every shard:
//   scatter  PE q copies its source's part of shard g into slot q of PE g's
//            inbox (the STAGED path's IPC-mapped staging, 4 x slot bytes per
//            PE: P slots of C elements), for every g -- one copy launch;
//   barrier  every inbox holds the chunk (every member has entered, so every
//            target is writable);
//   fold     PE g runs the team kernel over its inbox (local HBM reads) and
//            writes shard g of every member's target (remote writes);
//   barrier  every inbox slot is drained / every target shard written.
// Same fabric bytes as the pull form ((P-1)/P * N * s each way per PE),
// plus N * s of local inbox traffic; which form the links prefer is
// measured by bench.py's N > 1 xgmi_probe.
void run_team_push(const Call &c, const std::vector<const void *> &srcs,
                   const std::vector<void *> &dsts, int idx, StageSet &S)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const size_t s = type_size(c.type);
    const int P = c.PE_size;
    const long long g16 = s >= 16 ? 1 : (long long) (16 / s);
    std::vector<long long> lo(P), hi(P);
    long long most = 0;
    for (int g = 0; g < P; g++) {
        shard_of(c.nreduce, P, g, s, &lo[g], &hi[g]);
        most = std::max(most, hi[g] - lo[g]);
    }
    long long C = (long long) ((4 * S.slot) / (size_t) P / s) / g16 * g16;  // elements per slot
    if (C < 1) fatal(c.name, "staging too small for the push exchange of %d PEs", P);
    const long long nchunks = (most + C - 1) / C;
    t_last_path = OSGPU_RAN_TEAM_PUSH;
    DBG("%s PE %d: team push, %lld chunks of %lld", c.name, c.me, nchunks, C);
    entry_sync(c.name, st);
    // The inboxes are the staging areas of this active set, whose out slots
    // a member may still be draining into its host target after a STAGED or
    // fused-staged call it has not yet returned from: no member scatters
    // before every member has entered this call.
    barrier(c);
    std::vector<osgpu::CopySeg> segs;
    std::vector<const void *> sp(P);
    std::vector<void *> dp(P);
    for (long long k = 0; k < nchunks; k++) {
        segs.clear();
        for (int g = 0; g < P; g++) {
            const long long a = lo[g] + k * C, b = std::min(hi[g], a + C);
            if (b > a)
                segs.push_back({(const char *) srcs[idx] + (size_t) a * s,
                                S.region(g) + (size_t) idx * C * s, (size_t) (b - a) * s});
        }
        for_batches(segs, osgpu::kMaxCopySegs, [&](const osgpu::CopySeg *b, int m) {
            launched(c.name, "scatter launch", osgpu::launch_copy(b, m, st));
        });
        stream_wait(c.name, st);
        barrier(c);  // every inbox holds chunk k; every member has entered (:82)
        const long long a = lo[idx] + k * C, b = std::min(hi[idx], a + C);
        if (b > a) {
            for (int i = 0; i < P; i++) {
                sp[i] = S.region(idx) + (size_t) i * C * s;
                dp[i] = (char *) dsts[i] + (size_t) a * s;
            }
            launched(c.name, "team fold launch",
                     osgpu::launch_team(c.type, c.op, P, dp.data(), sp.data(), (size_t) (b - a),
                                        st, S.ndev > 1));
            stream_wait(c.name, st);
        }
        barrier(c);  // inboxes drained; after the last chunk every target is complete (:113)
    }
}

// The members this PE folds, caller first (osgpu_fold_order), as PE numbers
std::vector<int> caller_first(const Coll &c)
{
    std::vector<int> order(c.PE_size);
    fold_order(c.me, c.PE_start, c.step, c.PE_size, order.data());
    return order;
}

// the first K members of the set, ascending (the scan, the uniform reduce)
std::vector<int> ascending(const Coll &c, int K)
{
    std::vector<int> pes(K);
    for (int k = 0; k < K; k++) pes[k] = c.pe_at(k);
    return pes;
}

// `pes`' copies of the symmetric [p, p + nbytes), `off` bytes in, in the order
// of `pes`.  false: not inside every member's registered heap.
bool fold_sources(const Coll &c, const std::vector<int> &pes, const void *p, size_t nbytes,
                  size_t off, const void **srcs)
{
    std::vector<char *> all;
    if (!symmetric_ptrs(c, p, nbytes, all)) return false;
    for (size_t k = 0; k < pes.size(); k++) srcs[k] = all[c.index_of(pes[k])] + off;
    return true;
}

// PULL into my own target: the reference's schedule (src/reductions.c:82,
// :113) around ONE launch over the sources the caller put in fold order.
// `overlap`: peers read what the target overlaps, so the result goes to
// scratch until they are done.  launch(out, stream) reports its own failure.
template <class Launch>
void run_pull(const Call &c, size_t out_bytes, bool overlap, Launch launch)
{
    hipStream_t st = pe_stream(c.name, c.me);
    t_last_path = OSGPU_RAN_PULL;
    // prior device work of this process that produced `source` must be done
    entry_sync(c.name, st);
    barrier(c);  // :82 -- every source is ready
    const DeviceOut out(c, c.target, overlap, out_bytes);
    launch(out.out, st);
    stream_wait(c.name, st);
    barrier(c);  // :113 -- peers are done reading my source
    out.finish(out_bytes, st);
}

// members: every member's source in active-set order (symmetric_ptrs)
void run_p2p(const Call &c, const std::vector<const void *> &members)
{
    const std::vector<int> order = caller_first(c);
    std::vector<const void *> srcs(c.PE_size);  // in this PE's fold order
    for (int k = 0; k < c.PE_size; k++) srcs[k] = members[c.index_of(order[k])];
    const bool overlap = c.PE_size > 1 && ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    run_pull(c, c.nbytes, overlap, [&](void *out, hipStream_t st) {
        launched(c.name, "combine launch",
                 osgpu::launch_combine(c.type, c.op, out, srcs.data(), c.PE_size,
                                       (size_t) c.nreduce, st));
    });
}

// ---------------------------------------------------- fused small calls

// A device-resident call of at most fused_max_bytes() per PE runs as ONE
// launch with its barriers on the device (fused.hip); larger calls keep the
// host barriers around the full-chip streaming kernels.
// Only with entry ordering that does not wait for this PE's own stream:
// under hipDeviceSynchronize every call would first wait for the previous
// fused launch to retire (measured 26 us per 1 Ki-int call against 16 us on
// the host-barrier path; 12 us with `stream` ordering).
// The pull form reads P sources per PE (P times the team form's bytes) on
// its share of the CUs: its limit is a quarter of the team form's (measured
// with 4 processes on one GPU at 1 MiB per PE: fused pull 42 us against 29
// us with host barriers; fused team 23 us).
bool fused_eligible(const Call &c, bool team)
{
    const int em = entry_mode();
    const size_t lim = team ? fused_max_bytes() : fused_max_bytes() / 4;
    return (em == ENTRY_STREAM || em == ENTRY_NONE) && osgpu::fused_supported(c.type) &&
           c.PE_size >= 2 && c.PE_size <= osgpu::kMaxTeam && c.nbytes <= lim &&
           c.ops.getmem != nullptr;
}

// team = true: owner-computes over every member's target (srcs/dsts in
// active-set order); false: pull form, my own target from every source.
void run_fused(const Call &c, SyncSet &S, const std::vector<const void *> &srcs,
               const std::vector<void *> &dsts, bool team, const StageSet *G = nullptr,
               const void *host_in = nullptr, void *host_out = nullptr)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const size_t s = type_size(c.type);
    const int P = c.PE_size, idx = S.idx;
    osgpu::FusedArgs a = fused_args(c, S);
    long long lo = 0, hi = c.nreduce;
    if (team) shard_of(c.nreduce, P, idx, s, &lo, &hi);
    // (staged form: target and source may overlap -- the source is copied
    // into staging before any member writes, the target after all are done)
    const bool overlap = !G && !team && ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    const DeviceOut out(c, c.target, overlap, c.nbytes);
    for (int i = 0; i < P; i++) a.src[i] = (const char *) srcs[i] + (size_t) lo * s;
    if (team) {
        for (int d = 0; d < P; d++) {
            a.dst[d] = (char *) dsts[d] + (size_t) lo * s;
            a.q[d] = d;
        }
        a.D = P;
    } else {
        a.dst[0] = out.out;
        a.q[0] = idx;
        a.D = 1;
    }
    a.n = (size_t) (hi - lo);
    if (G) {
        a.host_in = host_in;
        a.host_out = host_out;
        a.stage_mine = G->in(idx, 0);
        a.stage_result = G->out(idx, 0);
        a.host_bytes = c.nbytes;
    }
    t_last_path = G ? OSGPU_RAN_FUSED_STAGED : team ? OSGPU_RAN_FUSED_TEAM : OSGPU_RAN_FUSED_PULL;
    DBG("%s PE %d: fused %s path, epoch %llu, [%lld, %lld)", c.name, c.me,
        G ? "staged" : team ? "team" : "pull", a.epoch, lo, hi);
    // OSGPU_FUSED_TRACE=1: phase clocks of workgroup 0 / the last workgroup
    static unsigned long long *trace = [] {
        unsigned long long *p = nullptr;
        if (getenv("OSGPU_FUSED_TRACE") &&
            hipHostMalloc((void **) &p, 64, hipHostMallocMapped | hipHostMallocCoherent) !=
                hipSuccess)
            p = nullptr;
        return p;
    }();
    a.trace = trace;
    if (trace) memset(trace, 0, 64);  // slots a continuation launch leaves unwritten stay 0
    if (!fused_run(c, S, st, a, [&](const osgpu::FusedArgs &x) {
            return osgpu::launch_fused(c.type, c.op, x, st);
        })) {
        t_last_path = OSGPU_RAN_FUSED_FAILED;
        return;
    }
    out.finish(c.nbytes, st);  // every reader of my source is done: the call passed its exit barrier
    if (trace && osgpu_last_continuations() > 0) {
        // the phase clocks are taken by the first launch only (fused.hip):
        // a call that needed continuations has no consistent breakdown
        fprintf(stderr, "[osgpu fused PE %d epoch %llu] %d continuation launch(es): no phase "
                        "breakdown\n", c.me, a.epoch, osgpu_last_continuations());
    } else if (trace) {
        const double tk = 1e3 / S.rate_khz;  // us per tick of the device wall clock
        fprintf(stderr, "[osgpu fused PE %d epoch %llu] arrive-wait %.2f body %.2f fence %.2f "
                        "ticket+fence %.2f done-wait %.2f us\n", c.me, a.epoch,
                (trace[1] - trace[0]) * tk, (trace[2] - trace[1]) * tk,
                (trace[3] - trace[2]) * tk, (trace[4] - trace[3]) * tk,
                (trace[6] - trace[5]) * tk);
    }
}

// RCCL's arithmetic for a (type, op), or false.
//  * integer sum/prod/min/max: order-independent (wrapping ring, lattice),
//    so ncclAllReduce is bit-exact -- allowed on the automatic path;
//  * FP / complex sum and prod: RCCL folds in its own order, identical on
//    every PE, where the reference folds in a per-PE order
//    (src/reductions.c:79-111): within tolerance only, so only when the
//    caller forces OSGPU_PATH_RCCL (`fp_ok`);
//  * half / bfloat16 (the extension types): never, for any op -- one
//    rounding per step in the per-PE order is their definition;
//  * FP min/max: never.  The reference's `a<b?a:b` / `a>b?a:b`
//    (src/shmemu/miscops.c:80-90) resolves NaN and signed-zero ties by fold
//    position; RCCL's min/max do not follow it.
bool rccl_types(int type, int op, bool fp_ok, ncclDataType_t *dt, ncclRedOp_t *rop,
                size_t *mult)
{
    *mult = 1;
    switch (op) {
    case OSGPU_OP_SUM: *rop = ncclSum; break;
    case OSGPU_OP_PROD: *rop = ncclProd; break;
    case OSGPU_OP_MAX: *rop = ncclMax; break;
    case OSGPU_OP_MIN: *rop = ncclMin; break;
    default: return false;
    }
    const bool arith = op == OSGPU_OP_SUM || op == OSGPU_OP_PROD;
    switch (type) {
    case OSGPU_T_INT: *dt = ncclInt32; return true;
    case OSGPU_T_LONG: case OSGPU_T_LONGLONG: *dt = ncclInt64; return true;
    case OSGPU_T_FLOAT: *dt = ncclFloat32; return fp_ok && arith;
    case OSGPU_T_DOUBLE: *dt = ncclFloat64; return fp_ok && arith;
    case OSGPU_T_COMPLEXF: *dt = ncclFloat32; *mult = 2; return fp_ok && op == OSGPU_OP_SUM;
    case OSGPU_T_COMPLEXD: *dt = ncclFloat64; *mult = 2; return fp_ok && op == OSGPU_OP_SUM;
    }
    return false;
}

bool rccl_usable(const Call &c, bool forced)
{
    ncclDataType_t dt;
    ncclRedOp_t rop;
    size_t mult;
    return rccl_whole_job(c) && rccl_types(c.type, c.op, forced, &dt, &rop, &mult);
}

void run_rccl(const Call &c)
{
    ncclDataType_t dt;
    ncclRedOp_t rop;
    size_t mult;
    rccl_types(c.type, c.op, true, &dt, &rop, &mult);
    t_last_path = OSGPU_RAN_RCCL;
    hipStream_t st = pe_stream(c.name, c.me);
    entry_sync(c.name);
    const bool overlap = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes) &&
                         c.target != c.source;
    const DeviceOut out(c, c.target, overlap, c.nbytes);
    ncclResult_t r = ncclAllReduce(c.source, out.out, (size_t) c.nreduce * mult, dt, rop,
                                   g_rccl.world, st);
    if (r != ncclSuccess) fatal(c.name, "ncclAllReduce: %s", ncclGetErrorString(r));
    stream_wait(c.name, st);
    out.finish(c.nbytes, st);
}

// How the STAGED path moves its chunks across PCIe (OSGPU_STAGE_COPY):
//   dma (default)   both legs by the DMA engines (hipMemcpyAsync on the two
//                   copy streams, runtime.cpp device_copy_streams): 44.5 GB/s
//                   each way pinned, 38-41 pageable, 2 PEs at 64 Mi doubles;
//   kout            H2D by DMA, D2H by launch_host_copy (a kernel writing
//                   the host's device view); 34.7 pinned;
//   kernel          both legs by kernel; 30.6-31.0 pinned
//   (profiles/r05_staged_copy_modes.jsonl).  The kernel legs exist for the
//   GPU's low power state, in which the DMA engine's D2H rate falls to
//   28-30 GB/s (the first second of an idle box) while a kernel's writes
//   hold 54 (tools/d2h_timeline.hip, profiles/r05_dma_state_timeline.jsonl);
//   the bench reports that state beside the rates (dma_state).
// A leg whose host memory has no device view takes the DMA engine.
// (runtime.cpp stage_copy_mode: osgpu_set_stage_copy, else the environment)
enum { STAGE_DMA = 0, STAGE_KOUT, STAGE_KERNEL };

// one staged leg: a kernel over the host side's device view (dview) when
// the mode asks for one and the view exists, else the DMA engine
void stage_leg(const char *name, int mode, void *dst, const void *src, size_t bytes,
               bool to_host, const void *dview, hipStream_t st)
{
    const bool kern = dview && (mode == STAGE_KERNEL || (mode == STAGE_KOUT && to_host));
    hipError_t e;
    if (kern)
        e = to_host ? osgpu::launch_host_copy(const_cast<void *>(dview), src, bytes, st)
                    : osgpu::launch_host_copy(dst, dview, bytes, st);
    else
        e = hipMemcpyAsync(dst, src, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice,
                           st);
    launched(name, "staging copy", e);
}

void run_staged(const Call &c, StageSet &S)
{
    const size_t s = type_size(c.type);
    const size_t C = S.slot / s;                       // elements per chunk
    const size_t N = (size_t) c.nreduce;
    const size_t nchunks = (N + C - 1) / C;
    t_last_path = OSGPU_RAN_STAGED;
    const int P = c.PE_size, idx = c.index_of(c.me);
    const bool overlap = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes) &&
                         c.target != c.source;
    HostTmp tmp(c, c.target, overlap, c.nbytes);
    char *result = tmp.out;
    const char *src = (const char *) c.source;
    std::vector<const void *> sp(P);
    std::vector<void *> dp(P);
    // pinned bounce slots for pageable arrays: in[2], out[2] of S.slot bytes
    const bool bounce_in = !host_pinned(c.source), bounce_out = !host_pinned(result);
    char *bounce = (bounce_in || bounce_out)
                       ? (char *) host_stage(c.name, c.me, 4 * S.slot) : nullptr;
    auto bin = [&](int sl) { return bounce + (size_t) sl * S.slot; };
    auto bout = [&](int sl) { return bounce + (size_t) (2 + sl) * S.slot; };
    // the GPU's view of the host side of each leg (null: DMA engine)
    const int cmode = stage_copy_mode();
    char *bounce_dev = nullptr;
    if (bounce && cmode != STAGE_DMA &&
        hipHostGetDevicePointer((void **) &bounce_dev, bounce, 0) != hipSuccess) {
        (void) hipGetLastError();
        bounce_dev = nullptr;
    }
    auto view = [&](const char *h, bool is_bounce, size_t n) -> const void * {
        if (cmode == STAGE_DMA) return nullptr;
        if (is_bounce) return bounce_dev ? bounce_dev + (h - bounce) : nullptr;
        return host_device_view(h, n);
    };
    auto chunk_n = [&](size_t ch) { return (ch + 1) * C <= N ? C : N - ch * C; };
    // D2H of chunk ch landed in bout: copy it to the caller's array
    auto drain = [&](size_t ch) {
        if (bounce_out) par_memcpy(result + ch * C * s, bout((int) (ch & 1)), chunk_n(ch) * s);
    };

    auto h2d = [&](size_t ch) {
        const size_t n = chunk_n(ch);
        const char *from = src + ch * C * s;
        if (bounce_in) {  // bin[ch & 1] is free: its previous H2D was waited for
            par_memcpy(bin((int) (ch & 1)), from, n * s);
            from = bin((int) (ch & 1));
        }
        stage_leg(c.name, cmode, S.in(idx, ch & 1), from, n * s, false, view(from, bounce_in, n * s),
                  S.st_in);
        HIPCHK(c.name, hipEventRecord(S.ev_in[ch & 1], S.st_in));
    };
    entry_sync(c.name);
    h2d(0);
    for (size_t ch = 0; ch < nchunks; ch++) {
        const int sl = (int) (ch & 1);
        const size_t n = chunk_n(ch);
        if (ch + 1 < nchunks) h2d(ch + 1);   // slot reuse is safe: team(ch-1) ended everywhere
        HIPCHK(c.name, hipEventSynchronize(S.ev_in[sl]));
        if (ch >= 2) {  // my out slot (and its bounce) drained
            HIPCHK(c.name, hipEventSynchronize(S.ev_out[sl]));
            drain(ch - 2);
        }
        barrier(c);  // chunk ch staged on every PE, every out[sl] free
        if (P == 1) {
            const void *one = S.in(0, sl);
            launched(c.name, "combine launch",
                     osgpu::launch_combine(c.type, c.op, S.out(0, sl), &one, 1, n, S.st_c));
        } else if (P <= osgpu::kMaxTeam) {
            long long lo = 0, hi = 0;
            shard_of((long long) n, P, idx, s, &lo, &hi);
            for (int i = 0; i < P; i++) {
                sp[i] = S.in(i, sl) + (size_t) lo * s;
                dp[i] = S.out(i, sl) + (size_t) lo * s;
            }
            if (hi > lo)
                launched(c.name, "team launch",
                         osgpu::launch_team(c.type, c.op, P, dp.data(), sp.data(),
                                            (size_t) (hi - lo), S.st_c, S.ndev > 1));
        } else {  // large active sets: every PE folds its own chunk (pull form)
            std::vector<int> order(P);
            fold_order(c.me, c.PE_start, c.step, P, order.data());
            for (int k = 0; k < P; k++) sp[k] = S.in((order[k] - c.PE_start) / c.step, sl);
            launched(c.name, "combine launch",
                     osgpu::launch_combine(c.type, c.op, S.out(idx, sl), sp.data(), P, n, S.st_c));
        }
        stream_wait(c.name, S.st_c);
        barrier(c);  // every shard of my out[sl] written
        char *to = bounce_out ? bout(sl) : result + ch * C * s;
        stage_leg(c.name, cmode, to, S.out(idx, sl), n * s, true, view(to, bounce_out, n * s), S.st_out);
        HIPCHK(c.name, hipEventRecord(S.ev_out[sl], S.st_out));
    }
    stream_wait(c.name, S.st_out);
    for (size_t ch = nchunks >= 2 ? nchunks - 2 : 0; ch < nchunks; ch++) drain(ch);
    tmp.finish(c.nbytes);
}

// Host symmetric-heap arguments: the data arrives and leaves through host
// memory (the UCX heap).  Peers' sources are pulled with the runtime's
// shmem_getmem (src/putget.h:539-561), like the reference, but in large
// chunks into pinned staging, then combined on the GPU.
// The chunk loop between the two barriers of every GETMEM form: the fold of
// c.nreduce elements from `off` bytes into c.source, read on the members
// `pes` in that order, into `result` (the target or its temporary).  Per
// chunk of host_chunk_bytes(): every input into its pinned slot (getmem, or
// memcpy of my own), H2D, one launch of `launch` (launch_combine, or
// launch_combine_shifted where the slots' 16-byte phases may differ from the
// caller's arrays'), D2H, wait, memcpy to the result.
void getmem_chunks(const Call &c, const std::vector<int> &pes, size_t off,
                   decltype(&osgpu::launch_combine) launch, char *result)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const size_t s = type_size(c.type), N = (size_t) c.nreduce;
    const int K = (int) pes.size();
    const size_t chunk = host_chunk_elems(host_chunk_bytes(), s, N), cb = chunk * s;
    // device: K input slots + 1 output slot; pinned: K input slots + output
    // (a slot of cb bytes need not be a multiple of 16)
    char *dbuf = (char *) device_scratch(c.name, c.me, cb * (K + 1));
    char *hbuf = (char *) host_stage(c.name, c.me, cb * (K + 1));
    std::vector<const void *> srcs(K);
    for (int k = 0; k < K; k++) srcs[k] = dbuf + (size_t) k * cb;
    char *dout = dbuf + (size_t) K * cb, *hout = hbuf + (size_t) K * cb;
    const char *mine = (const char *) c.source + off;

    scan_for_chunks(N, chunk, [&](size_t at, size_t n) {
        const size_t nb = n * s;
        for (int k = 0; k < K; k++) {
            char *hk = hbuf + (size_t) k * cb;
            if (pes[k] == c.me) memcpy(hk, mine + at * s, nb);
            else c.ops.getmem(hk, mine + at * s, nb, pes[k]);
            HIPCHK(c.name, hipMemcpyAsync((void *) srcs[k], hk, nb, hipMemcpyHostToDevice, st));
        }
        launched(c.name, "combine launch", launch(c.type, c.op, dout, srcs.data(), K, n, st));
        HIPCHK(c.name, hipMemcpyAsync(hout, dout, nb, hipMemcpyDeviceToHost, st));
        stream_wait(c.name, st);
        memcpy(result + at * s, hout, nb);
    });
}

void run_host(const Call &c)
{
    t_last_path = OSGPU_RAN_GETMEM;
    const bool overlap = c.PE_size > 1 && ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    HostTmp result(c, c.target, overlap, c.nbytes);
    barrier(c);  // src/reductions.c:82
    getmem_chunks(c, caller_first(c), 0, osgpu::launch_combine, result.out);
    barrier(c);  // src/reductions.c:113
    result.finish(c.nbytes);  // src/reductions.c:114-119
}

// long double: bytes 10..15 of each of the n slots a COPY wrote at p are zero,
// as after a fold
void zero_ld_padding(int type, void *p, size_t n)
{
    if (type != osgpu::T_LONGDOUBLE) return;
    for (size_t i = 0; i < n; i++) memset((char *) p + 16 * i + 10, 0, 6);
}

// Small calls on HOST symmetric-heap memory (each PE pulling at most the host
// fold's limit from its peers, automatic host path): the reference's
// algorithm on this PE's thread with the kernels' element ops compiled for the host (host_fold.hip)
// -- the source copied into the target, barrier (src/reductions.c:82), every
// other PE's whole source pulled with ONE shmem_getmem (the reference pulls
// 64 elements per getmem, :90-103) and folded in this PE's order (:84-111),
// barrier (:113), the temporary target copied back on overlap (:114-119).
// No GPU round trip: below this size the fastest GPU form (one fused launch
// reading and writing the host heap over PCIe) costs more than the whole
// loop.
// The table form, for every caller-first collective: accs[i] takes my own
// sources[i] BEFORE the entry barrier, then every peer's in my fold order.
// An accumulator is the entry's target, or the caller's temporary where the
// target overlaps what peers still read; the caller copies it back.
void host_fold_table(const Call &c, int M, void *const *accs, const void *const *sources,
                     const size_t *bytes, const size_t *nelems)
{
    t_last_path = OSGPU_RAN_HOST_FOLD;
    const int P = c.PE_size;
    const std::vector<int> order = caller_first(c);
    thread_local std::vector<unsigned char> peer;
    if (P > 1) peer.resize(*std::max_element(bytes, bytes + M));
    const bool ok = many_host_fold(  // the own copies: :79-81
        M, accs, sources, bytes, nelems, P > 1 ? peer.data() : nullptr, order.data(), P,
        [&](void *dst, const void *src, size_t n, int pe) { c.ops.getmem(dst, src, n, pe); },
        [&](void *a, const void *in, size_t n, int) { return osgpu::host_fold(c.type, c.op, a, in, n); },
        [&] {
            // long double: bytes 10..15 of every written slot are zero on every
            // path (longdouble.hip).  The folds write them so; a set of one PE
            // has no fold, and the copy would carry the source's padding along
            if (P == 1)
                for (int i = 0; i < M; i++) zero_ld_padding(c.type, accs[i], nelems[i]);
            barrier(c);  // :82 -- every source is ready
        });
    if (!ok) fatal(c.name, "host fold: type %d op %d", c.type, c.op);
    barrier(c);  // :113 -- every peer is done reading my sources
}

// One array: c.nreduce elements at `mine` (c.source, or a block of it) into
// c.target; `overlap`: the target shares bytes with my source (:114-119).
void run_host_fold(const Call &c, const void *mine, bool overlap)
{
    thread_local std::vector<unsigned char> tmp;
    if (overlap) tmp.resize(c.nbytes);
    void *acc = overlap ? (void *) tmp.data() : c.target;
    const size_t n = (size_t) c.nreduce;
    host_fold_table(c, 1, &acc, &mine, &c.nbytes, &n);
    if (overlap) memcpy(c.target, acc, c.nbytes);
}

void to_all(const char *name, int type, int op, void *target, void *source, int nreduce,
            int PE_start, int logPE_stride, int PE_size, void *pWrk, long *pSync)
{
    (void) pWrk;  // the combine needs no bounce buffer: peers are read directly
    Call c;
    if (!begin_call(c, name, type, op, target, source, nreduce, PE_start, logPE_stride, PE_size,
                    pSync, nreduce <= 0))
        return;
    c.nbytes = type_size(type) * (size_t) nreduce;  // no int overflow (cf. :44)

    int dt = -1;
    const Array arrays[] = {{target, c.nbytes}, {source, c.nbytes}};
    if (arrays_kind(c, arrays, 2, &dt) == MEM_HOST) {
        const int hp = host_path();
        if (host_route_fold(c, hp, (size_t) (c.PE_size - 1) * c.nbytes,
                            osgpu::host_fold_supported(type, op), nullptr)) {
            run_host_fold(c, source, ranges_overlap(target, c.nbytes, source, c.nbytes));
            return;
        }
        StageSet *S = hp == OSGPU_HOST_GETMEM ? nullptr : stage_setup(c);
        // small calls on host heaps pinned with osgpu_host_register (on every
        // PE, like the heap itself): H2D, exchange and D2H in one launch
        void *hin = nullptr, *hout = nullptr;
        SyncSet *Y = nullptr;
        if (S && fused_eligible(c, true) && c.nbytes <= S->slot &&
            (hin = host_device_view(source, c.nbytes)) &&
            (hout = host_device_view(target, c.nbytes)) && (Y = sync_setup(c))) {
            std::vector<const void *> srcs(c.PE_size);
            std::vector<void *> dsts(c.PE_size);
            for (int i = 0; i < c.PE_size; i++) {
                srcs[i] = S->in(i, 0);
                dsts[i] = S->out(i, 0);
            }
            run_fused(c, *Y, srcs, dsts, true, S, hin, hout);
        } else if (S) {
            run_staged(c, *S);
        } else {
            run_host(c);
        }
        return;
    }
    const DeviceGuard on_device(name, dt);
    const int mode = path_mode();
    std::vector<const void *> srcs;
    std::vector<void *> dsts;
    int idx = -1;
    bool remote = false;
    SyncSet *S = nullptr;
    // RCCL only where its result is the reference's: integer (type, op)s on
    // the automatic path when no device heap is registered; FP sum/prod only
    // when the caller forces OSGPU_PATH_RCCL (tolerance, not bit-exact); FP
    // min/max never (they take the exact kernels even when RCCL is forced),
    // and the extension types (half, bfloat16) never: rccl_types has no row
    // for them, so they run the exact kernels under every setting.
    if (mode == OSGPU_PATH_RCCL && rccl_usable(c, true)) {
        run_rccl(c);
    } else if (mode != OSGPU_PATH_PULL && (idx = team_ptrs(c, srcs, dsts, &remote)) >= 0) {
        StageSet *G = nullptr;
        if (fused_eligible(c, true) && (S = sync_setup(c)))
            run_fused(c, *S, srcs, dsts, true);
        else if (team_exchange() == 1 && c.ops.getmem && (G = stage_setup(c)))
            run_team_push(c, srcs, dsts, idx, *G);
        else
            run_team(c, srcs, dsts, idx, remote);
    } else if (symmetric_ptrs(c, c.source, c.nbytes, srcs)) {  // both pull forms
        if (fused_eligible(c, false) && (S = sync_setup(c)))
            run_fused(c, *S, srcs, dsts, false);
        else
            run_p2p(c, srcs);
    } else if (mode == OSGPU_PATH_AUTO && rccl_usable(c, false)) {
        run_rccl(c);
    } else {
        fatal(name,
              "device-resident arguments need every active PE's device heap registered "
              "(osgpu_heap_create / osgpu_heap_register), or -- integer types only, or FP "
              "sum/prod under OSGPU_PATH_RCCL -- an RCCL communicator over the whole job "
              "(path mode %d)",
              mode);
    }
}

// ------------------------------------------------------- reduce-scatter
//
// osgpu_reduce_scatter: member m of the set receives block m -- elements
// [m * nreduce, (m + 1) * nreduce) -- of what the reduce-to-all over the same
// P * nreduce element sources would leave in its target, bit for bit: the
// same fold order and element rules over a P-th of the elements.  `c.nbytes`
// is the block's size; the byte arithmetic is rscatter_host.hpp's (size_t).
// Paths: device heaps the pull form; host heaps the host fold and GETMEM.
// No FUSED, STAGED, RCCL or owner-push form.

// Device heaps, every member's registered: run_p2p over block m of every
// member's source.  Block m starts m * nreduce * size bytes into a source and
// the target sits at its own address, so the pointers' 16-byte phases differ
// unless the block is a multiple of 16 bytes: launch_combine_shifted.
void run_rs_pull(const Call &c, const RsBlock &b)
{
    const int P = c.PE_size;
    std::vector<const void *> srcs(P);  // block m of every source, in this PE's fold order
    if (!fold_sources(c, caller_first(c), c.source, b.source_bytes, b.offset, srcs.data()))
        no_device_heap(c, "source", b.source_bytes);
    DBG("%s PE %d: pull path, block %d of %d, %zu bytes at %zu", c.name, c.me, c.index_of(c.me), P,
        b.bytes, b.offset);
    const bool overlap = P > 1 && ranges_overlap(c.target, b.bytes, c.source, b.source_bytes);
    run_pull(c, b.bytes, overlap, [&](void *out, hipStream_t st) {
        launched(c.name, "combine launch",
                 osgpu::launch_combine_shifted(c.type, c.op, out, srcs.data(), P,
                                               (size_t) c.nreduce, st));
    });
}

// Host heaps above the host fold's limit: run_host restricted to block m.
void run_rs_host(const Call &c, const RsBlock &b)
{
    t_last_path = OSGPU_RAN_GETMEM;
    const bool overlap =
        c.PE_size > 1 && ranges_overlap(c.target, b.bytes, c.source, b.source_bytes);
    HostTmp result(c, c.target, overlap, b.bytes);
    barrier(c);  // every source is ready
    getmem_chunks(c, caller_first(c), b.offset, osgpu::launch_combine_shifted, result.out);
    barrier(c);  // every peer is done reading my source
    result.finish(b.bytes);
}

void reduce_scatter(const char *name, int type, int op, void *target, const void *source,
                    int nreduce, int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    require_reduction(name, type, op, "osgpu_has_reduce_scatter");
    Call c;
    if (!begin_call(c, name, type, op, target, source, nreduce, PE_start, logPE_stride, PE_size,
                    pSync, nreduce <= 0))
        return;
    RsBlock b;
    if (!rs_block(type_size(type), nreduce, PE_size, c.index_of(c.me), &b))
        fatal(name, "%d blocks of %d elements do not fit the address space", PE_size, nreduce);
    c.nbytes = b.bytes;

    int dt = -1;
    const Array arrays[] = {{target, b.bytes}, {source, b.source_bytes}};
    if (arrays_kind(c, arrays, 2, &dt) == MEM_HOST) {
        // the host fold: run_host_fold over block m, one shmem_getmem of the
        // block per peer ((P - 1) blocks pulled)
        if (host_route_fold(c, host_path(), b.pulled_bytes, osgpu::host_fold_supported(type, op),
                            "the reduce-scatter"))
            run_host_fold(c, (const char *) source + b.offset,
                          ranges_overlap(target, b.bytes, source, b.source_bytes));
        else
            run_rs_host(c, b);
        return;
    }
    const DeviceGuard on_device(name, dt);
    run_rs_pull(c, b);  // under every OSGPU_REDUCE_PATH setting; RCCL never serves it
}

// ------------------------------------------------- batched reduce-to-all
//
// osgpu_reduce_many: a table of independent reduce-to-all calls of one type,
// op and active set between ONE pair of barriers.  Every targets[i] ends up,
// bit for bit, as the single call on (targets[i], sources[i], nreduces[i])
// would leave it.  Paths: device heaps the pull form with one
// launch_combine_many; host heaps the host fold and GETMEM.  No TEAM, FUSED,
// STAGED or RCCL form, one type and op per call.

// the non-empty entries of the table; c (a Call) carries set, type and op
struct Many {
    std::vector<void *> target;
    std::vector<const void *> source;
    std::vector<size_t> n, bytes;
    size_t total = 0;  // bytes over all entries
    int count() const { return (int) target.size(); }
};

// Where entry i's result goes while peers may still read what its target
// overlaps: one temporary region for the whole table, each slot at its
// target's 16-byte phase (the batch kernel wants target and sources at one
// phase).  off[i] == (size_t) -1: the target itself.
struct ManyTmp {
    std::vector<size_t> off;
    size_t bytes = 0;
    // peers: somebody else reads the sources (or the path copies its own first)
    ManyTmp(const Many &m, bool peers) : off((size_t) m.count(), (size_t) -1)
    {
        for (int i = 0; i < m.count(); i++) {
            if (!peers || !ranges_overlap(m.target[i], m.bytes[i], m.source[i], m.bytes[i]))
                continue;
            off[i] = bytes + ((uintptr_t) m.target[i] & 15);
            bytes = (off[i] + m.bytes[i] + 15) & ~(size_t) 15;
        }
    }
    bool used(int i) const { return off[i] != (size_t) -1; }
};

void run_many_pull(const Call &c, const Many &m)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const int P = c.PE_size, M = m.count();
    const std::vector<int> order = caller_first(c);
    // every entry's source on every member, in this PE's fold order
    std::vector<const void *> srcs((size_t) M * P);
    std::vector<const void *const *> rows(M);
    for (int i = 0; i < M; i++) {
        if (!fold_sources(c, order, m.source[i], m.bytes[i], 0, &srcs[(size_t) i * P]))
            no_device_heap(c, "source of a non-empty entry", m.bytes[i]);
        rows[i] = &srcs[(size_t) i * P];
    }
    t_last_path = OSGPU_RAN_PULL;
    DBG("%s PE %d: pull path, %d arrays, %zu bytes", c.name, c.me, M, m.total);
    entry_sync(c.name, st);
    barrier(c);  // every source of every entry is ready
    const ManyTmp tmp(m, P > 1);
    char *scratch = tmp.bytes ? (char *) device_scratch(c.name, c.me, tmp.bytes) : nullptr;
    std::vector<void *> outs(M);
    for (int i = 0; i < M; i++) outs[i] = tmp.used(i) ? scratch + tmp.off[i] : m.target[i];
    launched(c.name, "combine launch",
             osgpu::launch_combine_many(c.type, c.op, M, outs.data(), rows.data(), P, m.n.data(),
                                        st));
    stream_wait(c.name, st);
    barrier(c);  // peers are done reading my sources
    if (tmp.bytes) {
        std::vector<osgpu::CopySeg> segs;
        for (int i = 0; i < M; i++)
            if (tmp.used(i)) segs.push_back({outs[i], m.target[i], m.bytes[i]});
        for_batches(segs, osgpu::kMaxCopySegs, [&](const osgpu::CopySeg *b, int k) {
            launched(c.name, "copy launch", osgpu::launch_copy(b, k, st));
        });
        stream_wait(c.name, st);
    }
}

void run_many_host_fold(const Call &c, const Many &m)
{
    const int M = m.count();
    // (the host fold copies its own source first, so any overlap takes a temporary, as run_host_fold)
    const ManyTmp tmp(m, true);
    thread_local std::vector<unsigned char> tbuf;
    tbuf.resize(tmp.bytes);
    std::vector<void *> accs(M);
    for (int i = 0; i < M; i++) accs[i] = tmp.used(i) ? (void *) (tbuf.data() + tmp.off[i]) : m.target[i];
    host_fold_table(c, M, accs.data(), m.source.data(), m.bytes.data(), m.n.data());
    for (int i = 0; i < M; i++)
        if (tmp.used(i)) memcpy(m.target[i], accs[i], m.bytes[i]);
}

void run_many_host(const Call &c, const Many &m)
{
    t_last_path = OSGPU_RAN_GETMEM;
    const int M = m.count();
    const ManyTmp tmp(m, c.PE_size > 1);
    std::vector<unsigned char> tbuf(tmp.bytes);
    const std::vector<int> order = caller_first(c);
    barrier(c);  // every source is ready
    for (int i = 0; i < M; i++) {
        Call e = c;
        e.target = m.target[i];
        e.source = const_cast<void *>(m.source[i]);
        e.nreduce = (int) m.n[i];
        e.nbytes = m.bytes[i];
        getmem_chunks(e, order, 0, osgpu::launch_combine,
                      tmp.used(i) ? (char *) tbuf.data() + tmp.off[i] : (char *) m.target[i]);
    }
    barrier(c);  // every peer is done reading my sources
    for (int i = 0; i < M; i++)
        if (tmp.used(i)) memcpy(m.target[i], tbuf.data() + tmp.off[i], m.bytes[i]);
}

void reduce_many(const char *name, int type, int op, int count, void *const *targets,
                 const void *const *sources, const int *nreduces, int PE_start, int logPE_stride,
                 int PE_size, long *pSync)
{
    require_reduction(name, type, op, "osgpu_has_reduce_many");
    if (count < 0) fatal(name, "count %d is negative", count);
    if (count > 0 && (!targets || !sources || !nreduces))
        fatal(name, "a table of %d entries needs targets, sources and nreduces", count);
    Many m;
    const size_t s = type_size(type);
    for (int i = 0; i < count; i++) {
        if (nreduces[i] <= 0) continue;
        m.target.push_back(targets[i]);
        m.source.push_back(sources[i]);
        m.n.push_back((size_t) nreduces[i]);
        m.bytes.push_back(s * (size_t) nreduces[i]);
        m.total += m.bytes.back();
    }
    const int M = m.count();
    Call c;  // (the set, type and op; the arrays are the table's)
    if (!begin_call(c, name, type, op, nullptr, nullptr, 0, PE_start, logPE_stride, PE_size, pSync,
                    M == 0))
        return;
    {   // the table's contract, before the first barrier
        std::vector<uintptr_t> ta(M), sa(M);
        for (int i = 0; i < M; i++) ta[i] = (uintptr_t) m.target[i], sa[i] = (uintptr_t) m.source[i];
        int other = -1;
        const int bad = many_overlap(M, ta.data(), sa.data(), m.bytes.data(), &other);
        if (bad >= 0)
            fatal(name, "the target of one entry overlaps the target or source of another "
                        "(non-empty entries %d and %d)", bad, other);
    }
    std::vector<Array> arrays;  // the first target first: its device is the call's
    for (int i = 0; i < M; i++) arrays.push_back({m.target[i], m.bytes[i]});
    for (int i = 0; i < M; i++) arrays.push_back({m.source[i], m.bytes[i]});
    int dev = -1;
    if (arrays_kind(c, arrays.data(), arrays.size(), &dev, true) == MEM_HOST) {
        if (host_route_fold(c, host_path(), (size_t) (c.PE_size - 1) * m.total,
                            osgpu::host_fold_supported(type, op), "the batched reduce"))
            run_many_host_fold(c, m);
        else
            run_many_host(c, m);
        return;
    }
    const DeviceGuard on_device(name, dev);
    run_many_pull(c, m);  // under every OSGPU_REDUCE_PATH setting
}

// ---------------------------------------------------------- prefix scans
//
// osgpu_scan: member m of the set receives the fold of the sources of members
// 0..m (inclusive) or 0..m-1 (exclusive; member 0 the op's identity), in
// ascending member order for EVERY member -- bit for bit what member 0 would
// receive from the reduce-to-all over the sub-set of those members.
// Paths: device heaps the owner-computes team kernel (launch_team_scan) or the
// pull form; host heaps the host fold and GETMEM.  No FUSED, STAGED, RCCL or
// push form, no long double team form, no local merge.
// The byte arithmetic and the identities are scan_host.hpp's.

static_assert((int) SCAN_T_SHORT == (int) OSGPU_T_SHORT &&
                  (int) SCAN_T_LONGDOUBLE == (int) OSGPU_T_LONGDOUBLE &&
                  (int) SCAN_T_COMPLEXD == (int) OSGPU_T_COMPLEXD &&
                  (int) SCAN_T_HALF == (int) OSGPU_T_HALF &&
                  (int) SCAN_T_BFLOAT16 == (int) OSGPU_T_BFLOAT16 &&
                  (int) SCAN_OP_SUM == (int) OSGPU_OP_SUM && (int) SCAN_OP_XOR == (int) OSGPU_OP_XOR &&
                  (int) SCAN_OP_MIN == (int) OSGPU_OP_MIN,
              "scan_host.hpp repeats the codes of osgpu_reduce.h");

// TEAM of the scan and the uniform reduce (`what`): every member launches the
// kernel, launch(P, dsts, srcs, n, stream), over its own contiguous shard of
// all P targets, between the two barriers.  (No tiles / merge scheme of local
// members: run_team's bookkeeping is the reduce-to-all's.)  cut_elem: the
// element size shard_of cuts by when it is not the type's (osgpu_reduce_loc:
// a second stream of 4-byte elements shares the boundaries).
template <class Launch>
void run_team_shards(const Call &c, const std::vector<const void *> &srcs,
                     const std::vector<void *> &dsts, int idx, const char *what, Launch launch,
                     size_t cut_elem = 0)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const size_t s = type_size(c.type);
    const int P = c.PE_size;
    t_last_path = OSGPU_RAN_TEAM;
    entry_sync(c.name, st);
    barrier(c);  // every source is ready, every target writable
    long long lo = 0, hi = 0;
    shard_of(c.nreduce, P, idx, cut_elem ? cut_elem : s, &lo, &hi);
    std::vector<const void *> sp(P);
    std::vector<void *> dp(P);
    for (int i = 0; i < P; i++) {
        sp[i] = (const char *) srcs[i] + (size_t) lo * s;
        dp[i] = (char *) dsts[i] + (size_t) lo * s;
    }
    DBG("%s PE %d: %s, [%lld, %lld) of %d, P=%d", c.name, c.me, what, lo, hi, c.nreduce, P);
    if (hi > lo) launched(c.name, what, launch(P, dp.data(), sp.data(), (size_t) (hi - lo), st));
    stream_wait(c.name, st);
    barrier(c);  // every shard of my target is written
}

// PULL of the first K members of the set: the caller folds their sources
// itself, ascending (launch_combine_shifted: the target may sit at another
// 16-byte phase); one input is a copy, none the identity fill.  The scan's
// member m takes K = scan_prefix_len, the uniform reduce K = PE_size.
void run_prefix_pull(const Call &c, int K)
{
    std::vector<const void *> srcs(K);
    if (!fold_sources(c, ascending(c, K), c.source, c.nbytes, 0, srcs.data()))
        no_device_heap(c, "source", c.nbytes);
    DBG("%s PE %d: pull over the first %d members, ascending", c.name, c.me, K);
    // (member 0's identity too: peers read the source its target may overlap)
    const bool overlap = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    run_pull(c, c.nbytes, overlap, [&](void *out, hipStream_t st) {
        if (K == 0)
            launched(c.name, "identity fill launch",
                     osgpu::launch_scan_fill(c.type, c.op, out, (size_t) c.nreduce, st));
        else
            launched(c.name, "combine launch",
                     osgpu::launch_combine_shifted(c.type, c.op, out, srcs.data(), K,
                                                   (size_t) c.nreduce, st));
    });
}

// member j's bytes [off, off + nb) of the symmetric host array `array` as
// this member sees them: its own array, or one getmem into `buf`
const void *host_input(const Coll &c, const void *array, int j, size_t off, size_t nb, void *buf)
{
    const int pe = c.pe_at(j);
    const char *src = (const char *) array + off;
    if (pe == c.me) return src;
    c.ops.getmem(buf, src, nb, pe);
    return buf;
}

// Host heaps, the last member's pull ((P - 1) arrays) within the host fold's
// limit: the fold of the first K members on this PE's thread,
// ascending -- the caller's own source in its place in the order -- one
// getmem of the whole array per peer it folds.
void run_prefix_host_fold(const Call &c, int K)
{
    t_last_path = OSGPU_RAN_HOST_FOLD;
    const bool overlap = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    thread_local std::vector<unsigned char> tmp, peer;
    if (overlap) tmp.resize(c.nbytes);
    if (K > 0) peer.resize(c.nbytes);
    void *acc = overlap ? (void *) tmp.data() : c.target;
    barrier(c);  // every source is ready
    if (K == 0) {
        if (!scan_fill_identity(c.type, c.op, acc, (size_t) c.nreduce))
            fatal(c.name, "no identity for type %d op %d", c.type, c.op);
    } else {
        memmove(acc, host_input(c, c.source, 0, 0, c.nbytes, peer.data()), c.nbytes);
        if (K == 1) zero_ld_padding(c.type, acc, (size_t) c.nreduce);
        for (int j = 1; j < K; j++)
            if (!osgpu::host_fold(c.type, c.op, acc,
                                  host_input(c, c.source, j, 0, c.nbytes, peer.data()),
                                  (size_t) c.nreduce))
                fatal(c.name, "host fold: type %d op %d", c.type, c.op);
    }
    barrier(c);  // every peer is done reading my source
    if (overlap) memcpy(c.target, acc, c.nbytes);
}

// Host heaps above that: the K inputs pulled in chunks of host_chunk_bytes()
// into pinned staging, combined on the GPU.  Member 0 of an exclusive scan
// (K == 0) writes the identity on the host.
void run_prefix_host(const Call &c, int K)
{
    t_last_path = OSGPU_RAN_GETMEM;
    const bool overlap = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    HostTmp result(c, c.target, overlap, c.nbytes);
    barrier(c);  // every source is ready
    if (K > 0)
        getmem_chunks(c, ascending(c, K), 0, osgpu::launch_combine_shifted, result.out);
    else if (!scan_fill_identity(c.type, c.op, result.out, (size_t) c.nreduce))
        fatal(c.name, "no identity for type %d op %d", c.type, c.op);
    barrier(c);  // every peer is done reading my source
    result.finish(c.nbytes);
}

void scan(const char *name, int type, int op, int exclusive, void *target, const void *source,
          int nreduce, int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    require_reduction(name, type, op, "osgpu_has_scan");
    if (exclusive != 0 && exclusive != 1)
        fatal(name, "exclusive is %d: 0 (inclusive) or 1 (exclusive)", exclusive);
    Call c;
    if (!begin_call(c, name, type, op, target, source, nreduce, PE_start, logPE_stride, PE_size,
                    pSync, nreduce <= 0))
        return;
    ScanBytes b;
    if (!scan_bytes(type_size(type), nreduce, PE_size, c.index_of(c.me), exclusive, &b))
        fatal(name, "%d arrays of %d elements do not fit the address space", PE_size, nreduce);
    c.nbytes = b.bytes;
    const int K = scan_prefix_len(c.index_of(c.me), exclusive);  // the members I fold

    int dt = -1;
    const Array arrays[] = {{target, b.bytes}, {source, b.bytes}};
    if (arrays_kind(c, arrays, 2, &dt) == MEM_HOST) {
        if (host_route_fold(c, host_path(), b.pulled_bound, osgpu::host_fold_supported(type, op),
                            "the scan"))
            run_prefix_host_fold(c, K);
        else
            run_prefix_host(c, K);
        return;
    }
    const DeviceGuard on_device(name, dt);
    std::vector<const void *> srcs;
    std::vector<void *> dsts;
    int idx = -1;
    // the team kernel under every setting but OSGPU_PATH_PULL (RCCL never
    // serves a scan); long double, an overlap, a target outside the heaps
    // and more than 8 members take the pull form
    if (path_mode() != OSGPU_PATH_PULL && type != OSGPU_T_LONGDOUBLE &&
        (idx = team_ptrs(c, srcs, dsts)) >= 0)
        run_team_shards(c, srcs, dsts, idx, exclusive ? "team exclusive scan" : "team inclusive scan",
                        [&](int P, void *const *d, const void *const *sr, size_t n, hipStream_t st) {
                            return osgpu::launch_team_scan(type, op, exclusive, P, d, sr, n, st);
                        });
    else
        run_prefix_pull(c, K);
}

// ------------------------------------------------- uniform reduce-to-all
//
// osgpu_reduce_uniform: every member receives the ONE ascending fold of all
// members' sources -- member 0's reduce-to-all result, the last member's
// inclusive scan -- so all targets hold the same bytes.  Paths: device heaps
// the owner-computes uniform kernel (launch_team_uniform, long double
// included) or the pull form; host heaps the host fold and GETMEM.  The pull
// and host forms are the scan's (run_prefix_*) over K = PE_size members: never
// osgpu_fold_order's caller-first order.  No FUSED, STAGED, RCCL or push form.

void reduce_uniform(const char *name, int type, int op, void *target, const void *source,
                    int nreduce, int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    require_reduction(name, type, op, "osgpu_has_reduce_uniform");
    Call c;
    if (!begin_call(c, name, type, op, target, source, nreduce, PE_start, logPE_stride, PE_size,
                    pSync, nreduce <= 0))
        return;
    ScanBytes b;  // the inclusive scan's byte counts: every member folds what its last one does
    if (!scan_bytes(type_size(type), nreduce, PE_size, c.index_of(c.me), 0, &b))
        fatal(name, "%d arrays of %d elements do not fit the address space", PE_size, nreduce);
    c.nbytes = b.bytes;

    int dt = -1;
    const Array arrays[] = {{target, b.bytes}, {source, b.bytes}};
    if (arrays_kind(c, arrays, 2, &dt) == MEM_HOST) {
        if (host_route_fold(c, host_path(), b.pulled_bound, osgpu::host_fold_supported(type, op),
                            "the uniform reduce"))
            run_prefix_host_fold(c, PE_size);
        else
            run_prefix_host(c, PE_size);
        return;
    }
    const DeviceGuard on_device(name, dt);
    std::vector<const void *> srcs;
    std::vector<void *> dsts;
    int idx = -1;
    // the team kernel under every setting but OSGPU_PATH_PULL (RCCL's order
    // is not this one), for every type; an overlap, a target outside the
    // heaps, one member and more than 8 take the pull form
    if (path_mode() != OSGPU_PATH_PULL && (idx = team_ptrs(c, srcs, dsts)) >= 0)
        run_team_shards(c, srcs, dsts, idx, "team uniform",
                        [&](int P, void *const *d, const void *const *sr, size_t n, hipStream_t st) {
                            return osgpu::launch_team_uniform(type, op, P, d, sr, n, st);
                        });
    else
        run_prefix_pull(c, PE_size);
}

// ------------------------------------------- max / min with location
//
// osgpu_reduce_loc: the uniform reduce's one ascending fold over pairs
// (value, 32-bit index): every member receives the extreme and where it came
// from (elem_ops.hpp LocStep).  Paths: device heaps the owner-computes kernel
// (launch_team_loc with every member's targets) or the pull form (the
// caller's targets alone, in chunks of 8 inputs); host heaps the host fold
// and GETMEM.  No FUSED, STAGED, RCCL or push form.  The byte arithmetic, the
// overlap rule and the chunk walks are loc_host.hpp's.

struct LocCall : Call {
    int *loc_target = nullptr;
    const int *loc_source = nullptr;  // null: member j's elements carry its PE number
    size_t lbytes = 0;
    int member_pe(int j) const { return pe_at(j); }
};

// TEAM: all four arrays (three without index sources) symmetric, nothing
// overlapping, 2..8 members.  Every member folds its shard of all targets.
// Shards are cut with element size min(sizeof(T), 4): every boundary is then
// a multiple of the kernel's group for both streams (with 8 for an 8-byte
// type the index stream would start 8 bytes off a vector on every shard but
// the first).
bool run_loc_team(const LocCall &c)
{
    const int P = c.PE_size;
    if (P < 2 || P > osgpu::kMaxTeam) return false;
    if (ranges_overlap(c.target, c.nbytes, c.source, c.nbytes) ||
        (c.loc_source && ranges_overlap(c.loc_target, c.lbytes, c.loc_source, c.lbytes)))
        return false;
    std::vector<char *> vs, vd, ls, ld;
    if (!symmetric_ptrs(c, c.source, c.nbytes, vs) || !symmetric_ptrs(c, c.target, c.nbytes, vd) ||
        !symmetric_ptrs(c, c.loc_target, c.lbytes, ld) ||
        (c.loc_source && !symmetric_ptrs(c, c.loc_source, c.lbytes, ls)))
        return false;
    const size_t s = type_size(c.type);
    std::vector<const void *> srcs(vs.begin(), vs.end());
    std::vector<void *> dsts(vd.begin(), vd.end());
    std::vector<int> member(P);
    for (int j = 0; j < P; j++) member[j] = c.member_pe(j);
    run_team_shards(
        c, srcs, dsts, c.index_of(c.me), "team max/min with location",
        [&](int np, void *const *d, const void *const *sr, size_t n, hipStream_t st) {
            const size_t lo = (size_t) ((const char *) sr[0] - (const char *) srcs[0]) / s;
            std::vector<int *> lt(np);
            std::vector<const int *> lsrc(np);
            for (int j = 0; j < np; j++) {
                lt[j] = (int *) ld[j] + lo;
                if (c.loc_source) lsrc[j] = (const int *) ls[j] + lo;
            }
            return osgpu::launch_team_loc(c.type, c.op, np, np, d, lt.data(), sr,
                                          c.loc_source ? lsrc.data() : nullptr, member.data(), n,
                                          st);
        },
        s < 4 ? s : 4);
    return true;
}

// PULL: the caller folds all P pairs itself, ascending, into its own targets:
// launches of at most 8 inputs, the pair folded so far fed back as input 0.
// A target that overlaps its source is folded into scratch and copied back
// after the exit barrier.
void run_loc_pull(const LocCall &c)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const int P = c.PE_size;
    std::vector<char *> vs, ls;
    if (!symmetric_ptrs(c, c.source, c.nbytes, vs) ||
        (c.loc_source && !symmetric_ptrs(c, c.loc_source, c.lbytes, ls)))
        no_device_heap(c, c.loc_source ? "source (and its index source)" : "source", c.nbytes);
    t_last_path = OSGPU_RAN_PULL;
    DBG("%s PE %d: pull over %d members, ascending", c.name, c.me, P);
    entry_sync(c.name, st);
    barrier(c);  // every source is ready
    const bool ov = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    const bool ol = c.loc_source && ranges_overlap(c.loc_target, c.lbytes, c.loc_source, c.lbytes);
    const size_t vslot = (c.nbytes + 15) & ~(size_t) 15;
    char *scr = ov || ol ? (char *) device_scratch(c.name, c.me, vslot + c.lbytes) : nullptr;
    void *vout = ov ? (void *) scr : c.target;
    int *lout = ol ? (int *) (scr + vslot) : c.loc_target;
    loc_for_input_chunks(P, [&](int first, int count, bool feedback) {
        const void *v[kLocMaxInputs];
        const int *l[kLocMaxInputs];
        int member[kLocMaxInputs], k = 0;
        if (feedback) v[k] = vout, l[k] = lout, member[k] = 0, k++;
        for (int j = first; j < first + count; j++, k++) {
            v[k] = vs[j];
            l[k] = c.loc_source ? (const int *) ls[j] : nullptr;
            member[k] = c.member_pe(j);
        }
        launched(c.name, "max/min with location launch",
                 osgpu::launch_team_loc(c.type, c.op, k, 1, &vout, &lout, v,
                                        c.loc_source || feedback ? l : nullptr, member,
                                        (size_t) c.nreduce, st));
    });
    stream_wait(c.name, st);
    barrier(c);  // peers are done reading my sources
    if (ov) HIPCHK(c.name, hipMemcpyAsync(c.target, vout, c.nbytes, hipMemcpyDeviceToDevice, st));
    if (ol) HIPCHK(c.name, hipMemcpyAsync(c.loc_target, lout, c.lbytes, hipMemcpyDeviceToDevice, st));
    if (ov || ol) stream_wait(c.name, st);
}

// Host heaps, small calls: the fold on this PE's thread, ascending, one
// getmem of each whole array per peer.
void run_loc_host_fold(const LocCall &c)
{
    t_last_path = OSGPU_RAN_HOST_FOLD;
    const int P = c.PE_size;
    const size_t N = (size_t) c.nreduce;
    const bool ov = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    const bool ol = c.loc_source && ranges_overlap(c.loc_target, c.lbytes, c.loc_source, c.lbytes);
    thread_local std::vector<unsigned char> tv, tl, pv, pl;
    if (ov) tv.resize(c.nbytes);
    if (ol) tl.resize(c.lbytes);
    pv.resize(c.nbytes);
    pl.resize(c.lbytes);
    void *accv = ov ? (void *) tv.data() : c.target;
    int *accl = ol ? (int *) tl.data() : c.loc_target;
    barrier(c);  // every source is ready
    memmove(accv, host_input(c, c.source, 0, 0, c.nbytes, pv.data()), c.nbytes);
    if (c.loc_source)
        memmove(accl, host_input(c, c.loc_source, 0, 0, c.lbytes, pl.data()), c.lbytes);
    else
        std::fill(accl, accl + N, c.member_pe(0));
    for (int j = 1; j < P; j++) {
        const void *bv = host_input(c, c.source, j, 0, c.nbytes, pv.data());
        const int *bl = c.loc_source
                            ? (const int *) host_input(c, c.loc_source, j, 0, c.lbytes, pl.data())
                            : nullptr;
        if (!osgpu::host_fold_loc(c.type, c.op, accv, accl, bv, bl, c.member_pe(j), N))
            fatal(c.name, "host fold: type %d op %d", c.type, c.op);
    }
    barrier(c);  // every peer is done reading my sources
    if (ov) memcpy(c.target, accv, c.nbytes);
    if (ol) memcpy(c.loc_target, accl, c.lbytes);
}

// Host heaps above that: chunks of host_chunk_bytes() (loc_chunk_elems), BOTH
// streams of a chunk pulled into pinned staging before it is folded on the
// GPU, at most 8 inputs a launch.
void run_loc_host(const LocCall &c)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const int P = c.PE_size, K = std::min(P, (int) kLocMaxInputs);
    const size_t s = type_size(c.type), N = (size_t) c.nreduce;
    t_last_path = OSGPU_RAN_GETMEM;
    const bool ov = ranges_overlap(c.target, c.nbytes, c.source, c.nbytes);
    const bool ol = c.loc_source && ranges_overlap(c.loc_target, c.lbytes, c.loc_source, c.lbytes);
    HostTmp resv(c, c.target, ov, c.nbytes), resl(c, c.loc_target, ol, c.lbytes);
    barrier(c);  // every source is ready
    // slots 0 .. K-1 the inputs, slot K the result; the value slots first
    const size_t chunk = loc_chunk_elems(host_chunk_bytes(), s, N);
    const size_t vb = chunk * s, lb = chunk * kLocIndexBytes, loff = (size_t) (K + 1) * vb;
    const size_t total = loff + (size_t) (K + 1) * lb;
    char *dbuf = (char *) device_scratch(c.name, c.me, total);
    char *hbuf = (char *) host_stage(c.name, c.me, total);
    void *dvout = dbuf + (size_t) K * vb;
    int *dlout = (int *) (dbuf + loff + (size_t) K * lb);
    scan_for_chunks(N, chunk, [&](size_t off, size_t n) {
        const size_t nvb = n * s, nlb = n * kLocIndexBytes;
        loc_for_input_chunks(P, [&](int first, int count, bool feedback) {
            const void *v[kLocMaxInputs];
            const int *l[kLocMaxInputs];
            int member[kLocMaxInputs], k = 0;
            if (feedback) v[k] = dvout, l[k] = dlout, member[k] = 0, k++;
            for (int j = first, slot = 0; j < first + count; j++, k++, slot++) {
                char *hv = hbuf + (size_t) slot * vb, *hl = hbuf + loff + (size_t) slot * lb;
                char *dv = dbuf + (size_t) slot * vb, *dl = dbuf + loff + (size_t) slot * lb;
                const void *in = host_input(c, c.source, j, off * s, nvb, hv);
                if (in != hv) memcpy(hv, in, nvb);
                HIPCHK(c.name, hipMemcpyAsync(dv, hv, nvb, hipMemcpyHostToDevice, st));
                if (c.loc_source) {
                    in = host_input(c, c.loc_source, j, off * kLocIndexBytes, nlb, hl);
                    if (in != hl) memcpy(hl, in, nlb);
                    HIPCHK(c.name, hipMemcpyAsync(dl, hl, nlb, hipMemcpyHostToDevice, st));
                }
                v[k] = dv;
                l[k] = c.loc_source ? (const int *) dl : nullptr;
                member[k] = c.member_pe(j);
            }
            launched(c.name, "max/min with location launch",
                     osgpu::launch_team_loc(c.type, c.op, k, 1, &dvout, &dlout, v,
                                            c.loc_source || feedback ? l : nullptr, member, n, st));
            stream_wait(c.name, st);  // the staging slots are reused by the next launch
        });
        char *hvout = hbuf + (size_t) K * vb, *hlout = hbuf + loff + (size_t) K * lb;
        HIPCHK(c.name, hipMemcpyAsync(hvout, dvout, nvb, hipMemcpyDeviceToHost, st));
        HIPCHK(c.name, hipMemcpyAsync(hlout, dlout, nlb, hipMemcpyDeviceToHost, st));
        stream_wait(c.name, st);
        memcpy(resv.out + off * s, hvout, nvb);
        memcpy(resl.out + off * kLocIndexBytes, hlout, nlb);
    });
    barrier(c);  // every peer is done reading my sources
    resv.finish(c.nbytes);
    resl.finish(c.lbytes);
}

void reduce_loc(const char *name, int type, int op, void *target, int *loc_target,
                const void *source, const int *loc_source, int nreduce, int PE_start,
                int logPE_stride, int PE_size, long *pSync)
{
    if (!loc_pair(type, op))
        fatal(name, "type %d op %d is no max / min with location of this library "
                    "(osgpu_has_reduce_loc)", type, op);
    LocCall c;
    c.loc_target = loc_target;
    c.loc_source = loc_source;
    if (!begin_call(c, name, type, op, target, source, nreduce, PE_start, logPE_stride, PE_size,
                    pSync, nreduce <= 0))
        return;
    LocBytes b;
    if (!loc_bytes(type_size(type), nreduce, PE_size, loc_source != nullptr, &b))
        fatal(name, "%d arrays of %d elements do not fit the address space", PE_size, nreduce);
    c.nbytes = b.vbytes;
    c.lbytes = b.lbytes;
    if (!target || !source || !loc_target) fatal(name, "a null array");
    if (const char *pair = loc_cross_overlap(target, source, b.vbytes, loc_target, loc_source,
                                             b.lbytes))
        fatal(name, "%s overlap: a value array and an index array must not share a byte", pair);

    const Array arrays[] = {
        {target, b.vbytes}, {source, b.vbytes}, {loc_target, b.lbytes}, {loc_source, b.lbytes}};
    int dev = -1;
    if (arrays_kind(c, arrays, loc_source ? 4 : 3, &dev) == MEM_HOST) {
        if (host_route_fold(c, host_path(), b.pulled_bound,
                            osgpu::host_fold_loc_supported(type, op),
                            "the max / min with location"))
            run_loc_host_fold(c);
        else
            run_loc_host(c);
        return;
    }
    const DeviceGuard on_device(name, dev);
    // the team kernel under every setting but OSGPU_PATH_PULL (RCCL never
    // serves this call); an overlap, an array outside the heaps, one member
    // and more than 8 take the pull form
    if (path_mode() == OSGPU_PATH_PULL || !run_loc_team(c)) run_loc_pull(c);
}

// ------------------------------------------- float-accumulated 16-bit sum
//
// osgpu_reduce_wsum: the uniform reduce's one ascending fold of half /
// bfloat16 sources in a FLOAT accumulator, rounded once at the end -- or not at
// all, into a float target (elem_ops.hpp WsumStep).  Paths: device heaps the
// owner-computes kernel (launch_team_wsum with every member's targets) or the
// pull form (the caller's target alone, 8 sources a launch, the float
// accumulator carried between launches); host heaps the host fold and GETMEM.
// No FUSED, STAGED, RCCL or push form.  The byte arithmetic and the chunk
// walks are wsum_host.hpp's.

static_assert((int) SCAN_T_FLOAT == (int) OSGPU_T_FLOAT, "wsum_host.hpp takes scan_host.hpp's codes");

struct WsumCall : Call {  // nbytes: one source array
    int out_type = 0;
    size_t osz = 0;     // bytes of a target element: 2 or 4
    size_t tbytes = 0;  // one target array
    size_t abytes = 0;  // one float accumulator array
};

// TEAM: source and target symmetric, not overlapping, 2..8 members.  Every
// member folds its shard of all targets.  Shards are cut by the 2-byte source
// element, so a boundary is a multiple of 8 elements: 16 bytes of the source
// stream and 32 of a float target's.
bool run_wsum_team(const WsumCall &c)
{
    const int P = c.PE_size;
    if (P < 2 || P > osgpu::kMaxTeam) return false;
    if (ranges_overlap(c.target, c.tbytes, c.source, c.nbytes)) return false;
    std::vector<char *> vs, vd;
    if (!symmetric_ptrs(c, c.source, c.nbytes, vs) || !symmetric_ptrs(c, c.target, c.tbytes, vd))
        return false;
    std::vector<const void *> srcs(vs.begin(), vs.end());
    std::vector<void *> dsts(vd.begin(), vd.end());
    run_team_shards(
        c, srcs, dsts, c.index_of(c.me), "team float-accumulated sum",
        // run_team_shards moved the targets on by the source's element size:
        // they are taken from the shard's element offset instead
        [&](int np, void *const *, const void *const *sr, size_t n, hipStream_t st) {
            const size_t lo = (size_t) ((const char *) sr[0] - (const char *) srcs[0]) / kWsumSrcBytes;
            std::vector<void *> d(np);
            for (int j = 0; j < np; j++) d[j] = vd[j] + lo * c.osz;
            return osgpu::launch_team_wsum(c.type, c.out_type, np, np, d.data(), sr, nullptr, n, st);
        },
        kWsumSrcBytes);
    return true;
}

// PULL: the caller folds all P sources itself, ascending, into its own target:
// launches of at most 8 sources, the float accumulator carried from one to the
// next -- in the target itself when that is float, else in scratch -- and only
// the last launch narrows.  A target that overlaps the source is folded into
// scratch and copied back after the exit barrier.
void run_wsum_pull(const WsumCall &c)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const int P = c.PE_size;
    std::vector<char *> vs;
    if (!symmetric_ptrs(c, c.source, c.nbytes, vs)) no_device_heap(c, "source", c.nbytes);
    t_last_path = OSGPU_RAN_PULL;
    DBG("%s PE %d: pull over %d members, ascending, float accumulator", c.name, c.me, P);
    entry_sync(c.name, st);
    barrier(c);  // every source is ready
    const bool ov = ranges_overlap(c.target, c.tbytes, c.source, c.nbytes);
    const bool cs = wsum_needs_carry_scratch(P, c.osz);
    const size_t oslot = ov ? (c.tbytes + 15) & ~(size_t) 15 : 0;
    char *scr = ov || cs ? (char *) device_scratch(c.name, c.me, oslot + (cs ? c.abytes : 0)) : nullptr;
    void *out = ov ? (void *) scr : c.target;
    float *acc = cs ? (float *) (scr + oslot) : (float *) out;  // a float target carries itself
    wsum_for_source_chunks(P, [&](int first, int count, bool carry_in, bool last) {
        const void *v[kWsumMaxSources];
        for (int k = 0; k < count; k++) v[k] = vs[first + k];
        void *dst = last ? out : (void *) acc;
        launched(c.name, "float-accumulated sum launch",
                 osgpu::launch_team_wsum(c.type, last ? c.out_type : (int) OSGPU_T_FLOAT, count, 1,
                                         &dst, v, carry_in ? acc : nullptr, (size_t) c.nreduce, st));
    });
    stream_wait(c.name, st);
    barrier(c);  // peers are done reading my source
    if (ov) {
        HIPCHK(c.name, hipMemcpyAsync(c.target, out, c.tbytes, hipMemcpyDeviceToDevice, st));
        stream_wait(c.name, st);
    }
}

// Host heaps, small calls: the fold on this PE's thread, ascending, one getmem
// of the whole source per peer, in a float accumulator -- a float target that
// does not overlap the source, else a temporary narrowed or copied after the
// exit barrier.
void run_wsum_host_fold(const WsumCall &c)
{
    t_last_path = OSGPU_RAN_HOST_FOLD;
    const int P = c.PE_size;
    const size_t N = (size_t) c.nreduce;
    const bool direct = c.osz == kWsumAccBytes &&
                        !ranges_overlap(c.target, c.tbytes, c.source, c.nbytes);
    thread_local std::vector<float> tmp;
    thread_local std::vector<unsigned char> peer;
    if (!direct) tmp.resize(N);
    peer.resize(c.nbytes);
    float *acc = direct ? (float *) c.target : tmp.data();
    barrier(c);  // every source is ready
    bool ok = osgpu::host_wsum_widen(c.type, acc, host_input(c, c.source, 0, 0, c.nbytes, peer.data()), N);
    for (int j = 1; ok && j < P; j++)
        ok = osgpu::host_wsum_add(c.type, acc, host_input(c, c.source, j, 0, c.nbytes, peer.data()), N);
    barrier(c);  // every peer is done reading my source
    if (ok && !direct) {
        if (c.osz == kWsumAccBytes) memcpy(c.target, acc, c.tbytes);
        else ok = osgpu::host_wsum_narrow(c.type, c.target, acc, N);
    }
    if (!ok) fatal(c.name, "host fold: type %d", c.type);
}

// Host heaps above that: chunks of host_chunk_bytes() (wsum_chunk_elems), the
// sources of a chunk pulled into pinned staging 8 at a time and folded on the
// GPU, the float accumulator carried in device scratch.
void run_wsum_host(const WsumCall &c)
{
    hipStream_t st = pe_stream(c.name, c.me);
    const int P = c.PE_size, K = std::min(P, (int) kWsumMaxSources);
    const size_t N = (size_t) c.nreduce;
    t_last_path = OSGPU_RAN_GETMEM;
    const bool ov = ranges_overlap(c.target, c.tbytes, c.source, c.nbytes);
    HostTmp res(c, c.target, ov, c.tbytes);
    barrier(c);  // every source is ready
    // slots 0 .. K-1 the sources; then the accumulator and the result (device),
    // the result (host)
    const size_t chunk = wsum_chunk_elems(host_chunk_bytes(), N);
    const size_t sb = chunk * kWsumSrcBytes, ab = chunk * kWsumAccBytes, in = (size_t) K * sb;
    char *dbuf = (char *) device_scratch(c.name, c.me, in + 2 * ab);
    char *hbuf = (char *) host_stage(c.name, c.me, in + ab);
    float *dacc = (float *) (dbuf + in);
    void *dout = dbuf + in + ab;
    scan_for_chunks(N, chunk, [&](size_t off, size_t n) {
        const size_t nsb = n * kWsumSrcBytes, nob = n * c.osz;
        wsum_for_source_chunks(P, [&](int first, int count, bool carry_in, bool last) {
            const void *v[kWsumMaxSources];
            for (int k = 0; k < count; k++) {
                char *hv = hbuf + (size_t) k * sb, *dv = dbuf + (size_t) k * sb;
                const void *got = host_input(c, c.source, first + k, off * kWsumSrcBytes, nsb, hv);
                if (got != hv) memcpy(hv, got, nsb);
                HIPCHK(c.name, hipMemcpyAsync(dv, hv, nsb, hipMemcpyHostToDevice, st));
                v[k] = dv;
            }
            void *dst = last ? dout : (void *) dacc;
            launched(c.name, "float-accumulated sum launch",
                     osgpu::launch_team_wsum(c.type, last ? c.out_type : (int) OSGPU_T_FLOAT, count,
                                             1, &dst, v, carry_in ? dacc : nullptr, n, st));
            stream_wait(c.name, st);  // the staging slots are reused by the next launch
        });
        char *hout = hbuf + in;
        HIPCHK(c.name, hipMemcpyAsync(hout, dout, nob, hipMemcpyDeviceToHost, st));
        stream_wait(c.name, st);
        memcpy(res.out + off * c.osz, hout, nob);
    });
    barrier(c);  // every peer is done reading my source
    res.finish(c.tbytes);
}

void reduce_wsum(const char *name, int type, int out_type, void *target, const void *source,
                 int nreduce, int PE_start, int logPE_stride, int PE_size, long *pSync)
{
    if (!wsum_pair(type, out_type))
        fatal(name, "type %d with out_type %d is no float-accumulated sum of this library "
                    "(osgpu_has_reduce_wsum)", type, out_type);
    WsumCall c;
    c.out_type = out_type;
    c.osz = wsum_out_size(type, out_type);
    if (!begin_call(c, name, type, OSGPU_OP_SUM, target, source, nreduce, PE_start, logPE_stride,
                    PE_size, pSync, nreduce <= 0))
        return;
    WsumBytes b;
    if (!wsum_bytes(c.osz, nreduce, PE_size, &b))
        fatal(name, "%d arrays of %d elements do not fit the address space", PE_size, nreduce);
    c.nbytes = b.sbytes;
    c.tbytes = b.tbytes;
    c.abytes = b.abytes;
    if (!target || !source) fatal(name, "a null array");

    const Array arrays[] = {{target, b.tbytes}, {source, b.sbytes}};
    int dev = -1;
    if (arrays_kind(c, arrays, 2, &dev) == MEM_HOST) {
        if (host_route_fold(c, host_path(), b.pulled_bound, true, "the float-accumulated sum"))
            run_wsum_host_fold(c);
        else
            run_wsum_host(c);
        return;
    }
    const DeviceGuard on_device(name, dev);
    // the team kernel under every setting but OSGPU_PATH_PULL (RCCL never
    // serves this call); an overlap, a target outside the heaps, one member
    // and more than 8 take the pull form
    if (path_mode() == OSGPU_PATH_PULL || !run_wsum_team(c)) run_wsum_pull(c);
}

}  // namespace

extern "C" int osgpu_last_path(void) { return t_last_path; }

// ======================================================================
// Part 1: the 44 entry points (pshmem_* strong, shmem_* weak aliases, as in
// the reference's --enable-pshmem build, src/reductions.c:156-245)
// ======================================================================

#define OSGPU_DEFINE(_name, _type, _op, _tcode, _ocode)                        \
    extern "C" void pshmem_##_name##_##_op##_to_all(                           \
        _type *target, _type *source, int nreduce, int PE_start,               \
        int logPE_stride, int PE_size, _type *pWrk, long *pSync)               \
    {                                                                          \
        to_all("shmem_" #_name "_" #_op "_to_all", _tcode, _ocode, target,     \
               source, nreduce, PE_start, logPE_stride, PE_size, pWrk, pSync); \
    }                                                                          \
    extern "C" void shmem_##_name##_##_op##_to_all(                            \
        _type *target, _type *source, int nreduce, int PE_start,               \
        int logPE_stride, int PE_size, _type *pWrk, long *pSync)               \
        __attribute__((weak, alias("pshmem_" #_name "_" #_op "_to_all")));

#define OSGPU_DEFINE_TYPE_OPS(_name, _type, _tcode)                            \
    OSGPU_DEFINE(_name, _type, sum, _tcode, OSGPU_OP_SUM)                      \
    OSGPU_DEFINE(_name, _type, prod, _tcode, OSGPU_OP_PROD)

#define OSGPU_DEFINE_BITS(_name, _type, _tcode)                                \
    OSGPU_DEFINE(_name, _type, and, _tcode, OSGPU_OP_AND)                      \
    OSGPU_DEFINE(_name, _type, or, _tcode, OSGPU_OP_OR)                        \
    OSGPU_DEFINE(_name, _type, xor, _tcode, OSGPU_OP_XOR)

#define OSGPU_DEFINE_MINMAX(_name, _type, _tcode)                              \
    OSGPU_DEFINE(_name, _type, max, _tcode, OSGPU_OP_MAX)                      \
    OSGPU_DEFINE(_name, _type, min, _tcode, OSGPU_OP_MIN)

typedef std::complex<float> osgpu_cf;
typedef std::complex<double> osgpu_cd;

OSGPU_DEFINE_TYPE_OPS(short, short, OSGPU_T_SHORT)
OSGPU_DEFINE_TYPE_OPS(int, int, OSGPU_T_INT)
OSGPU_DEFINE_TYPE_OPS(long, long, OSGPU_T_LONG)
OSGPU_DEFINE_TYPE_OPS(longlong, long long, OSGPU_T_LONGLONG)
OSGPU_DEFINE_TYPE_OPS(float, float, OSGPU_T_FLOAT)
OSGPU_DEFINE_TYPE_OPS(double, double, OSGPU_T_DOUBLE)
OSGPU_DEFINE_TYPE_OPS(longdouble, long double, OSGPU_T_LONGDOUBLE)
OSGPU_DEFINE_TYPE_OPS(complexf, osgpu_cf, OSGPU_T_COMPLEXF)
OSGPU_DEFINE_TYPE_OPS(complexd, osgpu_cd, OSGPU_T_COMPLEXD)
OSGPU_DEFINE_BITS(short, short, OSGPU_T_SHORT)
OSGPU_DEFINE_BITS(int, int, OSGPU_T_INT)
OSGPU_DEFINE_BITS(long, long, OSGPU_T_LONG)
OSGPU_DEFINE_BITS(longlong, long long, OSGPU_T_LONGLONG)
OSGPU_DEFINE_MINMAX(short, short, OSGPU_T_SHORT)
OSGPU_DEFINE_MINMAX(int, int, OSGPU_T_INT)
OSGPU_DEFINE_MINMAX(long, long, OSGPU_T_LONG)
OSGPU_DEFINE_MINMAX(longlong, long long, OSGPU_T_LONGLONG)
OSGPU_DEFINE_MINMAX(float, float, OSGPU_T_FLOAT)
OSGPU_DEFINE_MINMAX(double, double, OSGPU_T_DOUBLE)
OSGPU_DEFINE_MINMAX(longdouble, long double, OSGPU_T_LONGDOUBLE)

// ======================================================================
// Part 1c: extension types (half, bfloat16).  Elements are 16-bit patterns;
// the same funnel as Part 1, so every path and setting applies.
// ======================================================================

#define OSGPU_DEFINE_EXT(_name, _op, _tcode, _ocode)                           \
    extern "C" void osgpu_##_name##_##_op##_reduce(                            \
        uint16_t *target, const uint16_t *source, int nreduce, int PE_start,   \
        int logPE_stride, int PE_size, uint16_t *pWrk, long *pSync)            \
    {                                                                          \
        to_all("osgpu_" #_name "_" #_op "_reduce", _tcode, _ocode, target,     \
               const_cast<uint16_t *>(source), nreduce, PE_start,              \
               logPE_stride, PE_size, pWrk, pSync);                            \
    }

#define OSGPU_DEFINE_EXT_OPS(_name, _tcode)                                    \
    OSGPU_DEFINE_EXT(_name, sum, _tcode, OSGPU_OP_SUM)                         \
    OSGPU_DEFINE_EXT(_name, prod, _tcode, OSGPU_OP_PROD)                       \
    OSGPU_DEFINE_EXT(_name, max, _tcode, OSGPU_OP_MAX)                         \
    OSGPU_DEFINE_EXT(_name, min, _tcode, OSGPU_OP_MIN)

OSGPU_DEFINE_EXT_OPS(half, OSGPU_T_HALF)
OSGPU_DEFINE_EXT_OPS(bfloat16, OSGPU_T_BFLOAT16)

extern "C" void osgpu_reduce_ext(int type, int op, void *target, const void *source, int nreduce,
                                 int PE_start, int logPE_stride, int PE_size, void *pWrk,
                                 long *pSync)
{
    if (!osgpu::rt::has_ext_op(type, op))
        osgpu::rt::fatal("osgpu_reduce_ext",
                         "type %d op %d is not an extension reduction (half = %d, bfloat16 = "
                         "%d; sum, prod, max, min)",
                         type, op, (int) OSGPU_T_HALF, (int) OSGPU_T_BFLOAT16);
    to_all("osgpu_reduce_ext", type, op, target, const_cast<void *>(source), nreduce, PE_start,
           logPE_stride, PE_size, pWrk, pSync);
}

// ======================================================================
// Part 1d: reduce-scatter (no reference counterpart: osgpu_* names only)
// ======================================================================

extern "C" void osgpu_reduce_scatter(int type, int op, void *target, const void *source,
                                     int nreduce, int PE_start, int logPE_stride, int PE_size,
                                     void *pWrk, long *pSync)
{
    (void) pWrk;  // as for the reduce-to-all: peers are read directly
    reduce_scatter("osgpu_reduce_scatter", type, op, target, source, nreduce, PE_start,
                   logPE_stride, PE_size, pSync);
}

extern "C" int osgpu_has_reduce_scatter(int type, int op)
{
    return is_reduction(type, op) ? 1 : 0;
}

// ======================================================================
// Part 1e: batched reduce-to-all (no reference counterpart)
// ======================================================================

extern "C" void osgpu_reduce_many(int type, int op, int count, void *const *targets,
                                  const void *const *sources, const int *nreduces, int PE_start,
                                  int logPE_stride, int PE_size, void *pWrk, long *pSync)
{
    (void) pWrk;  // as for the reduce-to-all: peers are read directly
    reduce_many("osgpu_reduce_many", type, op, count, targets, sources, nreduces, PE_start,
                logPE_stride, PE_size, pSync);
}

extern "C" int osgpu_has_reduce_many(int type, int op)
{
    return is_reduction(type, op) ? 1 : 0;
}

// ======================================================================
// Part 1f: prefix scans across PEs (no reference counterpart)
// ======================================================================

extern "C" void osgpu_scan(int type, int op, int exclusive, void *target, const void *source,
                           int nreduce, int PE_start, int logPE_stride, int PE_size, void *pWrk,
                           long *pSync)
{
    (void) pWrk;  // as for the reduce-to-all: peers are read directly
    scan("osgpu_scan", type, op, exclusive, target, source, nreduce, PE_start, logPE_stride,
         PE_size, pSync);
}

extern "C" int osgpu_has_scan(int type, int op)
{
    return is_reduction(type, op) ? 1 : 0;
}

extern "C" int osgpu_scan_identity(int type, int op, void *elem_out)
{
    unsigned char id[16];
    const size_t s = osgpu::rt::scan_identity(type, op, id);
    if (!elem_out || !s || !osgpu_has_scan(type, op)) {
        osgpu::rt::set_err("osgpu_scan_identity: type %d op %d is not a reduction of this library",
                           type, op);
        return OSGPU_EINVAL;
    }
    memcpy(elem_out, id, s);
    return OSGPU_OK;
}

// ======================================================================
// Part 1g: uniform reduce-to-all (no reference counterpart)
// ======================================================================

extern "C" void osgpu_reduce_uniform(int type, int op, void *target, const void *source,
                                     int nreduce, int PE_start, int logPE_stride, int PE_size,
                                     void *pWrk, long *pSync)
{
    (void) pWrk;  // as for the reduce-to-all: peers are read directly
    reduce_uniform("osgpu_reduce_uniform", type, op, target, source, nreduce, PE_start,
                   logPE_stride, PE_size, pSync);
}

extern "C" int osgpu_has_reduce_uniform(int type, int op)
{
    return is_reduction(type, op) ? 1 : 0;
}

// ======================================================================
// Part 1h: max / min with location (no reference counterpart)
// ======================================================================

extern "C" void osgpu_reduce_loc(int type, int op, void *target, int *loc_target,
                                 const void *source, const int *loc_source, int nreduce,
                                 int PE_start, int logPE_stride, int PE_size, void *pWrk,
                                 long *pSync)
{
    (void) pWrk;  // as for the reduce-to-all: peers are read directly
    reduce_loc("osgpu_reduce_loc", type, op, target, loc_target, source, loc_source, nreduce,
               PE_start, logPE_stride, PE_size, pSync);
}

extern "C" int osgpu_has_reduce_loc(int type, int op)
{
    return osgpu::rt::loc_pair(type, op) ? 1 : 0;
}

// ======================================================================
// Part 1i: float-accumulated half / bfloat16 sum (no reference counterpart)
// ======================================================================

extern "C" void osgpu_reduce_wsum(int type, int out_type, void *target, const void *source,
                                  int nreduce, int PE_start, int logPE_stride, int PE_size,
                                  void *pWrk, long *pSync)
{
    (void) pWrk;  // as for the reduce-to-all: peers are read directly
    reduce_wsum("osgpu_reduce_wsum", type, out_type, target, source, nreduce, PE_start,
                logPE_stride, PE_size, pSync);
}

extern "C" int osgpu_has_reduce_wsum(int type, int out_type)
{
    return osgpu::rt::wsum_pair(type, out_type) ? 1 : 0;
}
