// call_common.hpp -- per-call scaffolding shared by the host layers of the
// reduce (shmem_reduce.cpp) and the data-movement collectives
// (shmem_collect.cpp).  The schedules (which barriers, which launch, which
// bytes) stay in their run_* functions, and so do the decisions: the helpers
// here take "use a temporary" as a bool.  Not installed, not exported.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/osgpu_reduce.h"
#include "combine.hpp"
#include "runtime.hpp"

#pragma GCC visibility push(hidden)
namespace osgpu {
namespace rt {

// ------------------------------------------------------------- fused calls

// The fields every fused form shares (fused.hip protocol), the rest zeroed.
// The ++S.epoch here is the call's one and only epoch bump.
inline osgpu::FusedArgs fused_args(const Coll &c, SyncSet &S)
{
    osgpu::FusedArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < c.PE_size; i++) a.flags[i] = S.peer[i];
    a.mine = S.local;
    a.err = S.err_d;
    a.done_host = S.done_d;
    a.epoch = ++S.epoch;
    a.P = c.PE_size;
    a.me = S.idx;
    a.max_blocks = S.max_blocks;
    return a;
}

// Entry ordering, then the launch driven to completion (fused_complete).
// false: the call failed; the caller records OSGPU_RAN_FUSED_FAILED.
inline bool fused_run(const Coll &c, SyncSet &S, hipStream_t st, osgpu::FusedArgs &a,
                      const std::function<hipError_t(const osgpu::FusedArgs &)> &launch)
{
    entry_order(c.name, st);
    return fused_complete(c.name, S, st, a, launch);
}

// ------------------------------------- a target that overlaps a source

// Device heaps: the call writes `out` -- the PE's scratch when peers may
// still read what the target overlaps, else the target itself -- and
// finish() copies it to the target once every reader is done (after the
// exit barrier, or the completed fused launch).  device_scratch hands out
// one growing buffer per PE: a call holds at most one DeviceOut in scratch.
struct DeviceOut {
    const Coll &c;
    void *target;
    bool scratch;
    char *out;
    DeviceOut(const Coll &c_, void *target_, bool use_scratch, size_t scratch_bytes)
        : c(c_), target(target_), scratch(use_scratch),
          out((char *) (use_scratch ? device_scratch(c_.name, c_.me, scratch_bytes) : target_)) {}
    void finish(size_t copy_bytes, hipStream_t st) const
    {
        if (!scratch) return;
        if (copy_bytes)
            HIPCHK(c.name, hipMemcpyAsync(target, out, copy_bytes, hipMemcpyDeviceToDevice, st));
        stream_wait(c.name, st);
    }
};

// Host heaps: the same with a malloc'ed temporary target.  finish() copies;
// a path with its own scatter-back only lets it go out of scope.
struct HostTmp {
    void *target;
    bool tmp;
    char *out;
    HostTmp(const Coll &c, void *target_, bool use_tmp, size_t bytes)
        : target(target_), tmp(use_tmp), out((char *) (use_tmp ? malloc(bytes) : target_))
    {
        if (tmp && !out) fatal(c.name, "out of memory for the temporary target");
    }
    HostTmp(const HostTmp &) = delete;
    ~HostTmp() { if (tmp) free(out); }
    void finish(size_t copy_bytes) const { if (tmp) memcpy(target, out, copy_bytes); }
};

// ------------------------------------------------------- the small repeats

// `dev` is the calling thread's device for the scope
struct DeviceGuard {
    const char *where;
    int cur = 0, dev;
    DeviceGuard(const char *where_, int dev_) : where(where_), dev(dev_)
    {
        HIPCHK(where, hipGetDevice(&cur));
        if (cur != dev) HIPCHK(where, hipSetDevice(dev));
    }
    DeviceGuard(const DeviceGuard &) = delete;
    ~DeviceGuard() { if (cur != dev) HIPCHK(where, hipSetDevice(cur)); }
};

// Host symmetric-heap arguments: the data still crosses the GPU, and peers'
// memory is reached through the runtime's shmem_getmem.
inline void require_host_heaps(const Coll &c)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        fatal(c.name, "no GPU visible: the collectives run only on the GPU");
    if (!c.ops.getmem) fatal(c.name, "host-memory arguments need shmem_getmem");
}

// The whole job only (g_rccl): a subset communicator would need
// ncclCommSplit, which every PE of the parent must call -- OpenSHMEM forbids
// non-members from calling a collective on an active set.
inline bool rccl_whole_job(const Coll &c)
{
    return g_rccl.world && c.PE_start == 0 && c.step == 1 && c.PE_size == g_rccl.npes &&
           c.me == g_rccl.me;
}

// nothing moves; the collective still syncs
inline void sync_only(const Coll &c) { barrier(c); barrier(c); }

// shard g of n elements split over P owners on 16-byte boundaries
inline void shard_of(long long n, int P, int g, size_t elem_size, long long *lo, long long *hi)
{
    osgpu_shard_range(n, P, g, (int) (elem_size > 16 ? 16 : elem_size), lo, hi);
}

inline void launched(const char *where, const char *what, hipError_t e)
{
    if (e != hipSuccess) fatal(where, "%s: %s", what, hipGetErrorString(e));
}

// fn(first, count) over runs of at most `max` segments (one launch each)
template <class Seg, class Fn>
void for_batches(const std::vector<Seg> &segs, int max, Fn fn)
{
    for (size_t i = 0; i < segs.size(); i += (size_t) max)
        fn(segs.data() + i, (int) std::min(segs.size() - i, (size_t) max));
}

}  // namespace rt
}  // namespace osgpu
#pragma GCC visibility pop
