"""half_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one process)
of a two-process run of the half / bfloat16 reduce-to-all on IPC device heaps
over the shared-memory PE runtime, as mp_worker.py's `ipc` mode sets it up:
small calls take the fused one-launch paths with their device-side barriers
-- the team form, the pull form (forced) and, on the pinned shared-memory
host heap, the staged form.
A member that never arrives ends the call with an error after 20 s
(osgpu_set_device_barrier) instead of a wait without bound.
usage: RANK=.. WORLD_SIZE=.. MASTER_ADDR=127.0.0.1 MASTER_PORT=.. \
       python half_worker.py OUTDIR
"""
import ctypes
import json
import os
import sys

import mp_worker  # noqa: F401  (sets sys.path for osgpu / support)
import numpy as np
import torch
import torch.distributed as dist

import osgpu
from support import peshm

CASES = (("half", "sum", 1024), ("half", "sum", 4096 + 3), ("bfloat16", "max", 1024),
         ("bfloat16", "max", 4096 + 3))


def source(t, n, rank):
    """Rank's source: the order-sensitive value mix of half_ref.py."""
    from support import half_ref
    return half_ref.order_values(t, n, 900 + rank)


def main():
    outdir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    L = osgpu.load()
    PES = peshm.init(rank, world, 1 << 24, dist)
    assert L.osgpu_set_pe_ops(PES.pes_ops()) == 0
    assert L.osgpu_set_device_barrier(20.0, 0) == 0
    torch.cuda.set_device(0)
    H = 1 << 20
    heap = torch.zeros(H, dtype=torch.uint8, device="cuda:0")
    h = (ctypes.c_char * 64)()
    assert L.osgpu_ipc_get_handle(ctypes.c_void_p(heap.data_ptr()), h) == 0
    hs = [None] * world
    dist.all_gather_object(hs, bytes(h))
    mapped = []
    for pe in range(world):
        if pe == rank:
            base = heap.data_ptr()
        else:
            base = L.osgpu_ipc_open((ctypes.c_char * 64).from_buffer_copy(hs[pe]))
            assert base, L.osgpu_last_error().decode()
            mapped.append(base)
        assert L.osgpu_heap_register(pe, ctypes.c_void_p(base), H) == 0
    psync = PES.pes_heap(rank) + (1 << 24) - 8192
    res = {"rank": rank, "out": {}, "paths": {}, "errors": {}}
    toff = 1 << 19
    wrk = (ctypes.c_byte * 4096)()

    def record(key, got):
        res["paths"][key] = osgpu.last_path()
        res["errors"][key] = L.osgpu_last_error().decode()
        res["out"][key] = got.tobytes().hex()
        assert not any(ctypes.string_at(psync, 1024)), "pSync not reset"

    # device heaps: the team form (FUSED_TEAM), then the pull form forced
    # (FUSED_PULL)
    for form, path in (("team", osgpu.PATH_AUTO), ("pull", osgpu.PATH_PULL)):
        assert L.osgpu_set_path(path) == 0
        for t, op, n in CASES:
            raw = source(t, n, rank).view(np.uint8)
            heap[:raw.size].copy_(torch.from_numpy(raw.copy()).cuda())
            heap[toff:toff + 2 * n].fill_(0xA5)
            torch.cuda.synchronize()
            dist.barrier()
            osgpu.ext_reduce(t, op)(heap.data_ptr() + toff, heap.data_ptr(), n, 0, 0, world, wrk,
                                    psync)
            torch.cuda.synchronize()
            record(f"{form}/{t}/{op}/{n}", heap[toff:toff + 2 * n].cpu().numpy())
            dist.barrier()
    assert L.osgpu_set_path(osgpu.PATH_AUTO) == 0
    # host heaps (the shared-memory symmetric heap, pinned on every PE, the
    # host fold off): H2D, exchange and D2H in one launch (FUSED_STAGED)
    hbase = PES.pes_heap(rank)
    assert L.osgpu_set_host_fold_max_bytes(0) == 0
    assert L.osgpu_host_register(ctypes.c_void_p(hbase), 1 << 23) == 0
    for t, op, n in CASES:
        raw = source(t, n, rank).view(np.uint8)
        ctypes.memmove(hbase, raw.ctypes.data, raw.size)
        ctypes.memset(hbase + toff, 0xA5, 2 * n)
        dist.barrier()
        osgpu.ext_reduce(t, op)(hbase + toff, hbase, n, 0, 0, world, wrk, psync)
        record(f"staged/{t}/{op}/{n}",
               np.frombuffer(ctypes.string_at(hbase + toff, 2 * n), np.uint8))
        dist.barrier()
    assert L.osgpu_host_unregister(ctypes.c_void_p(hbase)) == 0
    assert L.osgpu_set_host_fold_max_bytes(-1) == 0
    for p in mapped:
        L.osgpu_ipc_close(ctypes.c_void_p(p))
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
