"""door_mp.py -- TEST INFRASTRUCTURE: one rank (= one PE = one process) of a
multi-process run of a reduce front door on one GPU; what the workers
tests/support/*_mp_worker.py share.  A rank is started by
tests/support/gpu_doors.py run_ranks (RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT; torch.distributed gloo for the setup, the shared-memory PE runtime
tests/support/pe_shm.c for the PE services).  Its device heap comes from
osgpu_heap_create, so a door reads a peer's source, and a team kernel writes a
peer's target, through a mapping of another process's memory.

A worker keeps its case table, its door call and its expected path:

    R = Rank("tag")
    for case in CASES:
        before = R.load([(offset, array), ...])         # 0xC3 elsewhere; a barrier
        osgpu.<door>(...)(R.base + ..., ..., R.world, R.wrk, R.psync)
        after = R.called(path, what)                    # the path, pSync reset
        got = R.check(after, before, [(offset, type, want)], what)
        R.barrier()
    R.close("<DOOR>_MP_OK")
"""
from __future__ import annotations

import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "test-resilient-osss-ucx_amd"), os.path.join(ROOT, "oracle"),
                os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import osgpu  # noqa: E402
from support import peshm  # noqa: E402
from support.rscatter_cases import dtype, esize, same_bits  # noqa: E402

HEAP = 8 << 20


class Rank:
    def __init__(self, tag):
        self.rank, self.world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        dist.init_process_group("gloo")
        self.dist = dist
        self.L = osgpu.load()
        self.PES = PES = peshm.init(self.rank, self.world, 1 << 24, dist, tag=tag)
        assert self.L.osgpu_set_pe_ops(PES.pes_ops()) == 0
        PES.pes_barrier.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        torch.cuda.set_device(0)
        hsync = PES.pes_heap(self.rank) + PES.pes_heap_bytes() - 8192
        self.psync = PES.pes_heap(self.rank) + PES.pes_heap_bytes() - 4096
        self.base = osgpu.heap_create(HEAP, 0, 0, self.world, hsync)
        self.heap = osgpu.device_view(self.base, HEAP)
        self._wrk = (ctypes.c_byte * 4096)()
        self.wrk = ctypes.addressof(self._wrk)

    def barrier(self):
        self.PES.pes_barrier(0, 0, self.world, None)

    def load(self, writes):
        """The heap filled with 0xC3, then `writes` ((offset, array) each); a
        barrier.  Returns the heap's bytes as they now are."""
        image = np.full(HEAP, 0xC3, dtype=np.uint8)
        self.heap.fill_(0xC3)
        for off, arr in writes:
            raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            image[off:off + raw.size] = raw
            self.heap[off:off + raw.size].copy_(torch.from_numpy(raw.copy()).cuda())
        torch.cuda.synchronize()
        self.barrier()
        return image

    def called(self, path, what):
        """After the door's call: it took `path` and left pSync reset.  Returns
        the heap's bytes."""
        assert osgpu.last_path() == path, (what, osgpu.last_path())
        assert not any(ctypes.string_at(self.psync, 1024)), f"{what}: pSync not reset"
        torch.cuda.synchronize()
        return self.heap.cpu().numpy()

    def check(self, after, before, targets, what):
        """targets: (offset, type, expected elements) each.  Every target equals
        its expected elements bit for bit (long double: padding zero); every
        other byte -- a source no target lies on, the 0xC3 before, between and
        after -- is as load() left it.  Returns the first target's bytes."""
        what = f"rank {self.rank} {what}"
        written = np.zeros(HEAP, dtype=bool)
        for off, t, want in targets:
            got = after[off:off + len(want) * esize(t)]
            bad = same_bits(t, got.view(dtype(t)), want)
            assert bad is None, f"{what}: element {bad} of the target at {off} differs"
            if t == "longdouble":
                assert not got.reshape(-1, 16)[:, 10:].any(), f"{what}: long double padding not zero"
            written[off:off + got.size] = True
        stray = np.flatnonzero(~written & (after != before))
        assert stray.size == 0, \
            f"{what}: byte {int(stray[0]) if stray.size else 0} outside the targets was written"
        off, t, want = targets[0]
        return after[off:off + len(want) * esize(t)]

    def close(self, token):
        del self.heap
        self.barrier()
        assert self.L.osgpu_heap_destroy(ctypes.c_void_p(self.base)) == 0
        print(token, flush=True)
