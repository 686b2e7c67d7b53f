"""loc_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one process)
of a multi-process osgpu_reduce_loc run on one GPU, started the way
tests/support/uniform_mp_worker.py is (RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT; torch.distributed gloo for the setup, the shared-memory PE runtime
tests/support/pe_shm.c for the PE services).  The device heaps come from
osgpu_heap_create, so the kernel reads a peer's two sources and writes a
peer's two targets through a mapping of another process's memory.  Prints
LOC_MP_OK when every case matched.
usage: python loc_mp_worker.py OUTDIR
"""
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
from support import loc_cases as C  # noqa: E402
from support import peshm  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    L = osgpu.load()
    PES = peshm.init(rank, world, 1 << 24, dist, tag="lc")
    assert L.osgpu_set_pe_ops(PES.pes_ops()) == 0
    PES.pes_barrier.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    torch.cuda.set_device(0)
    hsync = PES.pes_heap(rank) + PES.pes_heap_bytes() - 8192
    psync = PES.pes_heap(rank) + PES.pes_heap_bytes() - 4096
    base = osgpu.heap_create(8 << 20, 0, 0, world, hsync)
    heap = osgpu.device_view(base, 8 << 20)
    wrk = (ctypes.c_byte * 4096)()
    soff, lsoff, toff, ltoff = 0, 1 << 20, 2 << 20, 3 << 20
    # (type, op, n, target shift in elements, no index source, in place) -> the path
    for t, op, n, shift, null, inplace in (("double", "max", 4101, 0, False, False),
                                           ("short", "min", 6161, 3, False, False),
                                           ("half", "max", 777, 0, True, False),
                                           ("float", "min", 515, 0, True, False),
                                           ("int", "max", 300, 0, False, True)):
        s = C.esize(t)
        vals, locs = C.tie_values(t, world, n, 0xA11 + n), C.tie_indices(world, n, 0xA11 + n)
        heap.fill_(0xC3)
        for off, arr in ((soff, vals[rank]), (lsoff, locs[rank])):
            raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            heap[off:off + raw.size].copy_(torch.from_numpy(raw.copy()).cuda())
        torch.cuda.synchronize()
        before = heap.cpu().numpy()
        PES.pes_barrier(0, 0, world, None)
        tv, tl = (soff, lsoff) if inplace else (toff + shift * s, ltoff + shift * 4)
        osgpu.reduce_loc(t, op)(base + tv, base + tl, base + soff, None if null else base + lsoff,
                                n, 0, 0, world, ctypes.addressof(wrk), psync)
        want_path = "pull" if inplace else "team"
        assert osgpu.last_path() == want_path, (t, op, osgpu.last_path())
        assert not any(ctypes.string_at(psync, 1024)), "pSync not reset"
        torch.cuda.synchronize()
        after = heap.cpu().numpy()
        idx = C.const_indices(list(range(world)), n) if null else locs
        wv, wi = C.expected(t, op, vals, idx)
        bad = C.same_bits(t, after[tv:tv + n * s].view(C.dtype(t)), wv)
        assert bad is None, f"rank {rank} {t} {op} n={n}: value {bad} differs"
        gi = after[tl:tl + n * 4].view(np.int32)
        assert np.array_equal(gi, wi), f"rank {rank} {t} {op} n={n}: an index differs"
        mask = np.ones(after.size, bool)
        mask[tv:tv + n * s] = False
        mask[tl:tl + n * 4] = False
        assert np.array_equal(after[mask], before[mask]), "bytes outside the targets were written"
        PES.pes_barrier(0, 0, world, None)
    del heap
    PES.pes_barrier(0, 0, world, None)
    assert L.osgpu_heap_destroy(ctypes.c_void_p(base)) == 0
    print("LOC_MP_OK", flush=True)


if __name__ == "__main__":
    main()
