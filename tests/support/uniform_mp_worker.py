"""uniform_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one
process) of a multi-process osgpu_reduce_uniform run on one GPU, started the
way tests/support/scan_mp_worker.py is (RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT; torch.distributed gloo for the setup, the shared-memory PE runtime
tests/support/pe_shm.c for the PE services).  The device heaps come from
osgpu_heap_create, so the uniform kernel reads a peer's source and writes a
peer's target through a mapping of another process's memory.  Prints
UNIFORM_MP_OK when every case matched.
usage: python uniform_mp_worker.py OUTDIR
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
from support import peshm  # noqa: E402
from support import uniform_cases as C  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    L = osgpu.load()
    PES = peshm.init(rank, world, 1 << 24, dist, tag="un")
    assert L.osgpu_set_pe_ops(PES.pes_ops()) == 0
    PES.pes_barrier.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    torch.cuda.set_device(0)
    hsync = PES.pes_heap(rank) + PES.pes_heap_bytes() - 8192
    psync = PES.pes_heap(rank) + PES.pes_heap_bytes() - 4096
    base = osgpu.heap_create(8 << 20, 0, 0, world, hsync)
    heap = osgpu.device_view(base, 8 << 20)
    wrk = (ctypes.c_byte * 4096)()
    toff = 4 << 20
    # (type, op, n, target shift in elements, in place) -> the path
    for t, op, n, shift, inplace in (("double", "sum", 1001, 0, False), ("short", "min", 2051, 3, False),
                                     ("half", "sum", 777, 0, False), ("complexf", "prod", 515, 0, False),
                                     ("longdouble", "sum", 65, 0, False), ("int", "sum", 300, 0, True)):
        s = C.esize(t)
        src = C.inputs(t, op, world, n, 0xA11 + n)
        raw = np.ascontiguousarray(src[rank]).view(np.uint8).reshape(-1)
        heap.fill_(0xC3)
        heap[:raw.size].copy_(torch.from_numpy(raw.copy()).cuda())
        torch.cuda.synchronize()
        PES.pes_barrier(0, 0, world, None)
        tgt = 0 if inplace else toff + shift * s
        osgpu.reduce_uniform(t, op)(base + tgt, base, n, 0, 0, world, ctypes.addressof(wrk), psync)
        want_path = "pull" if inplace else "team"
        assert osgpu.last_path() == want_path, (t, op, osgpu.last_path())
        assert not any(ctypes.string_at(psync, 1024)), "pSync not reset"
        torch.cuda.synchronize()
        after = heap.cpu().numpy()
        want = C.expected(t, op, src)[rank]
        got = after[tgt:tgt + n * s]
        bad = C.same_bits(t, got.view(C.dtype(t)), want)
        assert bad is None, f"rank {rank} {t} {op} n={n}: element {bad} differs"
        if t == "longdouble":
            assert not got.reshape(-1, 16)[:, 10:].any(), "long double padding not zero"
        if not inplace:
            assert np.array_equal(after[:raw.size], raw), "the source changed"
            assert (after[raw.size:tgt] == 0xC3).all(), "bytes before the target were written"
        assert (after[tgt + n * s:] == 0xC3).all(), "bytes after the target were written"
        # every rank holds the same bytes: compare digests through gloo
        mine = torch.from_numpy(np.frombuffer(got.tobytes(), np.uint8).copy())
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        assert all(torch.equal(b, both[0]) for b in both), f"{t} {op}: the ranks' targets differ"
        PES.pes_barrier(0, 0, world, None)
    del heap
    PES.pes_barrier(0, 0, world, None)
    assert L.osgpu_heap_destroy(ctypes.c_void_p(base)) == 0
    print("UNIFORM_MP_OK", flush=True)


if __name__ == "__main__":
    main()
