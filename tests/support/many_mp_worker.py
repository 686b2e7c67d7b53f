"""many_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one
process) of a multi-process osgpu_reduce_many run on one GPU, started the way
tests/support/rscatter_mp_worker.py is (RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT; torch.distributed gloo for the setup, the shared-memory PE
runtime tests/support/pe_shm.c for the PE services).  The device heaps come
from osgpu_heap_create, so every peer source is read through a mapping of
another process's memory.  Prints MANY_MP_OK when every case matched.
usage: python many_mp_worker.py OUTDIR
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
from support import many_cases as M  # noqa: E402
from support import peshm  # noqa: E402
from support import rscatter_cases as C  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    L = osgpu.load()
    PES = peshm.init(rank, world, 1 << 24, dist, tag="many")
    assert L.osgpu_set_pe_ops(PES.pes_ops()) == 0
    PES.pes_barrier.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    torch.cuda.set_device(0)
    hsync = PES.pes_heap(rank) + PES.pes_heap_bytes() - 8192
    psync = PES.pes_heap(rank) + PES.pes_heap_bytes() - 4096
    base = osgpu.heap_create(8 << 20, 0, 0, world, hsync)
    heap = osgpu.device_view(base, 8 << 20)
    wrk = (ctypes.c_byte * 4096)()
    for t, op in (("double", "sum"), ("bfloat16", "prod")):
        W = 16 // C.esize(t)
        lens = [1001, 0, 1, M.TILE_VECTORS * W + 3] * 4 + [7]   # 17 entries
        lay = M.Layout(t, lens, inplace=(4,), odd={7: 3})
        assert lay.bytes <= 8 << 20
        src = M.sources(t, op, world, lens, 0xA11)
        image = np.full(8 << 20, 0xC3, dtype=np.uint8)
        for i, n in enumerate(lens):
            raw = np.ascontiguousarray(src[i][rank]).view(np.uint8).reshape(-1)
            image[lay.soff[i]:lay.soff[i] + raw.size] = raw
        heap.copy_(torch.from_numpy(image).cuda())
        torch.cuda.synchronize()
        PES.pes_barrier(0, 0, world, None)
        osgpu.reduce_many(t, op)([base + o for o in lay.toff], [base + o for o in lay.soff], lens,
                                 0, 0, world, ctypes.addressof(wrk), psync)
        assert osgpu.last_path() == "pull", osgpu.last_path()
        assert not any(ctypes.string_at(psync, 1024)), "pSync not reset"
        torch.cuda.synchronize()
        after = heap.cpu().numpy()
        want = M.expected(t, op, src)
        for i, n in enumerate(lens):
            if n == 0:
                continue
            got = after[lay.toff[i]:lay.toff[i] + n * lay.s].view(C.dtype(t))
            bad = C.same_bits(t, got, want[i][rank])
            assert bad is None, f"rank {rank} {t} {op} entry {i} n={n}: element {bad} differs"
        mask = np.zeros(8 << 20, dtype=bool)
        mask[:lay.bytes] = lay.target_mask()
        assert np.array_equal(after[~mask], image[~mask]), "bytes outside the targets were written"
        PES.pes_barrier(0, 0, world, None)
    del heap
    PES.pes_barrier(0, 0, world, None)
    assert L.osgpu_heap_destroy(ctypes.c_void_p(base)) == 0
    print("MANY_MP_OK", flush=True)


if __name__ == "__main__":
    main()
