"""many_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one
process) of a multi-process osgpu_reduce_many run on one GPU
(tests/support/door_mp.py).  The device heaps come from osgpu_heap_create, so
every peer source is read through a mapping of another process's memory.
Prints MANY_MP_OK when every case matched.
usage: python many_mp_worker.py OUTDIR
"""
from door_mp import HEAP, Rank  # first: it sets the import path

import osgpu
from support import many_cases as M
from support import rscatter_cases as C

CASES = (("double", "sum"), ("bfloat16", "prod"))


def main():
    R = Rank("many")
    for t, op in CASES:
        what = f"{t} {op}"
        W = 16 // C.esize(t)
        lens = [1001, 0, 1, M.TILE_VECTORS * W + 3] * 4 + [7]   # 17 entries
        lay = M.Layout(t, lens, inplace=(4,), odd={7: 3})
        assert lay.bytes <= HEAP
        src = M.sources(t, op, R.world, lens, 0xA11)
        before = R.load([(lay.soff[i], src[i][R.rank]) for i in range(len(lens))])
        osgpu.reduce_many(t, op)([R.base + o for o in lay.toff], [R.base + o for o in lay.soff], lens,
                                 0, 0, R.world, R.wrk, R.psync)
        after = R.called("pull", what)
        want = M.expected(t, op, src)
        R.check(after, before, [(lay.toff[i], t, want[i][R.rank]) for i, n in enumerate(lens) if n],
                what)
        R.barrier()
    R.close("MANY_MP_OK")


if __name__ == "__main__":
    main()
