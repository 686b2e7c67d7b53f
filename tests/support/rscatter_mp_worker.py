"""rscatter_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one
process) of a multi-process osgpu_reduce_scatter run on one GPU
(tests/support/door_mp.py).  The device heaps come from osgpu_heap_create, so
every peer source is read through a mapping of another process's memory.
Prints RSCATTER_MP_OK when every case matched.
usage: python rscatter_mp_worker.py OUTDIR
"""
from door_mp import Rank  # first: it sets the import path

import osgpu
from support import rscatter_cases as C

TOFF = 4 << 20
# (type, op, n, target shift in elements)
CASES = (("double", "sum", 1001, 1), ("short", "min", 2051, 3), ("half", "sum", 777, 0),
         ("complexf", "prod", 515, 1))


def main():
    R = Rank("rs")
    for t, op, n, shift in CASES:
        what = f"{t} {op} n={n}"
        src = C.inputs(t, op, R.world, R.world * n, 0xA11 + n)
        before = R.load([(0, src[R.rank])])
        tgt = TOFF + shift * C.esize(t)
        osgpu.reduce_scatter(t, op)(R.base + tgt, R.base, n, 0, 0, R.world, R.wrk, R.psync)
        after = R.called("pull", what)
        R.check(after, before, [(tgt, t, C.expected(t, op, src, n)[R.rank])], what)
        R.barrier()
    R.close("RSCATTER_MP_OK")


if __name__ == "__main__":
    main()
