"""scan_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one process)
of a multi-process osgpu_scan run on one GPU (tests/support/door_mp.py).  The
device heaps come from osgpu_heap_create, so the team kernel reads a peer's
source and writes a peer's target through a mapping of another process's
memory.  Prints SCAN_MP_OK when every case matched.
usage: python scan_mp_worker.py OUTDIR
"""
from door_mp import Rank  # first: it sets the import path

import osgpu
from support import scan_cases as C

TOFF = 4 << 20
# (type, op, n, target shift in elements, in place) -> the path
CASES = (("double", "sum", 1001, 0, False), ("short", "min", 2051, 3, False),
         ("half", "sum", 777, 0, False), ("complexf", "prod", 515, 0, False),
         ("longdouble", "sum", 65, 0, False), ("int", "sum", 300, 0, True))


def main():
    R = Rank("sc")
    for t, op, n, shift, inplace in CASES:
        src = C.inputs(t, op, R.world, n, 0xA11 + n)
        for ex in (0, 1):
            what = f"{t} {op} ex={ex} n={n}"
            before = R.load([(0, src[R.rank])])
            tgt = 0 if inplace else TOFF + shift * C.esize(t)
            osgpu.scan(t, op, ex)(R.base + tgt, R.base, n, 0, 0, R.world, R.wrk, R.psync)
            after = R.called("pull" if inplace or t == "longdouble" else "team", what)
            R.check(after, before, [(tgt, t, C.expected(t, op, src, ex)[R.rank])], what)
            R.barrier()
    R.close("SCAN_MP_OK")


if __name__ == "__main__":
    main()
