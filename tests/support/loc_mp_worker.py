"""loc_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one process)
of a multi-process osgpu_reduce_loc run on one GPU (tests/support/door_mp.py).
The device heaps come from osgpu_heap_create, so the kernel reads a peer's two
sources and writes a peer's two targets through a mapping of another process's
memory.  Prints LOC_MP_OK when every case matched.
usage: python loc_mp_worker.py OUTDIR
"""
from door_mp import Rank  # first: it sets the import path

import osgpu
from support import loc_cases as C

SOFF, LSOFF, TOFF, LTOFF = 0, 1 << 20, 2 << 20, 3 << 20
# (type, op, n, target shift in elements, no index source, in place) -> the path
CASES = (("double", "max", 4101, 0, False, False), ("short", "min", 6161, 3, False, False),
         ("half", "max", 777, 0, True, False), ("float", "min", 515, 0, True, False),
         ("int", "max", 300, 0, False, True))


def main():
    R = Rank("lc")
    for t, op, n, shift, null, inplace in CASES:
        what = f"{t} {op} n={n}"
        vals, locs = C.tie_values(t, R.world, n, 0xA11 + n), C.tie_indices(R.world, n, 0xA11 + n)
        before = R.load([(SOFF, vals[R.rank]), (LSOFF, locs[R.rank])])
        tv, tl = (SOFF, LSOFF) if inplace else (TOFF + shift * C.esize(t), LTOFF + shift * 4)
        osgpu.reduce_loc(t, op)(R.base + tv, R.base + tl, R.base + SOFF,
                                None if null else R.base + LSOFF, n, 0, 0, R.world, R.wrk, R.psync)
        after = R.called("pull" if inplace else "team", what)
        idx = C.const_indices(list(range(R.world)), n) if null else locs
        wv, wi = C.expected(t, op, vals, idx)
        R.check(after, before, [(tv, t, wv), (tl, "int", wi)], what)
        R.barrier()
    R.close("LOC_MP_OK")


if __name__ == "__main__":
    main()
