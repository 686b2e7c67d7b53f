"""wsum_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one process)
of a multi-process osgpu_reduce_wsum run on one GPU (tests/support/door_mp.py).
The device heaps come from osgpu_heap_create, so the kernel reads a peer's
source and writes a peer's target through a mapping of another process's
memory.  Prints WSUM_MP_OK when every case matched.
usage: python wsum_mp_worker.py OUTDIR
"""
from door_mp import Rank  # first: it sets the import path

import osgpu
from support import wsum_cases as C
from support import wsum_ref as W

SOFF, TOFF = 0, 2 << 20
# (type, out_type, n, target shift in elements, in place) -> the path
CASES = (("bfloat16", "bfloat16", 4101, 0, False), ("half", "float", 6161, 0, False),
         ("half", "half", 777, 3, False), ("bfloat16", "float", 515, 4, False),
         ("bfloat16", "float", 300, 0, True), ("half", "half", 300, 0, True))


def main():
    R = Rank("ws")
    for t, out_t, n, shift, inplace in CASES:
        what = f"{t} -> {out_t} n={n}"
        srcs = C.mixed_inputs(t, R.world, n, 0xA11 + n)
        before = R.load([(SOFF, srcs[R.rank])])
        tv = SOFF if inplace else TOFF + shift * C.out_size(out_t)
        osgpu.reduce_wsum(t, out_t)(R.base + tv, R.base + SOFF, n, 0, 0, R.world, R.wrk, R.psync)
        after = R.called("pull" if inplace else "team", what)
        R.check(after, before, [(tv, "float" if out_t == "float" else t, W.wsum(t, out_t, srcs))],
                what)
        R.barrier()
    R.close("WSUM_MP_OK")


if __name__ == "__main__":
    main()
