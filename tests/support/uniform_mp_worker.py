"""uniform_mp_worker.py -- TEST INFRASTRUCTURE: one rank (= one PE = one
process) of a multi-process osgpu_reduce_uniform run on one GPU
(tests/support/door_mp.py).  The device heaps come from osgpu_heap_create, so
the uniform kernel reads a peer's source and writes a peer's target through a
mapping of another process's memory.  Prints UNIFORM_MP_OK when every case
matched.
usage: python uniform_mp_worker.py OUTDIR
"""
from door_mp import Rank, torch  # first: it sets the import path

import osgpu
from support import uniform_cases as C

TOFF = 4 << 20
# (type, op, n, target shift in elements, in place) -> the path
CASES = (("double", "sum", 1001, 0, False), ("short", "min", 2051, 3, False),
         ("half", "sum", 777, 0, False), ("complexf", "prod", 515, 0, False),
         ("longdouble", "sum", 65, 0, False), ("int", "sum", 300, 0, True))


def main():
    R = Rank("un")
    for t, op, n, shift, inplace in CASES:
        what = f"{t} {op} n={n}"
        src = C.inputs(t, op, R.world, n, 0xA11 + n)
        before = R.load([(0, src[R.rank])])
        tgt = 0 if inplace else TOFF + shift * C.esize(t)
        osgpu.reduce_uniform(t, op)(R.base + tgt, R.base, n, 0, 0, R.world, R.wrk, R.psync)
        after = R.called("pull" if inplace else "team", what)
        got = R.check(after, before, [(tgt, t, C.expected(t, op, src)[R.rank])], what)
        # every rank holds the same bytes: compare them through gloo
        mine = torch.from_numpy(got.copy())
        both = [torch.empty_like(mine) for _ in range(R.world)]
        R.dist.all_gather(both, mine)
        assert all(torch.equal(b, both[0]) for b in both), f"{what}: the ranks' targets differ"
        R.barrier()
    R.close("UNIFORM_MP_OK")


if __name__ == "__main__":
    main()
