"""The prefix scans on the GPU: osgpu_team_scan (team_scan_lds_kernel,
team_scan_scalar_kernel, csrc/team.hip) and osgpu_scan on device and host
heaps.

1. The raw launcher against the reduce-to-all oracle over sub-sets, at the
   smallest shapes that reach each branch.  With W = 16 / element size and
   V = 64 tile vectors (OSGPU_TEAM_LDS_U = 1): lengths 1, W-1, W, W+1, V W-1,
   V W, V W+1, 2 V W + W-1; P in {2, 3, 5, 8} at every length and {4, 6, 7}
   at V W+1; both modes.  Every source and target is allocated EXACTLY n
   elements between guard bands (tests/support/guarded.py): the sources come
   back unchanged, the bands untouched.  All pointers at a common non-zero
   16-byte phase (head / tail edges), one target at another phase (the
   element-granular kernel), a multi-launch case, long double refused.
2. The collective with threads as PEs on device heaps: P in {2, 3, 8},
   nreduce in {1, P-1, 1001, P V W + 3} (empty shards, uneven shards, every
   shard with whole tiles), both modes; the team path, pSync back at 0, every
   byte round every member's target untouched, non-members untouched on a
   strided set.  OSGPU_PATH_PULL, in-place overlap, long double and 9 members
   take the pull form.  PE_size 1.
3. Host heaps: host fold, GETMEM with a 2048-byte chunk, a forced STAGED.
4. Two processes on one GPU through osgpu_heap_create
   (tests/support/scan_mp_worker.py).
5. A seeded fuzz of 30 calls.

Expected values: tests/support/scan_cases.py.
"""
import ctypes
import os

import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import guarded as G
from support import scan_cases as C
from support.gpu_doors import small_launches, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

V = C.TILE_VECTORS
RAW_PAIRS = C.PAIRS + [("float", "max")]    # float max: NaNs and signed zeros (the edge inputs)


def lengths(t):
    W = 16 // C.esize(t)
    return sorted({1, max(W - 1, 1), W, W + 1, V * W - 1, V * W, V * W + 1, 2 * V * W + W - 1})


# ------------------------------------------------------------ 1. raw launcher
class Batch(D.LauncherBatch):
    """Cases of one (type, op).  The expected values of P members are computed
    once at the longest length and sliced."""

    def __init__(self, t, op, nmax, seed):
        super().__init__(t)
        self.op = op
        self.pool = C.inputs(t, op, 8, nmax, seed)
        self.inc = {}       # P -> the inclusive results of P members at nmax

    def add(self, P, n, ex, src_phase, dst_phases, what):
        srcs = [self.arena.add(n * self.s, src_phase, self.pool[p][:n]) for p in range(P)]
        dsts = [self.arena.add(n * self.s, dst_phases[q]) for q in range(P)]
        self.case(srcs, dsts, what, op=self.op, P=P, n=n, exclusive=ex)

    def call(self, c, sp):
        osgpu.team_scan(self.t, self.op, c.exclusive, D.ptrs(c.dsts), D.ptrs(c.srcs), c.n, stream=sp)

    def want(self, c, q):
        if c.P not in self.inc:
            self.inc[c.P] = C.inclusive(self.t, self.op, self.pool[:c.P])
        if c.exclusive and q == 0:
            return np.repeat(C.identity(self.t, self.op), c.n)
        return self.inc[c.P][q - c.exclusive][:c.n]


@pytest.mark.parametrize("t,op", RAW_PAIRS, ids=lambda x: x)
def test_launcher_lengths_and_members(torch_cuda, t, op):
    s = C.esize(t)
    W = 16 // s
    ns = lengths(t)
    b = Batch(t, op, max(ns), 0x5CA7 + s)
    for ex in (0, 1):
        for P in (2, 3, 5, 8):
            for n in ns:
                b.add(P, n, ex, 0, [0] * P, "aligned")
        for P in (4, 6, 7):
            b.add(P, V * W + 1, ex, 0, [0] * P, "aligned")
    b.launch(torch_cuda).check()


@pytest.mark.parametrize("t,op", RAW_PAIRS, ids=lambda x: x)
def test_launcher_phases(torch_cuda, t, op):
    """All pointers at one non-zero 16-byte phase: a scalar head and tail round
    the vectors.  One target at another phase: the element-granular kernel."""
    s = C.esize(t)
    W = 16 // s
    ph = 16 - s if W > 1 else 8       # a head of one element (complexf: phase 8)
    ns = [W - 1 or 1, W + 1, V * W + 1, 2 * V * W + W - 1]
    b = Batch(t, op, max(ns), 0xFA5E + s)
    for ex in (0, 1):
        for P in (2, 3, 8):
            for n in ns:
                b.add(P, n, ex, ph, [ph] * P, f"common phase {ph}")
                other = [ph] * P
                other[P - 1] = (ph + s) % 16
                b.add(P, n, ex, ph, other, f"target {P - 1} at phase {other[P - 1]}")
    b.launch(torch_cuda).check()


@pytest.mark.parametrize("t,op", [("int", "sum"), ("double", "sum"), ("half", "sum")],
                         ids=lambda x: x)
def test_launcher_multi_launch(torch_cuda, small_launches, t, op):
    """3 tiles + 1 vector under a limit of 512 threads a launch (4 tiles a
    launch at 2 members, 2 at 3, 1 at 8): equal to the single launch and to
    the oracle; a common non-zero phase adds the edges to the first launch."""
    s = C.esize(t)
    W = 16 // s
    res = []
    for limit in (0, 512):
        small_launches(limit)
        b = Batch(t, op, (3 * V + 1) * W + W, 0x3717E)
        for ex in (0, 1):
            for P in (2, 3, 8):
                b.add(P, (3 * V + 1) * W, ex, 0, [0] * P, f"limit {limit}")
                b.add(P, (3 * V + 1) * W + W - 1, ex, 16 - s, [16 - s] * P, f"limit {limit} edges")
        b.launch(torch_cuda).check()
        res.append([d.data().copy() for c in b.cases for d in c.dsts])
    for one, many in zip(*res):
        assert np.array_equal(one, many)


def test_launcher_refuses_long_double_and_bad_arguments(torch_cuda):
    a = G.Arena()
    bufs = [a.add(64) for _ in range(4)]
    a.upload(torch_cuda)
    d, s = [g.ptr for g in bufs[:2]], [g.ptr for g in bufs[2:]]
    assert osgpu.team_scan("longdouble", "sum", 0, d, s, 4, check=False) == -5   # OSGPU_ENOTSUP
    assert osgpu.team_scan("complexf", "max", 0, d, s, 4, check=False) == -1     # OSGPU_EINVAL
    assert osgpu.team_scan("int", "sum", 0, d[:1], s[:1], 4, check=False) == -1  # P = 1
    L = osgpu.load()
    assert L.osgpu_team_scan(1, 0, 2, 2, (ctypes.c_void_p * 2)(*d), (ctypes.c_void_p * 2)(*s), 4,
                             None) == -1                                        # exclusive = 2
    torch_cuda.cuda.synchronize()
    a.download()
    for g in bufs:
        g.assert_unchanged("a refused call")


# ---------------------------------------------------- 2. collective, PE threads
SCAN = [D.Door(f"scan exclusive={ex}", lambda tm, t, op, *a, ex=ex: C.run(tm, t, op, ex, *a),
               lambda t, op, src, n, *active, ex=ex: C.expected(t, op, src, ex, *active))
        for ex in (0, 1)]


def _collective(t, op, ex, npes, n, seed, PE_start=0, log=0, PE_size=None, in_place=False, **kw):
    D.collective(SCAN[ex], t, op, npes, n, seed, PE_start, log, PE_size,
                 on_source=0 if in_place else None, **kw)


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, op, P):
    W = 16 // C.esize(t)
    for n in sorted({1, P - 1, 1001, P * V * W + 3}):
        for ex in (0, 1):
            _collective(t, op, ex, P, n, 0xD0 + P)


def test_collective_strided_active_set(torch_cuda):
    for ex in (0, 1):
        _collective("double", "sum", ex, 8, 1001, 5, PE_start=1, log=1, PE_size=3)
        _collective("short", "min", ex, 6, 259, 6, PE_start=0, log=1, PE_size=3)


def test_collective_pull_forms(torch_cuda):
    """OSGPU_PATH_PULL, in-place overlap, long double and 9 members (the team
    form stops at 8) take the pull form."""
    for ex in (0, 1):
        with D.forced_path(osgpu.PATH_PULL):
            _collective("double", "sum", ex, 3, 1001, 21, path="pull")
            _collective("half", "sum", ex, 8, 515, 22, path="pull")
        _collective("float", "prod", ex, 3, 1001, 23, path="pull", in_place=True)
        _collective("int", "sum", ex, 4, 7, 24, path="pull", in_place=True,
                    target_elem_off=3)
        _collective("longdouble", "sum", ex, 3, 257, 25, path="pull")
        _collective("longdouble", "max", ex, 2, 33, 26, path="pull")
        _collective("int", "sum", ex, 9, 1001, 27, path="pull")
        _collective("float", "max", ex, 9, 130, 28, path="pull")


def test_collective_single_member(torch_cuda):
    """PE_size == 1: a copy (inclusive) or the identity (exclusive)."""
    for ex in (0, 1):
        _collective("int", "sum", ex, 1, 1001, 5, path=None)
        _collective("double", "min", ex, 4, 11, 6, PE_start=2, PE_size=1, path=None)
        _collective("longdouble", "prod", ex, 1, 9, 7, path=None)
        _collective("short", "and", ex, 1, 77, 8, path=None, in_place=True)


def test_collective_target_sub_view(torch_cuda):
    """A target an odd number of elements into its array: its phase differs
    from the sources', the team path's element-granular kernel."""
    for t, op in (("short", "min"), ("int", "sum"), ("half", "sum")):
        for ex in (0, 1):
            _collective(t, op, ex, 3, 1001, 0x5B, target_elem_off=3)


# ------------------------------------------------------ 3. host heaps (need a GPU)
@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path; a
    forced STAGED takes GETMEM), the chunk below the array size; a strided
    set, overlap, one member, long double."""
    cases = [("double", "sum", 3, 0, 0, 3, 1001, False), ("short", "min", 2, 0, 0, 2, 5, False),
             ("float", "prod", 8, 1, 1, 3, 700, False), ("int", "sum", 3, 0, 0, 3, 1001, True),
             ("half", "sum", 3, 0, 0, 3, 1501, False), ("longdouble", "sum", 3, 0, 0, 3, 300, False),
             ("longdouble", "max", 1, 0, 0, 1, 9, False), ("complexf", "prod", 2, 0, 0, 2, 333, True)]
    with D.host_heaps(path) as (force, team, ran):
        for t, op, npes, start, log, size, n, ov in cases:
            for ex in (0, 1):
                force()
                _collective(t, op, ex, npes, n, 31 + n, start, log, size, path=ran, in_place=ov,
                            **team)


# ------------------------------------------------------------ 4. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the team
    kernel writes a peer's target through a mapping of another process's
    memory (tests/support/scan_mp_worker.py)."""
    D.run_ranks("scan_mp_worker.py", tmp_path, "SCAN_MP_OK")


# -------------------------------------------------------------------- 5. fuzz
def test_fuzz_30_calls(torch_cuda):
    seed = int(os.environ.get("SCAN_FUZZ_SEED", "20261020"))
    rng = np.random.default_rng(seed)
    pairs = C.PAIRS + [("bfloat16", "max"), ("longlong", "and"), ("float", "min"),
                       ("longdouble", "prod"), ("complexd", "sum"), ("double", "max")]
    for i in range(30):
        t, op = pairs[int(rng.integers(len(pairs)))]
        ex = int(rng.integers(2))
        P = int(rng.integers(1, 9))
        n = int(rng.integers(1, 5001))
        W = 16 // C.esize(t)
        shift = int(rng.integers(0, W)) if W > 1 else 0
        overlap = bool(rng.integers(2))
        team = P >= 2 and not overlap and t != "longdouble"
        what = f"seed {seed} call {i}: {t} {op} ex={ex} P={P} n={n} shift={shift} overlap={overlap}"
        with D.named(what):
            _collective(t, op, ex, P, n, seed + i, target_elem_off=shift,
                        in_place=overlap, path="team" if team else "pull")
