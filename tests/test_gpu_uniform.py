"""The uniform reduce-to-all on the GPU: osgpu_team_uniform
(team_uniform_lds_kernel, team_uniform_scalar_kernel, csrc/team.hip;
ld_uniform_kernel, csrc/longdouble.hip) and osgpu_reduce_uniform on device and
host heaps.

1. The raw launcher against the reduce-to-all oracle's FIRST member, at the
   smallest shapes that reach each branch.  With W = 16 / element size and a
   tile of T = 64 P W elements: lengths 1, W-1, W, W+1, 64 W + 1 (a tile
   where only waves 0 and 1 have fold work), T-1, T, T+1, 2 T + W-1; P in
   {2, 3, 5, 8} at every length and {4, 6, 7} at T+1.  Every source and target
   is allocated EXACTLY n elements between guard bands
   (tests/support/guarded.py): the sources come back unchanged, the bands
   untouched, and all P targets hold the same bytes.  All pointers at a common
   non-zero 16-byte phase (head / tail edges), one target at another phase
   (the element-granular kernel), a multi-launch case, long double (aligned
   and with one pointer at phase 8, padding zero), bad arguments.
2. The collective with threads as PEs on device heaps: P in {2, 3, 8},
   nreduce in {1, P-1, 1001, P T + 3} (empty shards, uneven shards, every
   shard with whole tiles), long double too; the team path, pSync back at 0,
   every byte round every member's target untouched, all targets identical,
   non-members untouched on a strided set.  OSGPU_PATH_PULL, in-place overlap
   and 9 members take the pull form.  PE_size 1.  A target sub-view.
3. Host heaps: host fold, GETMEM with a 2048-byte chunk, a forced STAGED.
4. Two processes on one GPU through osgpu_heap_create
   (tests/support/uniform_mp_worker.py).
5. A seeded fuzz of 30 calls.

Expected values: tests/support/uniform_cases.py.  The inputs of the collective
tests (n = 1001, seed 0xD0 + P) are the ones tests/test_uniform_ref.py shows a
caller-first fold to differ on.
"""
import os

import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import guarded as G
from support import uniform_cases as C
from support.gpu_doors import small_launches, torch_cuda  # noqa: F401  (fixtures)
from test_x87_softfloat import raw_random

pytestmark = pytest.mark.gpu

SUB = C.SUB_VECTORS
RAW_PAIRS = C.PAIRS + [("float", "max")]    # float max: NaNs and signed zeros (the edge inputs)


def lengths(t, P):
    W = 16 // C.esize(t)
    T = C.tile_elems(t, P)
    return sorted({1, max(W - 1, 1), W, W + 1, SUB * W + 1, T - 1, T, T + 1, 2 * T + W - 1})


# ------------------------------------------------------------ 1. raw launcher
class Batch(D.LauncherBatch):
    """Cases of one (type, op).  The expected value of P members is computed
    once at the longest length and sliced."""

    def __init__(self, t, op, nmax, seed, pool=None):
        super().__init__(t)
        self.op = op
        self.pool = C.inputs(t, op, 8, nmax, seed) if pool is None else pool
        self.val = {}       # P -> the uniform value of P members at nmax

    def add(self, P, n, src_phases, dst_phases, what):
        srcs = [self.arena.add(n * self.s, src_phases[p], self.pool[p][:n]) for p in range(P)]
        dsts = [self.arena.add(n * self.s, dst_phases[q]) for q in range(P)]
        self.case(srcs, dsts, what, op=self.op, P=P, n=n)

    def call(self, c, sp):
        osgpu.team_uniform(self.t, self.op, D.ptrs(c.dsts), D.ptrs(c.srcs), c.n, stream=sp)

    def want(self, c, q):
        if c.P not in self.val:
            self.val[c.P] = C.value(self.t, self.op, self.pool[:c.P])
        return self.val[c.P][:c.n]

    check_case = staticmethod(D.targets_identical)


@pytest.mark.parametrize("t,op", RAW_PAIRS, ids=lambda x: x)
def test_launcher_lengths_and_members(torch_cuda, t, op):
    s = C.esize(t)
    b = Batch(t, op, max(lengths(t, 8)), 0x0F17 + s)
    for P in (2, 3, 5, 8):
        for n in lengths(t, P):
            b.add(P, n, [0] * P, [0] * P, "aligned")
    for P in (4, 6, 7):
        b.add(P, C.tile_elems(t, P) + 1, [0] * P, [0] * P, "aligned")
    b.launch(torch_cuda).check()


@pytest.mark.parametrize("t,op", RAW_PAIRS, ids=lambda x: x)
def test_launcher_phases(torch_cuda, t, op):
    """All pointers at one non-zero 16-byte phase: a scalar head and tail round
    the vectors.  One target at another phase: the element-granular kernel."""
    s = C.esize(t)
    W = 16 // s
    ph = 16 - s if W > 1 else 8       # a head of one element (complexf: phase 8)
    b = Batch(t, op, 2 * C.tile_elems(t, 8) + W - 1, 0xFA5E + s)
    for P in (2, 3, 8):
        T = C.tile_elems(t, P)
        for n in (W - 1 or 1, W + 1, SUB * W + 1, T + 1, 2 * T + W - 1):
            b.add(P, n, [ph] * P, [ph] * P, f"common phase {ph}")
            other = [ph] * P
            other[P - 1] = (ph + s) % 16
            b.add(P, n, [ph] * P, other, f"target {P - 1} at phase {other[P - 1]}")
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
        b = Batch(t, op, (3 * SUB * 8 + 1) * W + W, 0x3717E)
        for P in (2, 3, 8):
            n = (3 * SUB * P + 1) * W
            b.add(P, n, [0] * P, [0] * P, f"limit {limit}")
            b.add(P, n + W - 1, [16 - s] * P, [16 - s] * P, f"limit {limit} edges")
        b.launch(torch_cuda).check()
        res.append([d.data().copy() for c in b.cases for d in c.dsts])
    for one, many in zip(*res):
        assert np.array_equal(one, many)


@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
def test_launcher_long_double(torch_cuda, op):
    """ld_uniform_kernel: 16-byte aligned pointers (one dwordx4 per element)
    and one pointer at phase 8 (the byte-pair form).  The inputs hold the edge
    rows (NaNs with payloads, unsupported x87 encodings, signed zeros) and, in
    every other element, random raw encodings (tests/test_gpu_x87.py's)."""
    nmax = 257
    pool = C.inputs("longdouble", op, 8, nmax, 0x87 + len(op))
    for p in range(8):
        pool[p] = np.array(pool[p], copy=True)
        raw = raw_random(nmax, 0x870 + p, "any")
        pool[p][1::2] = raw[1::2]
    b = Batch("longdouble", op, nmax, 0, pool=pool)
    for P in (2, 3, 5, 8):
        for n in (1, 255, 256, 257):
            b.add(P, n, [0] * P, [0] * P, "aligned")
            sp, dp = [0] * P, [0] * P
            sp[P - 1] = 8
            b.add(P, n, sp, dp, f"source {P - 1} at phase 8")
            sp, dp = [0] * P, [0] * P
            dp[0] = 8
            b.add(P, n, sp, dp, "target 0 at phase 8")
    b.launch(torch_cuda).check()


def test_launcher_bad_arguments(torch_cuda):
    a = G.Arena()
    bufs = [a.add(64) for _ in range(18)]
    a.upload(torch_cuda)
    d, s = [g.ptr for g in bufs[:9]], [g.ptr for g in bufs[9:]]
    assert osgpu.team_uniform("complexf", "max", d[:2], s[:2], 4, check=False) == -1   # OSGPU_EINVAL
    assert osgpu.team_uniform("longdouble", "xor", d[:2], s[:2], 4, check=False) == -1
    assert osgpu.team_uniform("int", "sum", d[:1], s[:1], 4, check=False) == -1        # P = 1
    assert osgpu.team_uniform("int", "sum", d, s, 4, check=False) == -1                # P = 9
    assert osgpu.team_uniform("longdouble", "sum", d, s, 4, check=False) == -1
    torch_cuda.cuda.synchronize()
    a.download()
    for g in bufs:
        g.assert_unchanged("a refused call")


# ---------------------------------------------------- 2. collective, PE threads
UNIFORM = D.Door("uniform", C.run, lambda t, op, src, n, *active: C.expected(t, op, src, *active),
                 extra=D.same_bytes_as_first)


def _collective(t, op, npes, n, seed, PE_start=0, log=0, PE_size=None, in_place=False, **kw):
    D.collective(UNIFORM, t, op, npes, n, seed, PE_start, log, PE_size,
                 on_source=0 if in_place else None, **kw)


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS + [("longdouble", "sum")], ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, op, P):
    for n in sorted({1, P - 1, 1001, P * C.tile_elems(t, P) + 3}):
        _collective(t, op, P, n, 0xD0 + P)


def test_collective_discriminating_pairs(torch_cuda):
    """float max, the one pair of tests/test_uniform_ref.py's discrimination
    condition outside PAIRS, on the same inputs."""
    for P in (3, 8):
        _collective("float", "max", P, 1001, 0xD0 + P)


def test_collective_strided_active_set(torch_cuda):
    _collective("double", "sum", 8, 1001, 5, PE_start=1, log=1, PE_size=3)
    _collective("short", "min", 6, 259, 6, PE_start=0, log=1, PE_size=3)
    _collective("longdouble", "prod", 5, 77, 7, PE_start=0, log=2, PE_size=2)


def test_collective_pull_forms(torch_cuda):
    """OSGPU_PATH_PULL, in-place overlap and 9 members (the team form stops
    at 8) take the pull form."""
    with D.forced_path(osgpu.PATH_PULL):
        _collective("double", "sum", 3, 1001, 0xD0 + 3, path="pull")
        _collective("half", "sum", 8, 1001, 0xD0 + 8, path="pull")
        _collective("longdouble", "sum", 3, 257, 25, path="pull")
    _collective("float", "prod", 3, 1001, 0xD0 + 3, path="pull", in_place=True)
    _collective("int", "sum", 4, 7, 24, path="pull", in_place=True, target_elem_off=3)
    _collective("longdouble", "max", 2, 33, 26, path="pull", in_place=True)
    _collective("int", "sum", 9, 1001, 27, path="pull")
    _collective("float", "max", 9, 130, 28, path="pull")
    _collective("double", "sum", 9, 1001, 29, path="pull")


def test_collective_single_member(torch_cuda):
    """PE_size == 1: a copy of the source."""
    _collective("int", "sum", 1, 1001, 5, path=None)
    _collective("double", "min", 4, 11, 6, PE_start=2, PE_size=1, path=None)
    _collective("longdouble", "prod", 1, 9, 7, path=None)
    _collective("short", "and", 1, 77, 8, path=None, in_place=True)


def test_collective_target_sub_view(torch_cuda):
    """A target an odd number of elements into its array: its phase differs
    from the sources', the team path's element-granular kernel."""
    for t, op in (("short", "min"), ("int", "sum"), ("half", "sum"), ("float", "prod")):
        _collective(t, op, 3, 1001, 0xD0 + 3, target_elem_off=3)


# ------------------------------------------------------ 3. host heaps (need a GPU)
@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path; a
    forced STAGED takes GETMEM), the chunk below the array size; a strided
    set, overlap, one member, long double."""
    cases = [("double", "sum", 3, 0, 0, 3, 1001, False), ("short", "min", 2, 0, 0, 2, 5, False),
             ("float", "prod", 8, 1, 1, 3, 700, False), ("int", "sum", 3, 0, 0, 3, 1001, True),
             ("half", "sum", 3, 0, 0, 3, 1501, False), ("longdouble", "sum", 3, 0, 0, 3, 300, False),
             ("longdouble", "max", 1, 0, 0, 1, 9, False), ("complexf", "prod", 2, 0, 0, 2, 333, True),
             ("float", "max", 8, 0, 0, 8, 1001, False)]
    with D.host_heaps(path) as (force, team, ran):
        for t, op, npes, start, log, size, n, ov in cases:
            force()
            _collective(t, op, npes, n, 0xD0 + size, start, log, size, path=ran, in_place=ov, **team)


# ------------------------------------------------------------ 4. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the uniform
    kernel writes a peer's target through a mapping of another process's
    memory (tests/support/uniform_mp_worker.py)."""
    D.run_ranks("uniform_mp_worker.py", tmp_path, "UNIFORM_MP_OK")


# -------------------------------------------------------------------- 5. fuzz
def test_fuzz_30_calls(torch_cuda):
    seed = int(os.environ.get("UNIFORM_FUZZ_SEED", "20261021"))
    rng = np.random.default_rng(seed)
    pairs = C.PAIRS + [("bfloat16", "max"), ("longlong", "and"), ("float", "min"),
                       ("longdouble", "prod"), ("longdouble", "sum"), ("complexd", "sum"),
                       ("double", "max")]
    for i in range(30):
        t, op = pairs[int(rng.integers(len(pairs)))]
        P = int(rng.integers(1, 9))
        n = int(rng.integers(1, 5001))
        W = 16 // C.esize(t)
        shift = int(rng.integers(0, W)) if W > 1 else 0
        overlap = bool(rng.integers(2))
        team = P >= 2 and not overlap
        what = f"seed {seed} call {i}: {t} {op} P={P} n={n} shift={shift} overlap={overlap}"
        with D.named(what):
            _collective(t, op, P, n, seed + i, target_elem_off=shift,
                        in_place=overlap, path="team" if team else "pull")
