"""The batched reduce-to-all on the GPU: osgpu_combine_many
(combine_many_kernel, csrc/combine.hip) and osgpu_reduce_many.

1. The raw launcher for every (type, op) of the library against the
   reduce-to-all oracle's left-to-right fold, one arena upload each.  With
   W = 16 / element size and V = 128 vectors a tile (OSGPU_MANY_U = 2), every
   entry has one of the lengths 1, W-1, W, W+1, V W-1, V W, V W+1,
   2 V W + W-1 (or 0); batches of 1, 2, 15, 16, 17 and 33 entries at K = 2, 3
   and 8 inputs; entries sit at different 16-byte phases from each other,
   every pointer of one entry at the same.  One batch mixes in the phase
   fall-backs (a target one element off its sources' phase, a pointer off its
   element alignment), one runs at K = 1 and one at K = 9 (one nsrc per
   call).  Long double and complexd get batches of their own.  Every target
   sits between guard bands (tests/support/guarded.py), every source must
   come back bitwise unchanged, long double padding is zero.  The inputs of
   one phase are shared by the entries at that phase (sources may share), so
   what the bands cannot show here is a read past an input's end.
2. test_routes: from the launcher's own counters (osgpu_test_many_routes)
   which kernel every entry took -- all routes give the same bits.
3. The collective with threads as PEs on device heaps: P in {2, 3, 8},
   count in {1, 3, 17}, lengths from {0, 1, 1001, V W + 3}, one entry in
   place, one target at an odd element offset, a strided active set; int sum,
   double sum, float max, bfloat16 prod, long double sum.  Every target equals
   the oracle's reduce-to-all of its entry; the same inputs through `count`
   single calls give identical bytes; the pull path; pSync all zero; no byte
   outside the targets written; and exactly TWO barriers per member, counted
   by a PE-ops table of the test's own (tests/support/bar_count.c).
4. Host heaps: the host fold and GETMEM, count = 3, P in {2, 3}.
5. Two processes on one GPU through osgpu_heap_create
   (tests/support/many_mp_worker.py).
6. The fatal contract: overlapping targets of two entries, count = -1.
7. A seeded fuzz of 30 calls.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import guarded as G
from support import many_cases as M
from support import rscatter_cases as C
from support.gpu_doors import small_launches, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = M.TILE_VECTORS
ALL_PAIRS = ([(t, o) for t in osgpu.TYPES for o in osgpu.OPS if osgpu.has_op(t, o)]
             + [(t, o) for t in osgpu.EXT_TYPES for o in osgpu.EXT_OPS])
assert len(ALL_PAIRS) == 52


def lengths(t):
    W = 16 // C.esize(t)
    return [1, max(W - 1, 1), W, W + 1, V * W - 1, V * W, V * W + 1, 2 * V * W + W - 1]


# ------------------------------------------------------------ 1. raw launcher
class Tables(D.LauncherBatch):
    """Calls of osgpu_combine_many for one (type, op): a case is one call, its
    targets the entries'.  Inputs: kmax arrays of nmax elements, one copy of
    each per 16-byte phase in use, shared by every call (so a case lists no
    sources of its own: check() looks at the shared ones once)."""

    def __init__(self, t, op, kmax, nmax, seed):
        super().__init__(t)
        self.op, self.nmax = op, nmax
        self.pool = C.inputs(t, op, kmax, nmax, seed)
        self.fold = {}      # K -> fold of pool[:K] at nmax
        self.src = {}       # (phase, k) -> Guarded

    def source(self, phase, k):
        if (phase, k) not in self.src:
            self.src[(phase, k)] = self.arena.add(self.nmax * self.s, phase, self.pool[k])
        return self.src[(phase, k)]

    def call_of(self, K, entries, what):
        """entries: (n, target phase, [source phases]) each."""
        rows = [(n, self.arena.add(n * self.s, tp), [self.source(sps[k], k) for k in range(K)])
                for n, tp, sps in entries]
        self.case([], [r[1] for r in rows], what, op=self.op, K=K, lens=[r[0] for r in rows],
                  ins=[r[2] for r in rows])

    def call(self, c, sp):
        osgpu.combine_many(self.t, self.op, D.ptrs(c.dsts), [D.ptrs(g) for g in c.ins], c.lens,
                           stream=sp)

    def want(self, c, q):
        if not c.lens[q]:
            return self.pool[0][:0]
        if c.K not in self.fold:
            self.fold[c.K] = C.fold_left(self.t, self.op, self.pool[:c.K])
        return self.fold[c.K][:c.lens[q]]

    def describe(self, c):
        return f"{self.t} {self.op} K={c.K} {c.what}, {len(c.lens)} entries of n={c.lens}"

    def check(self):
        super().check()
        for (phase, k), g in self.src.items():
            g.assert_unchanged(f"{self.t} {self.op} input {k} at phase {phase}")
        return self


def _mixed(t, count, K, salt=0):
    """count entries: lengths cycling through lengths(t), every fifth empty
    from 15 entries on, phases cycling through the element's own."""
    s = C.esize(t)
    W = 16 // s
    ns = lengths(t)
    out = []
    for i in range(count):
        n = 0 if count >= 15 and i % 5 == 2 else ns[(i + salt) % len(ns)]
        ph = ((i + salt) % W) * s if W > 1 else 0
        out.append((n, ph, [ph] * K))
    return out


@pytest.mark.parametrize("t,op", [p for p in ALL_PAIRS if p[0] != "longdouble"], ids=lambda x: x)
def test_launcher_batches(torch_cuda, t, op):
    s = C.esize(t)
    W = 16 // s
    b = Tables(t, op, 9, max(lengths(t)), 0x3A47 + s)
    for K in (2, 3, 8):
        for count in (1, 2, 15, 16, 17, 33):
            b.call_of(K, _mixed(t, count, K, salt=K + count), f"batch of {count}")
    # the fall-backs among batch entries
    n = V * W + 1
    off = s if W > 1 else 8         # a target one element off its sources' phase (complexd: 8 bytes)
    fb = [(n, 0, [0] * 3), (n, off, [0] * 3), (W + 1, 0, [0] * 3)]
    if s > 1 and t != "complexd":   # a pointer off its element alignment
        fb += [(n, 0, [0, s // 2, 0]), (W + 1, s // 2, [0] * 3)]
    b.call_of(3, fb + [(max(lengths(t)), 0, [0] * 3)], "phase fall-backs")
    b.call_of(1, _mixed(t, 3, 1), "one input")
    b.call_of(9, _mixed(t, 3, 9) + [(n, off, [0] * 9)], "nine inputs")
    b.launch(torch_cuda).check()


@pytest.mark.parametrize("t,op,phase", [("longdouble", "sum", 0), ("longdouble", "max", 0),
                                        ("complexd", "prod", 0), ("complexd", "sum", 8)],
                         ids=["longdouble_sum", "longdouble_max", "complexd", "complexd_8_off"])
def test_launcher_16_byte_elements(torch_cuda, t, op, phase):
    b = Tables(t, op, 9, 2 * V + 1, 0x16B)
    for K in (1, 2, 3, 9):
        b.call_of(K, [(n, phase, [0] * K) for n in (1, V, 0, 2 * V + 1, V + 1)], f"target phase {phase}")
    b.call_of(2, [((i * 37) % (2 * V) + 1, phase, [0, 0]) for i in range(17)], "17 entries")
    b.launch(torch_cuda).check()


# ------------------------------------------------------------------ 2. routes
def _routes():
    """osgpu_test_many_routes: [segments on the batch kernel, entries on the
    shifted combine, on the long double kernel, on the chunks of 8, on the
    one-input copy, launches of the batch kernel, continuations]."""
    c = (ctypes.c_ulonglong * 7)()
    L = osgpu.load()
    L.osgpu_test_many_routes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong * 7)]
    assert L.osgpu_test_many_routes(ctypes.byref(c)) == 0, L.osgpu_last_error()
    return np.array(list(c), dtype=np.int64)


def test_routes(torch_cuda, small_launches):
    t, op, s, W = "float", "prod", 4, 4

    def delta(K, entries, t=t, op=op):
        b = Tables(t, op, K, max(e[0] for e in entries), 0xA0)
        b.call_of(K, entries, "route")
        before = _routes()
        b.launch(torch_cuda).check()
        return list(_routes() - before), [g.data().copy() for g in b.cases[0].dsts]

    small_launches(0)
    n = V * W + 1
    same = [(n + i, (i % W) * s, [(i % W) * s] * 2) for i in range(17)]
    assert delta(2, same)[0] == [17, 0, 0, 0, 0, 2, 0], "17 entries: 16 segments and 1"
    assert delta(2, same[:16])[0] == [16, 0, 0, 0, 0, 1, 0]
    assert delta(2, [(0, 0, [0, 0])] * 3)[0] == [0] * 7, "empty entries: no launch"
    mixed = [(n, 0, [0] * 3), (n, s, [0] * 3), (n, 0, [0, 2, 0])]
    assert delta(3, mixed)[0] == [1, 2, 0, 0, 0, 1, 0], "off-phase target, misaligned source"
    assert delta(1, [(n, s, [0]), (3, 0, [0])])[0] == [0, 0, 0, 0, 2, 0, 0], "one input: copies"
    assert delta(9, [(n, 0, [0] * 9), (n, s, [s] * 9)])[0] == [0, 0, 0, 2, 0, 0, 0], "chunks of 8"
    assert delta(9, [(n, s, [0] * 9)])[0] == [0, 1, 0, 0, 0, 0, 0], "nine inputs off phase"
    assert delta(2, [(V + 1, 0, [0, 0])] * 2, "longdouble", "sum")[0] == [0, 0, 2, 0, 0, 0, 0]
    assert delta(2, [(V + 1, 8, [0, 0])], "complexd", "prod")[0] == [0, 1, 0, 0, 0, 0, 0]
    # an entry of 5 tiles where one launch holds 3 (K = 2: 128 threads a tile)
    five = [(5 * V * W, 0, [0, 0])]
    one, bits_one = delta(2, five)
    assert one == [1, 0, 0, 0, 0, 1, 0]
    small_launches(3 * 128)
    try:
        split, bits_split = delta(2, five)
        assert split == [2, 0, 0, 0, 0, 2, 1], "tiles [0, 3) and the continuation [3, 5)"
        assert np.array_equal(bits_one[0], bits_split[0])
        # with edges, among other entries: 1 + 5 + 1 tiles, three to a launch
        edgy = [(7, s, [s, s]), (5 * V * W - 2, 2 * s, [2 * s] * 2), (9, 0, [0, 0])]
        assert delta(2, edgy)[0] == [4, 0, 0, 0, 0, 3, 1]
    finally:
        small_launches(0)


# ---------------------------------------------------- 3. collective, PE threads
def _collective(t, op, npes, lens, seed, PE_start=0, log=0, PE_size=None, inplace=(),
                odd=None, sodd=None, device=True, host_fold=False, path="pull", setup=None):
    """One osgpu_reduce_many on a fresh team, checked against the oracle
    entry by entry, then against the same table as single calls."""
    from support import team as T
    PE_size = npes if PE_size is None else PE_size
    lay = M.Layout(t, lens, inplace, odd, sodd)
    tm = T.Team(npes, lay.bytes, device=device, host_fold=host_fold)
    if setup:
        setup()
    src = M.sources(t, op, npes, lens, seed)
    for pe in range(npes):
        tm.fill(pe, 0, lay.bytes, 0xC3)
        for i in range(len(lens)):
            tm.write(pe, lay.soff[i], src[i][pe])
    before = {pe: tm.read(pe, 0, lay.bytes) for pe in range(npes)}
    with M.counted_barriers(tm) as calls:
        members = M.run_many(tm, t, op, lay, PE_start, log, PE_size)
        nbar = {pe: calls(pe) for pe in members}
    paths = dict(tm.last_paths)
    want = M.expected(t, op, src, PE_start, log, PE_size)
    mask = lay.target_mask()
    after = {pe: tm.read(pe, 0, lay.bytes) for pe in range(npes)}
    what = f"{t} {op} P={PE_size} lens={list(lens)}"
    if not any(n > 0 for n in lens):
        path = "barrier_only"
    for pe in range(npes):
        if pe not in members:
            assert np.array_equal(after[pe], before[pe]), f"{what}: PE {pe} is not a member"
            continue
        for i, n in enumerate(lens):
            if n <= 0:
                continue
            got = after[pe][lay.toff[i]:lay.toff[i] + n * lay.s].view(C.dtype(t))
            bad = C.same_bits(t, got, want[i][pe])
            assert bad is None, f"{what} PE {pe} entry {i}: element {bad} differs from the oracle"
        d = G.first_diff(after[pe][~mask], before[pe][~mask])
        assert d is None, f"{what} PE {pe}: a byte outside the targets was written"
        assert nbar[pe] == 2, f"{what} PE {pe}: {nbar[pe]} barriers"
        assert paths[pe] == path, paths
    # the same table as single reduce-to-all calls: identical bytes
    for pe in range(npes):
        tm.write(pe, 0, before[pe])
    M.run_singles(tm, t, op, lay, PE_start, log, PE_size)
    for pe in members:
        d = G.first_diff(tm.read(pe, 0, lay.bytes), after[pe])
        assert d is None, f"{what} PE {pe}: byte {d} differs from the loop of single calls"


COLL_PAIRS = [("int", "sum"), ("double", "sum"), ("float", "max"), ("bfloat16", "prod"),
              ("longdouble", "sum")]


def _table(t, count):
    """count lengths from {0, 1, 1001, V W + 3}; one entry in place, one
    target at an odd element offset (both non-empty)."""
    W = 16 // C.esize(t)
    pick = [1001, 0, 1, V * W + 3]
    lens = [pick[i % 4] for i in range(count)]
    if count == 1:
        return lens, (0,), None
    odd = {2: 3} if t != "longdouble" else {2: 1}
    return lens, (0,), odd


@pytest.mark.parametrize("count", [1, 3, 17])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_collective_device_heaps(torch_cuda, P, count):
    for t, op in COLL_PAIRS:
        lens, inplace, odd = _table(t, count)
        _collective(t, op, P, lens, 0xD0 + P + count, inplace=inplace, odd=odd)


def test_collective_strided_active_set(torch_cuda):
    lens, inplace, odd = _table("double", 17)
    _collective("double", "sum", 8, lens, 5, PE_start=1, log=1, PE_size=3,
                inplace=inplace, odd=odd)
    _collective("int", "sum", 6, [259, 0, 3], 6, PE_start=0, log=1, PE_size=3)


def test_collective_edges(torch_cuda):
    """All entries empty, count == 0, a single member (copies; long double
    padding zeroed), sources at a phase their targets share."""
    _collective("int", "sum", 2, [0, 0, -3], 1)
    _collective("int", "sum", 2, [], 1)
    _collective("longdouble", "sum", 1, [9, 0, 257], 2, inplace=(2,))
    _collective("short", "min", 4, [1001, 33], 3, PE_start=2, PE_size=1)
    _collective("float", "max", 3, [1001, 2051, 5], 4, odd={0: 1, 1: 3}, sodd={0: 1, 1: 3})


# ------------------------------------------------------ 4. host heaps (need a GPU)
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("path", ["host_fold", "getmem"])
def test_collective_host_heaps(torch_cuda, path, P):
    with D.host_heaps(path) as (force, team, ran):
        for t, op in (("double", "sum"), ("bfloat16", "prod"), ("longdouble", "sum")):
            _collective(t, op, P, [1001, 0, 300], 31 + P, inplace=(2,), path=ran, setup=force, **team)


# ------------------------------------------------------------ 5. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the pull
    path over a peer mapping (tests/support/many_mp_worker.py), each worker
    under its own time limit."""
    D.run_ranks("many_mp_worker.py", tmp_path, "MANY_MP_OK")


# ---------------------------------------------------------- 6. fatal contract
_FATAL = """
import ctypes, sys
sys.path[:0] = %r
import numpy as np
import osgpu
from support import team as T
L = osgpu.load()
pet = T.pet()
assert pet.pet_init(1) == 0
pet.pet_set_me(0)
assert L.osgpu_set_pe_ops(pet.pet_ops()) == 0
buf = np.zeros(4096, dtype=np.uint8)   # host memory: the checks come before any GPU work
a = buf.ctypes.data
psync = (ctypes.c_long * 128)()
f = osgpu.reduce_many("int", "sum")
case = sys.argv[1]
if case == "overlap":      # target 1 starts on the last element of target 0
    f([a, a + 396], [a + 1024, a + 2048], [100, 100], 0, 0, 1, None, ctypes.addressof(psync))
elif case == "source":     # target 0 runs into the source of entry 1
    f([a, a + 2048], [a + 1024, a + 396], [100, 100], 0, 0, 1, None, ctypes.addressof(psync))
else:                      # count = -1
    L.osgpu_reduce_many(1, 0, -1, None, None, None, 0, 0, 1, None, ctypes.addressof(psync))
print("RETURNED")
"""


@pytest.mark.parametrize("case,msg", [("overlap", "overlaps the target or source of another"),
                                      ("source", "overlaps the target or source of another"),
                                      ("count", "count -1 is negative")])
def test_fatal_contract(case, msg):
    code = _FATAL % ([os.path.join(ROOT, "test-resilient-osss-ucx_amd"), os.path.join(ROOT, "oracle"),
                      os.path.join(ROOT, "tests")],)
    r = subprocess.run([sys.executable, "-c", code, case], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "RETURNED" not in r.stdout, r.stdout[-2000:]
    assert msg in r.stderr, r.stderr[-2000:]


# -------------------------------------------------------------------- 7. fuzz
def test_fuzz_30_calls(torch_cuda):
    seed = int(os.environ.get("MANY_FUZZ_SEED", "20261020"))
    rng = np.random.default_rng(seed)
    pairs = ALL_PAIRS
    for i in range(30):
        t, op = pairs[int(rng.integers(len(pairs)))]
        s = C.esize(t)
        W = 16 // s
        P = int(rng.integers(1, 9))
        count = int(rng.integers(0, 21))
        lens = [int(rng.integers(0, 3 * V * W + 1)) if rng.integers(8) else 0 for _ in range(count)]
        # element shifts of targets and sources: equal (one phase, the batch
        # kernel) or not (the shifted combine)
        odd = {j: int(rng.integers(0, max(W, 2))) for j in range(count)}
        sodd = {j: odd[j] if rng.integers(3) else int(rng.integers(0, max(W, 2))) for j in range(count)}
        inplace = tuple(j for j in range(count) if rng.integers(5) == 0)
        what = f"seed {seed} call {i}: {t} {op} P={P} lens={lens} odd={odd} sodd={sodd} inplace={inplace}"
        with D.named(what):
            _collective(t, op, P, lens, seed + i, inplace=inplace, odd=odd, sodd=sodd)
