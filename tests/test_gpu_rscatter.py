"""The reduce-scatter on the GPU: osgpu_combine_shifted (combine_shift_kernel,
csrc/combine.hip) and osgpu_reduce_scatter on device heaps.

1. The raw launcher against the reduce-to-all oracle's left-to-right fold,
   at the smallest shapes that reach each branch of the kernel and its
   launcher.  With W = 16 / element size elements per vector and V * W the
   elements of one tile (V = 128 vectors, OSGPU_SHIFT_U = 2):
   lengths 1, W-1, W, W+1, V W-1, V W, V W+1, 2 V W + W-1 (1 and W-1 leave
   no whole target vector at a non-zero shift); every target shift 0..W-1
   against sources at shift 0 (K = 2), shifts 1 and W-1 at K = 3, 8 and 9
   (9: a second chunk, the target fed back at a phase the sources do not
   share); every source at its own shift; one pointer off its element
   alignment (the element-granular kernel); long double and complexd, which
   keep their kernels.  Every input is allocated EXACTLY n elements between
   guard bands (tests/support/guarded.py); the target sits between bands
   too, and every source must come back bitwise unchanged.  What the bands
   can show is a WRITE outside the target or a fold that takes an element
   from the wrong offset.  They cannot show an aligned load that reaches
   past an input's end: the kernel discards the bytes of such a load that
   lie outside the 16 it folds, so the result would be the same.  (Nor can
   the guard layout put an input's end at the end of a mapping: a band
   always follows the payload.)  That the launcher keeps every aligned load
   inside its input (launch_shift_k: cut_first / cut_last) is checked by
   reading it, not here.
   test_launcher_routes asserts, from the launcher's own counters, which
   kernel each chunk took: every route gives the same bits, so nothing else
   tells the shift kernel from a fall-back.
2. The collective with threads as PEs on device heaps: P in {2, 3, 8},
   nreduce in {1, 1001, V W + 3}, a strided active set, in-place overlap, a
   target sub-view at an odd element offset; the pull path, pSync back at 0,
   the bytes round every member's target untouched.
3. Two processes on one GPU through osgpu_heap_create
   (tests/support/rscatter_mp_worker.py).
4. A seeded fuzz of 30 calls.

Expected values: tests/support/rscatter_cases.py (the reduce-to-all oracle
over the full P * n sources, member m's block m sliced out).
"""
import ctypes
import os

import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import rscatter_cases as C
from support.gpu_doors import small_launches, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

V = C.TILE_VECTORS


def lengths(t):
    W = 16 // C.esize(t)
    return sorted({1, max(W - 1, 1), W, W + 1, V * W - 1, V * W, V * W + 1, 2 * V * W + W - 1})


# ------------------------------------------------------------ 1. raw launcher
class Batch(D.LauncherBatch):
    """Cases of one (type, op): K inputs folded into one target."""

    def __init__(self, t, op, kmax, nmax, seed):
        super().__init__(t)
        self.op = op
        self.pool = C.inputs(t, op, kmax, nmax, seed)
        self.fold = {}      # K -> fold of pool[:K] at nmax

    def add(self, K, n, tgt_phase, src_phases, what):
        srcs = [self.arena.add(n * self.s, src_phases[k], self.pool[k][:n]) for k in range(K)]
        self.case(srcs, [self.arena.add(n * self.s, tgt_phase)], what, op=self.op, K=K, n=n)

    def launch(self, torch, shifted=True):
        self.launcher = osgpu.combine_shifted if shifted else osgpu.combine
        return super().launch(torch)

    def call(self, c, sp):
        self.launcher(self.t, self.op, c.dsts[0].ptr, D.ptrs(c.srcs), c.n, stream=sp)

    def want(self, c, q):
        if c.K not in self.fold:
            self.fold[c.K] = C.fold_left(self.t, self.op, self.pool[:c.K])
        return self.fold[c.K][:c.n]


@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_launcher_phases_and_lengths(torch_cuda, t, op):
    s = C.esize(t)
    W = 16 // s
    ns = lengths(t)
    b = Batch(t, op, 9, max(ns), 0x5CA7 + s)
    for shift in range(W):          # every target shift, sources at shift 0
        for n in ns:
            b.add(2, n, shift * s, [0, 0], f"target shift {shift}")
    for K in (3, 8, 9):
        for shift in sorted({1, W - 1}):
            for n in ns:
                b.add(K, n, shift * s, [0] * K, f"target shift {shift}")
    for K in (3, 8, 9):             # every source at its own shift
        for n in ns:
            b.add(K, n, (3 * s) % 16, [((k + 1) % W) * s for k in range(K)], "mixed shifts")
    off = s // 2                    # a pointer off its element alignment
    for n in (W + 1, V * W + 1):
        b.add(3, n, 0, [0, off, 0], f"source 1 at byte phase {off}")
        b.add(2, n, off, [0, 0], f"target at byte phase {off}")
    b.launch(torch_cuda).check()


@pytest.mark.parametrize("t,op,phases", [("longdouble", "sum", (0, 0)), ("complexd", "prod", (0, 0)),
                                         ("complexd", "prod", (8, 0))],
                         ids=["longdouble", "complexd", "complexd_8_off"])
def test_launcher_16_byte_elements_keep_their_kernels(torch_cuda, t, op, phases):
    b = Batch(t, op, 9, 2 * V + 1, 0x16B)
    for K in (2, 3, 9):
        for n in (1, V, 2 * V + 1):
            b.add(K, n, phases[0], [phases[1]] * K, f"phases {phases}")
    b.launch(torch_cuda).check()


def test_launcher_equal_phases_match_osgpu_combine(torch_cuda):
    """All phases equal: the launcher hands over to osgpu_combine's kernels."""
    for t, op in (("float", "prod"), ("short", "min")):
        s = C.esize(t)
        a, b = (Batch(t, op, 9, 3 * V * (16 // s), 77) for _ in range(2))
        for x in (a, b):
            for K in (1, 2, 9):
                x.add(K, 3 * V * (16 // s) - 1, s, [s] * K, "equal phases")
        a.launch(torch_cuda, shifted=True).check()
        b.launch(torch_cuda, shifted=False).check()


@pytest.mark.parametrize("t,op", [("int", "sum"), ("short", "min"), ("double", "sum")],
                         ids=lambda x: x)
def test_launcher_multi_launch(torch_cuda, small_launches, t, op):
    """3 tiles and 3 tiles + 1 vector at shifts 1 and W-1: several launches
    over shifted pointers give what one launch gives (and the oracle)."""
    s = C.esize(t)
    W = 16 // s
    res = []
    for limit in (0, 256):
        small_launches(limit)
        b = Batch(t, op, 3, (3 * V + 5) * W, 0x3717E)
        for K in (2, 3):
            # (the body gives a vector up to the edges at either end where an
            # input's cover would leave it: + 2 and + 3 land on 3 tiles (+ 1))
            for nvec in (3 * V, 3 * V + 1, 3 * V + 2, 3 * V + 3):
                for shift in sorted({1, W - 1}):
                    # a head of W - shift elements, then nvec whole target vectors
                    b.add(K, (W - shift) % W + nvec * W + 1, shift * s, [0] * K,
                          f"limit {limit} shift {shift}")
        b.launch(torch_cuda).check()
        res.append([c.dsts[0].data().copy() for c in b.cases])
    for one, many in zip(*res):
        assert np.array_equal(one, many)


def _routes(L):
    """osgpu_test_shift_routes: [chunks on osgpu_combine's kernels, chunks on
    the shift kernel, chunks off their element alignment, launches of the
    shift kernel] so far in this process."""
    L.osgpu_test_shift_routes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong * 4),
                                          ctypes.POINTER(ctypes.c_int)]
    c, u = (ctypes.c_ulonglong * 4)(), ctypes.c_int()
    assert L.osgpu_test_shift_routes(ctypes.byref(c), ctypes.byref(u)) == 0, L.osgpu_last_error()
    assert u.value * 64 == V, "tests/support/rscatter_cases.py TILE_VECTORS is not the shipped tile"
    return np.array(list(c), dtype=np.int64)


def test_launcher_routes(torch_cuda, small_launches):
    """Which kernel each chunk takes.  Every route gives the same bits, so the
    value checks above cannot tell combine_shift_kernel from a fall-back to
    the element-granular kernel: the launcher's own counters do."""
    L = osgpu.load()
    t, op, s, W = "float", "prod", 4, 4

    def delta(K, n, tgt_phase, src_phases, t=t, op=op):
        b = Batch(t, op, K, n, 0xA0)
        b.add(K, n, tgt_phase, src_phases, "route")
        before = _routes(L)
        b.launch(torch_cuda).check()
        return list(_routes(L) - before)

    small_launches(0)
    n = 3 * V * W + 1      # target phase 4: a head of 3 elements, 3 V - 1 vectors (3 tiles), a tail of 2
    assert delta(3, n, s, [0] * 3) == [0, 1, 0, 1], "phases differ: the shift kernel"
    assert delta(3, n, s, [0, 8, 12]) == [0, 1, 0, 1], "every input at its own phase"
    # 9 inputs: 8, then the target (phase 4) fed back with the ninth (phase 0)
    assert delta(9, n, s, [0] * 9) == [0, 2, 0, 2], "both chunks on the shift kernel"
    assert delta(3, 1, s, [0] * 3) == [0, 1, 0, 1], "no whole vector: its edges alone"
    assert delta(3, n, s, [s] * 3) == [1, 0, 0, 0], "equal phases: osgpu_combine's kernels"
    assert delta(1, n, s, [0]) == [1, 0, 0, 0], "one input: a copy"
    assert delta(3, n, 0, [0, 2, 0]) == [0, 0, 1, 0], "off the element alignment"
    assert delta(2, V + 1, 8, [0, 0], "complexd", "prod") == [1, 0, 0, 0], "16-byte elements"
    small_launches(256)    # K = 2: two tiles per launch, K = 3: one
    assert delta(2, n, s, [0, 0]) == [0, 1, 0, 2]
    assert delta(3, n, s, [0] * 3) == [0, 1, 0, 3]


# ---------------------------------------------------- 2. collective, PE threads
RSCATTER = D.Door("reduce-scatter", C.run, C.expected, src_elems=lambda n, PE_size: PE_size * n)


def _collective(t, op, npes, n, seed, PE_start=0, log=0, PE_size=None, target_elem_off=0,
                overlap_block=None, path="pull", **kw):
    """overlap_block: the target on top of that block of the source."""
    D.collective(RSCATTER, t, op, npes, n, seed, PE_start, log, PE_size, path, target_elem_off,
                 on_source=None if overlap_block is None else overlap_block * n, **kw)


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, op, P):
    W = 16 // C.esize(t)
    for n in (1, 1001, V * W + 3):
        _collective(t, op, P, n, 0xD0 + P)


def test_collective_strided_active_set(torch_cuda):
    _collective("double", "sum", 8, 1001, 5, PE_start=1, log=1, PE_size=3)
    _collective("short", "min", 6, 259, 6, PE_start=0, log=1, PE_size=3)


@pytest.mark.parametrize("block", [0, 1, 2])
def test_collective_in_place(torch_cuda, block):
    """The target on top of a block of the source (the caller's own block on
    one member, another's on the others)."""
    _collective("float", "prod", 3, 1001, 9 + block, overlap_block=block)
    _collective("int", "sum", 3, 7, 19 + block, overlap_block=block)


def test_collective_target_sub_view(torch_cuda):
    """A target that starts an odd number of elements into its array."""
    for t, op in (("short", "min"), ("int", "sum"), ("double", "sum"), ("half", "sum")):
        _collective(t, op, 3, 1001, 0x5B, target_elem_off=3)


def test_collective_long_double_and_single_member(torch_cuda):
    _collective("longdouble", "sum", 3, 257, 3)
    _collective("complexd", "prod", 2, 129, 4)
    _collective("int", "sum", 1, 1001, 5)          # PE_size == 1: a copy
    _collective("double", "sum", 4, 11, 6, PE_start=2, PE_size=1)


# ------------------------------------------------------ host heaps (need a GPU)
@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path;
    a forced STAGED takes GETMEM): blocks, a strided set, overlap with the
    caller's own and another block, a chunk smaller than the block."""
    cases = [("double", "sum", 3, 0, 0, 3, 1001, None), ("short", "min", 2, 0, 0, 2, 5, None),
             ("float", "prod", 8, 1, 1, 3, 300, None), ("int", "sum", 3, 0, 0, 3, 1001, 0),
             ("long", "xor", 3, 0, 0, 3, 64, 1), ("half", "sum", 3, 0, 0, 3, 1001, None),
             ("longdouble", "sum", 1, 0, 0, 1, 9, None), ("complexf", "prod", 1, 0, 0, 1, 33, None)]
    with D.host_heaps(path) as (force, team, ran):
        for t, op, npes, start, log, size, n, ov in cases:
            force()
            _collective(t, op, npes, n, 31 + n, start, log, size, overlap_block=ov, path=ran, **team)


# ------------------------------------------------------------ 3. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the pull
    path over a peer mapping (tests/support/rscatter_mp_worker.py)."""
    D.run_ranks("rscatter_mp_worker.py", tmp_path, "RSCATTER_MP_OK")


# -------------------------------------------------------------------- 4. fuzz
def test_fuzz_30_calls(torch_cuda):
    seed = int(os.environ.get("RSCATTER_FUZZ_SEED", "20261020"))
    rng = np.random.default_rng(seed)
    pairs = C.PAIRS + [("bfloat16", "max"), ("longlong", "and"), ("float", "min"),
                       ("longdouble", "prod"), ("complexd", "sum")]
    for i in range(30):
        t, op = pairs[int(rng.integers(len(pairs)))]
        P = int(rng.integers(1, 9))
        n = int(rng.integers(1, 5001))
        W = 16 // C.esize(t)
        shift = int(rng.integers(0, W)) if W > 1 else 0
        overlap = bool(rng.integers(2)) and P > 1
        what = f"seed {seed} call {i}: {t} {op} P={P} n={n} shift={shift} overlap={overlap}"
        with D.named(what):
            _collective(t, op, P, n, seed + i, target_elem_off=shift,
                        overlap_block=int(rng.integers(P)) if overlap else None)
