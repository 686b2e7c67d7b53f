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
import socket
import subprocess
import sys

import numpy as np
import pytest

import osgpu
from support import guarded as G
from support import rscatter_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = C.TILE_VECTORS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_S = []


def _stream(torch):
    """A non-default torch stream after draining the device (NULL means the
    calling thread's stream to the launchers, which is not ordered after
    torch's uploads)."""
    torch.cuda.synchronize()
    if not _S:
        _S.append(torch.cuda.Stream())
    return _S[0].cuda_stream


def lengths(t):
    W = 16 // C.esize(t)
    return sorted({1, max(W - 1, 1), W, W + 1, V * W - 1, V * W, V * W + 1, 2 * V * W + W - 1})


# ------------------------------------------------------------ 1. raw launcher
class Batch:
    """Cases of one (type, op) in one arena: one upload, the launches, one
    synchronize, one download."""

    def __init__(self, t, op, kmax, nmax, seed):
        self.t, self.op, self.s = t, op, C.esize(t)
        self.pool = C.inputs(t, op, kmax, nmax, seed)
        self.want = {}      # K -> fold of pool[:K] at nmax
        self.arena = G.Arena()
        self.cases = []

    def add(self, K, n, tgt_phase, src_phases, what):
        srcs = [self.arena.add(n * self.s, src_phases[k], self.pool[k][:n]) for k in range(K)]
        out = self.arena.add(n * self.s, tgt_phase)
        self.cases.append((K, n, srcs, out, what))

    def launch(self, torch, shifted=True):
        self.arena.upload(torch)
        sp = _stream(torch)
        f = osgpu.combine_shifted if shifted else osgpu.combine
        for K, n, srcs, out, _ in self.cases:
            f(self.t, self.op, out.ptr, [g.ptr for g in srcs], n, stream=sp)
        torch.cuda.synchronize()
        self.arena.download()
        return self

    def check(self):
        for K, n, srcs, out, what in self.cases:
            what = f"{self.t} {self.op} K={K} n={n} {what}"
            if K not in self.want:
                self.want[K] = C.fold_left(self.t, self.op, self.pool[:K])
            got = out.data().view(C.dtype(self.t)) if self.t != "longdouble" else out.data()
            want = self.want[K][:n]
            if self.t == "longdouble":
                got = got.view(np.longdouble)
                pad = out.data().reshape(-1, 16)[:, 10:]
                assert not pad.any(), f"{what}: long double padding not zero"
            bad = C.same_bits(self.t, got, want)
            assert bad is None, f"{what}: element {bad} differs from the oracle's fold"
            out.assert_guards(what + " target")
            for k, g in enumerate(srcs):
                g.assert_unchanged(f"{what} input {k}")


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


@pytest.fixture
def small_launches(monkeypatch):
    """At most 256 threads per launch (osgpu_test_max_launch_threads): at
    K = 2 a launch holds two tiles, at K = 3 one."""
    monkeypatch.setenv("OSGPU_TEST_HOOKS", "1")
    L = osgpu.load()
    L.osgpu_test_max_launch_threads.argtypes = [ctypes.c_longlong]

    def set_limit(n):
        assert L.osgpu_test_max_launch_threads(n) == 0, L.osgpu_last_error()
    yield set_limit
    assert L.osgpu_test_max_launch_threads(0) == 0


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
        res.append([c[3].data().copy() for c in b.cases])
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
def _heap_layout(t, P, n, target_elem_off=0):
    """(source offset, target offset, heap bytes): the target in its own
    4 KiB-aligned area behind the source, shifted by target_elem_off elements."""
    s = C.esize(t)
    src_bytes = P * n * s
    toff = (src_bytes + 4095) // 4096 * 4096 + 4096 + target_elem_off * s
    return 0, toff, toff + n * s + 8192


def _collective(torch, t, op, npes, n, seed, PE_start=0, log=0, PE_size=None, target_elem_off=0,
                overlap_block=None):
    """One call on a fresh team; checks every member's block, the bytes
    round its target, the path and (in Team._on_members) pSync."""
    from support import team as T
    PE_size = npes if PE_size is None else PE_size
    s = C.esize(t)
    soff, toff, hb = _heap_layout(t, PE_size, n, target_elem_off)
    if overlap_block is not None:   # the target on top of block `overlap_block` of the source
        toff = soff + (overlap_block * n + target_elem_off) * s
    tm = T.Team(npes, hb, device=True)
    src = C.inputs(t, op, npes, PE_size * n, seed)
    for pe in range(npes):
        tm.fill(pe, 0, hb, 0xC3)
        tm.write(pe, soff, src[pe])
    before = {pe: tm.read(pe, 0, hb) for pe in range(npes)}
    members = C.run(tm, t, op, toff, soff, n, PE_start, log, PE_size)
    want = C.expected(t, op, src, n, PE_start, log, PE_size)
    for pe in range(npes):
        after = tm.read(pe, 0, hb)
        if pe not in members:
            assert np.array_equal(after, before[pe]), f"PE {pe} is not a member"
            continue
        got = after[toff:toff + n * s].view(C.dtype(t))
        bad = C.same_bits(t, got, want[pe])
        what = f"{t} {op} P={PE_size} n={n} PE {pe}"
        assert bad is None, f"{what}: element {bad} differs"
        assert np.array_equal(after[:toff], before[pe][:toff]), f"{what}: bytes before the target"
        assert np.array_equal(after[toff + n * s:], before[pe][toff + n * s:]), \
            f"{what}: bytes after the target"
        assert tm.last_paths[pe] == "pull", tm.last_paths


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, op, P):
    W = 16 // C.esize(t)
    for n in (1, 1001, V * W + 3):
        _collective(torch_cuda, t, op, P, n, 0xD0 + P)


def test_collective_strided_active_set(torch_cuda):
    _collective(torch_cuda, "double", "sum", 8, 1001, 5, PE_start=1, log=1, PE_size=3)
    _collective(torch_cuda, "short", "min", 6, 259, 6, PE_start=0, log=1, PE_size=3)


@pytest.mark.parametrize("block", [0, 1, 2])
def test_collective_in_place(torch_cuda, block):
    """The target on top of a block of the source (the caller's own block on
    one member, another's on the others)."""
    _collective(torch_cuda, "float", "prod", 3, 1001, 9 + block, overlap_block=block)
    _collective(torch_cuda, "int", "sum", 3, 7, 19 + block, overlap_block=block)


def test_collective_target_sub_view(torch_cuda):
    """A target that starts an odd number of elements into its array."""
    for t, op in (("short", "min"), ("int", "sum"), ("double", "sum"), ("half", "sum")):
        _collective(torch_cuda, t, op, 3, 1001, 0x5B, target_elem_off=3)


def test_collective_long_double_and_single_member(torch_cuda):
    _collective(torch_cuda, "longdouble", "sum", 3, 257, 3)
    _collective(torch_cuda, "complexd", "prod", 2, 129, 4)
    _collective(torch_cuda, "int", "sum", 1, 1001, 5)          # PE_size == 1: a copy
    _collective(torch_cuda, "double", "sum", 4, 11, 6, PE_start=2, PE_size=1)


# ------------------------------------------------------ host heaps (need a GPU)
@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path;
    a forced STAGED takes GETMEM): blocks, a strided set, overlap with the
    caller's own and another block, a chunk smaller than the block."""
    from support import team as T
    L = osgpu.load()
    cases = [("double", "sum", 3, 0, 0, 3, 1001, None), ("short", "min", 2, 0, 0, 2, 5, None),
             ("float", "prod", 8, 1, 1, 3, 300, None), ("int", "sum", 3, 0, 0, 3, 1001, 0),
             ("long", "xor", 3, 0, 0, 3, 64, 1), ("half", "sum", 3, 0, 0, 3, 1001, None),
             ("longdouble", "sum", 1, 0, 0, 1, 9, None), ("complexf", "prod", 1, 0, 0, 1, 33, None)]
    try:
        for t, op, npes, start, log, size, n, ov in cases:
            s = C.esize(t)
            soff, toff, hb = _heap_layout(t, size, n)
            if ov is not None:
                toff = soff + ov * n * s
            tm = T.Team(npes, hb, device=False, host_fold=(path == "host_fold"))
            if path != "host_fold":
                assert L.osgpu_set_host_path(osgpu.HOST_PATHS[path]) == 0
                assert L.osgpu_set_host_chunk_bytes(2048) == 0
            src = C.inputs(t, op, npes, size * n, 31 + n)
            for pe in range(npes):
                tm.fill(pe, 0, hb, 0xC3)
                tm.write(pe, soff, src[pe])
            before = {pe: tm.read(pe, 0, hb) for pe in range(npes)}
            members = C.run(tm, t, op, toff, soff, n, start, log, size)
            want = C.expected(t, op, src, n, start, log, size)
            for pe in members:
                after = tm.read(pe, 0, hb)
                bad = C.same_bits(t, after[toff:toff + n * s].view(C.dtype(t)), want[pe])
                assert bad is None, f"{path} {t} {op} P={size} n={n} PE {pe}: element {bad}"
                assert np.array_equal(after[:toff], before[pe][:toff])
                assert np.array_equal(after[toff + n * s:], before[pe][toff + n * s:])
                assert tm.last_paths[pe] == ("host_fold" if path == "host_fold" else "getmem")
    finally:
        L.osgpu_set_host_path(-1)
        L.osgpu_set_host_chunk_bytes(-1)
        L.osgpu_set_host_fold_max_bytes(-1)


# ------------------------------------------------------------ 3. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the pull
    path over a peer mapping (tests/support/rscatter_mp_worker.py)."""
    worker = os.path.join(ROOT, "tests", "support", "rscatter_mp_worker.py")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, worker, str(tmp_path)],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                                       PYTHONUNBUFFERED="1"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=150)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "RSCATTER_MP_OK" in o, f"rank {r}:\n{o[-3000:]}"


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
        try:
            _collective(torch_cuda, t, op, P, n, seed + i, target_elem_off=shift,
                        overlap_block=int(rng.integers(P)) if overlap else None)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
