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
import socket
import subprocess
import sys

import numpy as np
import pytest

import osgpu
from support import guarded as G
from support import scan_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = C.TILE_VECTORS
RAW_PAIRS = C.PAIRS + [("float", "max")]    # float max: NaNs and signed zeros (the edge inputs)


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
    synchronize, one download.  The expected values of P members are computed
    once at the longest length and sliced."""

    def __init__(self, t, op, nmax, seed):
        self.t, self.op, self.s = t, op, C.esize(t)
        self.pool = C.inputs(t, op, 8, nmax, seed)
        self.inc = {}       # P -> the inclusive results of P members at nmax
        self.arena = G.Arena()
        self.cases = []

    def add(self, P, n, ex, src_phase, dst_phases, what):
        srcs = [self.arena.add(n * self.s, src_phase, self.pool[p][:n]) for p in range(P)]
        dsts = [self.arena.add(n * self.s, dst_phases[q]) for q in range(P)]
        self.cases.append((P, n, ex, srcs, dsts, what))

    def launch(self, torch):
        self.arena.upload(torch)
        sp = _stream(torch)
        for P, n, ex, srcs, dsts, _ in self.cases:
            osgpu.team_scan(self.t, self.op, ex, [g.ptr for g in dsts], [g.ptr for g in srcs], n,
                            stream=sp)
        torch.cuda.synchronize()
        self.arena.download()
        return self

    def want(self, P, q, n, ex):
        if P not in self.inc:
            self.inc[P] = C.inclusive(self.t, self.op, self.pool[:P])
        if ex and q == 0:
            return np.repeat(C.identity(self.t, self.op), n)
        return self.inc[P][q - ex][:n]

    def check(self):
        for P, n, ex, srcs, dsts, what in self.cases:
            what = f"{self.t} {self.op} P={P} n={n} exclusive={ex} {what}"
            for q, out in enumerate(dsts):
                got = out.data().view(C.dtype(self.t))
                bad = C.same_bits(self.t, got, self.want(P, q, n, ex))
                assert bad is None, f"{what}: member {q}, element {bad} differs from the oracle"
                out.assert_guards(f"{what} target {q}")
            for p, g in enumerate(srcs):
                g.assert_unchanged(f"{what} source {p}")


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


@pytest.fixture
def small_launches(monkeypatch):
    """osgpu_test_max_launch_threads: the multi-launch path at small sizes."""
    monkeypatch.setenv("OSGPU_TEST_HOOKS", "1")
    L = osgpu.load()
    L.osgpu_test_max_launch_threads.argtypes = [ctypes.c_longlong]

    def set_limit(n):
        assert L.osgpu_test_max_launch_threads(n) == 0, L.osgpu_last_error()
    yield set_limit
    assert L.osgpu_test_max_launch_threads(0) == 0


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
        res.append([d.data().copy() for c in b.cases for d in c[4]])
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
def _heap_layout(t, n, target_elem_off=0):
    """(source offset, target offset, heap bytes): the target in its own
    4 KiB-aligned area behind the source, shifted by target_elem_off elements."""
    s = C.esize(t)
    toff = (n * s + 4095) // 4096 * 4096 + 4096 + target_elem_off * s
    return 0, toff, toff + n * s + 8192


def _check_members(tm, t, op, ex, src, n, soff, toff, hb, before, members, start, log, size, path,
                   what):
    s = C.esize(t)
    want = C.expected(t, op, src, ex, start, log, size)
    for pe in range(tm.npes):
        after = tm.read(pe, 0, hb)
        if pe not in members:
            assert np.array_equal(after, before[pe]), f"{what}: PE {pe} is not a member"
            continue
        w = f"{what} PE {pe}"
        got = after[toff:toff + n * s]
        bad = C.same_bits(t, got.view(C.dtype(t)), want[pe])
        assert bad is None, f"{w}: element {bad} differs"
        if t == "longdouble":
            assert not got.reshape(-1, 16)[:, 10:].any(), f"{w}: long double padding not zero"
        assert np.array_equal(after[:toff], before[pe][:toff]), f"{w}: bytes before the target"
        assert np.array_equal(after[toff + n * s:], before[pe][toff + n * s:]), \
            f"{w}: bytes after the target"
        if path is not None:
            assert tm.last_paths[pe] == path, (w, tm.last_paths)


def _collective(torch, t, op, ex, npes, n, seed, PE_start=0, log=0, PE_size=None, path="team",
                target_elem_off=0, in_place=False, device=True, host_fold=False):
    """One call on a fresh team; checks every member's result, the bytes
    round its target, the path and (in Team._on_members) pSync."""
    from support import team as T
    PE_size = npes if PE_size is None else PE_size
    soff, toff, hb = _heap_layout(t, n, target_elem_off)
    if in_place:
        toff = soff + target_elem_off * C.esize(t)
        hb += target_elem_off * C.esize(t)
    tm = T.Team(npes, hb, device=device, host_fold=host_fold)
    src = C.inputs(t, op, npes, n, seed)
    for pe in range(npes):
        tm.fill(pe, 0, hb, 0xC3)
        tm.write(pe, soff, src[pe])
    before = {pe: tm.read(pe, 0, hb) for pe in range(npes)}
    members = C.run(tm, t, op, ex, toff, soff, n, PE_start, log, PE_size)
    _check_members(tm, t, op, ex, src, n, soff, toff, hb, before, members, PE_start, log, PE_size,
                   path, f"{t} {op} exclusive={ex} P={PE_size} n={n}")


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, op, P):
    W = 16 // C.esize(t)
    for n in sorted({1, P - 1, 1001, P * V * W + 3}):
        for ex in (0, 1):
            _collective(torch_cuda, t, op, ex, P, n, 0xD0 + P)


def test_collective_strided_active_set(torch_cuda):
    for ex in (0, 1):
        _collective(torch_cuda, "double", "sum", ex, 8, 1001, 5, PE_start=1, log=1, PE_size=3)
        _collective(torch_cuda, "short", "min", ex, 6, 259, 6, PE_start=0, log=1, PE_size=3)


def test_collective_pull_forms(torch_cuda):
    """OSGPU_PATH_PULL, in-place overlap, long double and 9 members (the team
    form stops at 8) take the pull form."""
    L = osgpu.load()
    for ex in (0, 1):
        try:
            assert L.osgpu_set_path(osgpu.PATH_PULL) == 0
            _collective(torch_cuda, "double", "sum", ex, 3, 1001, 21, path="pull")
            _collective(torch_cuda, "half", "sum", ex, 8, 515, 22, path="pull")
        finally:
            L.osgpu_set_path(osgpu.PATH_AUTO)
        _collective(torch_cuda, "float", "prod", ex, 3, 1001, 23, path="pull", in_place=True)
        _collective(torch_cuda, "int", "sum", ex, 4, 7, 24, path="pull", in_place=True,
                    target_elem_off=3)
        _collective(torch_cuda, "longdouble", "sum", ex, 3, 257, 25, path="pull")
        _collective(torch_cuda, "longdouble", "max", ex, 2, 33, 26, path="pull")
        _collective(torch_cuda, "int", "sum", ex, 9, 1001, 27, path="pull")
        _collective(torch_cuda, "float", "max", ex, 9, 130, 28, path="pull")


def test_collective_single_member(torch_cuda):
    """PE_size == 1: a copy (inclusive) or the identity (exclusive)."""
    for ex in (0, 1):
        _collective(torch_cuda, "int", "sum", ex, 1, 1001, 5, path=None)
        _collective(torch_cuda, "double", "min", ex, 4, 11, 6, PE_start=2, PE_size=1, path=None)
        _collective(torch_cuda, "longdouble", "prod", ex, 1, 9, 7, path=None)
        _collective(torch_cuda, "short", "and", ex, 1, 77, 8, path=None, in_place=True)


def test_collective_target_sub_view(torch_cuda):
    """A target an odd number of elements into its array: its phase differs
    from the sources', the team path's element-granular kernel."""
    for t, op in (("short", "min"), ("int", "sum"), ("half", "sum")):
        for ex in (0, 1):
            _collective(torch_cuda, t, op, ex, 3, 1001, 0x5B, target_elem_off=3)


# ------------------------------------------------------ 3. host heaps (need a GPU)
@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path; a
    forced STAGED takes GETMEM), the chunk below the array size; a strided
    set, overlap, one member, long double."""
    L = osgpu.load()
    cases = [("double", "sum", 3, 0, 0, 3, 1001, False), ("short", "min", 2, 0, 0, 2, 5, False),
             ("float", "prod", 8, 1, 1, 3, 700, False), ("int", "sum", 3, 0, 0, 3, 1001, True),
             ("half", "sum", 3, 0, 0, 3, 1501, False), ("longdouble", "sum", 3, 0, 0, 3, 300, False),
             ("longdouble", "max", 1, 0, 0, 1, 9, False), ("complexf", "prod", 2, 0, 0, 2, 333, True)]
    ran = "host_fold" if path == "host_fold" else "getmem"
    try:
        for t, op, npes, start, log, size, n, ov in cases:
            for ex in (0, 1):
                if path != "host_fold":
                    assert L.osgpu_set_host_path(osgpu.HOST_PATHS[path]) == 0
                    assert L.osgpu_set_host_chunk_bytes(2048) == 0
                _collective(torch_cuda, t, op, ex, npes, n, 31 + n, start, log, size, path=ran,
                            in_place=ov, device=False, host_fold=(path == "host_fold"))
    finally:
        L.osgpu_set_host_path(-1)
        L.osgpu_set_host_chunk_bytes(-1)
        L.osgpu_set_host_fold_max_bytes(-1)


# ------------------------------------------------------------ 4. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the team
    kernel writes a peer's target through a mapping of another process's
    memory (tests/support/scan_mp_worker.py)."""
    worker = os.path.join(ROOT, "tests", "support", "scan_mp_worker.py")
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
        assert p.returncode == 0 and "SCAN_MP_OK" in o, f"rank {r}:\n{o[-3000:]}"


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
        try:
            _collective(torch_cuda, t, op, ex, P, n, seed + i, target_elem_off=shift,
                        in_place=overlap, path="team" if team else "pull")
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
