"""gpu_doors.py -- TEST INFRASTRUCTURE: what the GPU tests of the reduce front
doors (tests/test_gpu_uniform.py, _scan, _rscatter, _loc, _many, _pair_matrix,
_bounds, _half) share, once.

  fixtures      torch_cuda, small_launches, and stream(torch); a test module
                imports the fixtures by name.
  LauncherBatch cases of one raw launcher in one guarded arena: one upload, the
                launches, one synchronize, one download, and the check of every
                target (bits, long double padding, guard bands) and source
                (unchanged).  A door's subclass supplies add(), call(), want().
  collective()  one call of a door on a fresh team of PE threads, described by
                a Door; check_members() is what it asserts of the heaps after.
  forced_path, host_heaps   the library's path switches, restored on the way out.
  run_ranks()   one process per rank of a tests/support/*_mp_worker.py.
  named()       a fuzz call's description in front of what it raised.

Everything but the fixtures, LauncherBatch.launch, collective() and run_ranks()
is plain numpy and runs without a GPU (tests/test_door_harness.py).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import osgpu
from support import guarded as G
from support.rscatter_cases import dtype, esize, inputs, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_S = []


def stream(torch):
    """A non-default torch stream after draining the device (NULL means the
    calling thread's stream to the launchers, which is not ordered after
    torch's uploads)."""
    torch.cuda.synchronize()
    if not _S:
        _S.append(torch.cuda.Stream())
    return _S[0].cuda_stream


@pytest.fixture
def small_launches(monkeypatch):
    """set_limit(n): at most n threads per launch (osgpu_test_max_launch_threads),
    the multi-launch path at small sizes; 0 lifts the limit, as the end of the
    test does."""
    monkeypatch.setenv("OSGPU_TEST_HOOKS", "1")
    L = osgpu.load()
    L.osgpu_test_max_launch_threads.argtypes = [ctypes.c_longlong]

    def set_limit(n):
        assert L.osgpu_test_max_launch_threads(n) == 0, L.osgpu_last_error()
    yield set_limit
    assert L.osgpu_test_max_launch_threads(0) == 0


# ------------------------------------------------------------- raw launchers
def ptrs(bufs):
    return [g.ptr for g in bufs]


def ld_padding(raw: np.ndarray) -> bool:
    """Whether bytes 10..15 of any 16-byte long double slot of `raw` are set."""
    return bool(raw.reshape(-1, 16)[:, 10:].any())


class LauncherBatch:
    """Cases of one element type in one arena.  A subclass has

      add(...)        allocate a case's buffers from self.arena, sources first,
                      and pass them to self.case() with whatever call() and
                      want() need, as keywords;
      call(c, sp)     enqueue case c on stream sp;
      want(c, q)      the expected elements of c.dsts[q];
      out_type(c, q)  the element type of c.dsts[q], where it is not self.t;
      check_case(c, what)   more to assert of a case, if anything."""

    def __init__(self, t):
        self.t, self.s = t, esize(t)
        self.arena = G.Arena()
        self.cases = []

    def case(self, srcs, dsts, what, **key):
        c = SimpleNamespace(srcs=srcs, dsts=dsts, what=what, **key)
        self.cases.append(c)
        return c

    def launch(self, torch):
        self.arena.upload(torch)
        sp = stream(torch)
        for c in self.cases:
            self.call(c, sp)
        torch.cuda.synchronize()
        self.arena.download()
        return self

    def out_type(self, c, q):
        return self.t

    def check_case(self, c, what):
        pass

    def describe(self, c):
        key = {k: v for k, v in vars(c).items() if k not in ("srcs", "dsts", "what")}
        return f"{self.t} " + " ".join(f"{k}={v}" for k, v in key.items()) + f" {c.what}"

    def check(self):
        for c in self.cases:
            what = self.describe(c)
            for q, out in enumerate(c.dsts):
                t = self.out_type(c, q)
                bad = same_bits(t, out.data().view(dtype(t)), self.want(c, q))
                assert bad is None, f"{what}: target {q}, element {bad} differs from the oracle"
                if t == "longdouble":
                    assert not ld_padding(out.data()), \
                        f"{what}: target {q}, long double padding not zero"
                out.assert_guards(f"{what} target {q}")
            self.check_case(c, what)
            for p, g in enumerate(c.srcs):
                g.assert_unchanged(f"{what} source {p}")
        return self


def targets_identical(c, what):
    """The uniform reduce's extra: every target of the case holds the same bytes."""
    for q, out in enumerate(c.dsts):
        assert np.array_equal(out.data(), c.dsts[0].data()), \
            f"{what}: members {q} and 0 hold different bytes"


# ------------------------------------------------------------- the collective
class Door:
    """One front door to the collective driver.

      run(tm, t, op, toff, soff, n, PE_start, log, PE_size) -> the member PEs,
          after every member called the door on its own thread (support/team.py);
      expected(t, op, src, n, PE_start, log, PE_size) -> {pe: its target's elements};
      src_elems(n, PE_size)   elements of a source (the reduce-scatter: PE_size * n);
      extra(w, got, first)    more to assert of a member's target bytes, given
                              the first member's (or None)."""

    def __init__(self, name, run, expected, src_elems=lambda n, PE_size: n, extra=None):
        self.name, self.run, self.expected = name, run, expected
        self.src_elems, self.extra = src_elems, extra


def same_bytes_as_first(w, got, first):
    """The uniform reduce's extra: all members hold identical bytes."""
    assert np.array_equal(got, first), f"{w}: not the bytes of the first member"


def heap_layout(t, nsrc, n, target_elem_off=0):
    """(source offset, target offset, heap bytes): the n-element target in its
    own 4 KiB-aligned area behind the nsrc-element source, shifted by
    target_elem_off elements."""
    s = esize(t)
    toff = (nsrc * s + 4095) // 4096 * 4096 + 4096 + target_elem_off * s
    return 0, toff, toff + n * s + 8192


def check_members(tm, t, want, n, toff, hb, before, members, path, what, extra=None):
    """The heaps of tm after a call that left want[pe] in the n elements at toff
    of every member: a non-member's whole heap is as before; a member's target
    equals want[pe] bit for bit (long double: padding zero), every byte before
    and after it is as before, and it took `path` (None: not looked at)."""
    s = esize(t)
    first = None
    for pe in range(tm.npes):
        after = tm.read(pe, 0, hb)
        if pe not in members:
            assert np.array_equal(after, before[pe]), f"{what}: PE {pe} is not a member"
            continue
        w = f"{what} PE {pe}"
        got = after[toff:toff + n * s]
        bad = same_bits(t, got.view(dtype(t)), want[pe])
        assert bad is None, f"{w}: element {bad} differs"
        if t == "longdouble":
            assert not ld_padding(got), f"{w}: long double padding not zero"
        first = got if first is None else first
        if extra is not None:
            extra(w, got, first)
        assert np.array_equal(after[:toff], before[pe][:toff]), f"{w}: bytes before the target"
        assert np.array_equal(after[toff + n * s:], before[pe][toff + n * s:]), \
            f"{w}: bytes after the target"
        if path is not None:
            assert tm.last_paths[pe] == path, (w, tm.last_paths)


def collective(door, t, op, npes, n, seed, PE_start=0, log=0, PE_size=None, path="team",
               target_elem_off=0, on_source=None, device=True, host_fold=False):
    """One call of `door` on a fresh team; checks every member's result, the
    bytes round its target, the path and (in Team._on_members) pSync.
    on_source: the target lies on the source, from that element on (in place)."""
    from support import team as T
    PE_size = npes if PE_size is None else PE_size
    s = esize(t)
    nsrc = door.src_elems(n, PE_size)
    soff, toff, hb = heap_layout(t, nsrc, n, target_elem_off)
    if on_source is not None:
        toff = soff + (on_source + target_elem_off) * s
        hb += target_elem_off * s
    tm = T.Team(npes, hb, device=device, host_fold=host_fold)
    src = inputs(t, op, npes, nsrc, seed)
    for pe in range(npes):
        tm.fill(pe, 0, hb, 0xC3)
        tm.write(pe, soff, src[pe])
    before = {pe: tm.read(pe, 0, hb) for pe in range(npes)}
    members = door.run(tm, t, op, toff, soff, n, PE_start, log, PE_size)
    want = door.expected(t, op, src, n, PE_start, log, PE_size)
    check_members(tm, t, want, n, toff, hb, before, members, path,
                  f"{door.name} {t} {op} P={PE_size} n={n}", door.extra)


# ------------------------------------------------------------ path switches
@contextlib.contextmanager
def forced_path(path):
    """osgpu_set_path(path) for the block, OSGPU_PATH_AUTO after."""
    L = osgpu.load()
    try:
        assert L.osgpu_set_path(path) == 0
        yield
    finally:
        L.osgpu_set_path(osgpu.PATH_AUTO)


@contextlib.contextmanager
def host_heaps(path):
    """Host heaps by "host_fold", "getmem" or "staged".  Yields (force, team, ran):
    force() before each case sets the host path and a 2048-byte chunk (the host
    fold needs neither), team are the Team keywords, ran is the path
    osgpu_last_path() names (a forced STAGED takes GETMEM below the staging
    size).  The library's host path, chunk and fold limit are reset after."""
    L = osgpu.load()

    def force():
        if path != "host_fold":
            assert L.osgpu_set_host_path(osgpu.HOST_PATHS[path]) == 0
            assert L.osgpu_set_host_chunk_bytes(2048) == 0
    try:
        yield (force, dict(device=False, host_fold=(path == "host_fold")),
               "host_fold" if path == "host_fold" else "getmem")
    finally:
        L.osgpu_set_host_path(-1)
        L.osgpu_set_host_chunk_bytes(-1)
        L.osgpu_set_host_fold_max_bytes(-1)


# ------------------------------------------------------------- several ranks
def run_ranks(worker, tmp_path, ok_token, world=2):
    """`world` ranks of tests/support/<worker>, one fresh process each under a
    time limit of its own, all on one GPU.  Every rank must exit 0 and print
    ok_token; if one outlives its limit all are killed and the test fails."""
    worker = os.path.join(ROOT, "tests", "support", worker)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, worker, str(tmp_path)],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(world),
                                       LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                                       MASTER_PORT=str(port), PYTHONUNBUFFERED="1"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=180)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ok_token in o, f"rank {r} (status {p.returncode}):\n{o[-3000:]}"


# ----------------------------------------------------------------------- fuzz
@contextlib.contextmanager
def named(what):
    """An AssertionError of the block, with `what` (the fuzz call) in front."""
    try:
        yield
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
