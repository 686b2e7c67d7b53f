"""Every (type, op) pair of the library through every reduce kernel and front
door that the per-door tests run for seven pairs only.

a. The raw launchers osgpu_combine_shifted, osgpu_team_scan (both modes) and
   osgpu_team_uniform, parametrized over (kernel, type) with the type's ops
   looped inside one arena and one upload: 2, 3 and 8 members (inputs) at
   n_small = W + 1 and at n_tile (a whole tile, one more vector, W - 1 more
   elements), each at three placements -- every pointer at phase 0, every
   pointer one element on (a scalar head and tail), one target at another
   phase (a target shift of 1 and of W - 1 for the shifted combine, the
   element-granular kernel for the scan and the uniform reduce).  16-byte
   elements have no "one element on": complexd runs phase 8 (target only for
   the combine), long double one pointer at phase 8 on the uniform kernel.
   Every array is exactly n elements between guard bands, every source comes
   back unchanged, values are compared bit for bit (long double: 10 value
   bytes, zero padding), the exclusive scan's member 0 holds the identity.
b. The collective, parametrized over (door, type): reduce-scatter, batched,
   scan (both modes), uniform and location, each pair on members 1, 2, 3 of a
   4-PE team by four paths -- device heaps automatic, device heaps
   OSGPU_PATH_PULL, host heaps by the host fold, host heaps by GETMEM with a
   2048-byte chunk (two chunks or more, the last ragged).
c. Eight members on the collective for the heaviest instantiations.

Inputs, lengths and the driver: tests/support/matrix_cases.py; the inputs'
conditions are asserted without a GPU in tests/test_matrix_ref.py.
"""
import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import guarded as G
from support import matrix_cases as X
from support import rscatter_cases as C
from support import scan_cases as S
from support import uniform_cases as U
from support.gpu_doors import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ a. raw launchers
def placements(kernel, t, P):
    """[(what, source phases, target phases)]; the shifted combine has one target."""
    s, W = X.esize(t), X.width(t)
    nt = 1 if kernel == "combine_shifted" else P
    out = [("phase 0", [0] * P, [0] * nt)]
    if W > 1:
        out.append(("one element on", [s] * P, [s] * nt))
        if kernel == "combine_shifted":
            for shift in sorted({1, W - 1}):
                out.append((f"target shift {shift}", [0] * P, [shift * s]))
        else:
            other = [s] * P
            other[P - 1] = (2 * s) % 16
            out.append((f"target {P - 1} at phase {other[P - 1]}", [s] * P, other))
    elif t == "complexd":
        out.append(("target at phase 8", [0] * P, [8] * nt) if kernel == "combine_shifted" else
                   ("every pointer at phase 8", [8] * P, [8] * P))
    elif kernel == "team_uniform":      # long double: the byte-pair form
        sp, dp = [0] * P, [0] * P
        sp[P - 1], dp[0] = 8, 8
        out.append((f"source {P - 1} at phase 8", sp, [0] * P))
        out.append(("target 0 at phase 8", [0] * P, dp))
    return out


class RawBatch(D.LauncherBatch):
    """Every case of one (kernel, type): all ops in one arena.  Expected values
    are computed once per (op, P) at the longest length and sliced."""

    def __init__(self, kernel, t):
        super().__init__(t)
        self.kernel = kernel
        self.pool = {}
        self.full = {}

    def add_op(self, op):
        t, kernel = self.t, self.kernel
        for P in X.MEMBERS:
            ns = [X.n_small(t), X.n_tile(kernel, t, P)]
            self.pool[op, P] = X.matrix_inputs(t, op, P, max(ns), 0x3A7 + P)
            for n in ns:
                for what, sph, dph in placements(kernel, t, P):
                    for ex in ((0, 1) if kernel == "team_scan" else (None,)):
                        srcs = [self.arena.add(n * self.s, sph[p], self.pool[op, P][p][:n])
                                for p in range(P)]
                        dsts = [self.arena.add(n * self.s, ph) for ph in dph]
                        self.case(srcs, dsts, what, kernel=kernel, op=op, P=P, n=n, exclusive=ex)

    def call(self, c, sp):
        d, s = D.ptrs(c.dsts), D.ptrs(c.srcs)
        if self.kernel == "combine_shifted":
            osgpu.combine_shifted(self.t, c.op, d[0], s, c.n, stream=sp)
        elif self.kernel == "team_scan":
            osgpu.team_scan(self.t, c.op, c.exclusive, d, s, c.n, stream=sp)
        else:
            osgpu.team_uniform(self.t, c.op, d, s, c.n, stream=sp)

    def want(self, c, q):
        key = (c.op, c.P)
        if key not in self.full:
            fold = {"combine_shifted": C.fold_left, "team_scan": S.inclusive,
                    "team_uniform": U.value}[self.kernel]
            self.full[key] = fold(self.t, c.op, self.pool[key])
        full = self.full[key]
        if self.kernel != "team_scan":
            return full[:c.n]
        if c.exclusive and q == 0:
            return np.repeat(S.identity(self.t, c.op), c.n)
        return full[q - c.exclusive][:c.n]


RAW = [(k, t) for k in X.RAW_KERNELS for t in X.RAW_TYPES[k]]


@pytest.mark.parametrize("kernel,t", RAW, ids=[f"{k}-{t}" for k, t in RAW])
def test_raw_launcher_every_op(torch_cuda, kernel, t):
    b = RawBatch(kernel, t)
    for op in X.ops_of(t):
        b.add_op(op)
    b.launch(torch_cuda).check()


def test_team_scan_keeps_refusing_long_double(torch_cuda):
    a = G.Arena()
    bufs = [a.add(64) for _ in range(4)]
    a.upload(torch_cuda)
    d, s = [g.ptr for g in bufs[:2]], [g.ptr for g in bufs[2:]]
    for op in X.ops_of("longdouble"):
        for ex in (0, 1):
            assert osgpu.team_scan("longdouble", op, ex, d, s, 4, check=False) == -5  # OSGPU_ENOTSUP
    torch_cuda.cuda.synchronize()
    a.download()
    for g in bufs:
        g.assert_unchanged("a refused call")


# ------------------------------------------- b. every door by every path
PATHS = ("device auto", "device pull", "host fold", "host getmem")


def _team_for(path, npes=X.NPES):
    """The cached team of the path's heap kind, the library set to the path;
    the path osgpu_last_path() must name (None: the case's team path)."""
    L = osgpu.load()
    if path.startswith("device"):
        tm = X.team(True, npes=npes)
        assert L.osgpu_set_path(osgpu.PATH_PULL if path == "device pull" else osgpu.PATH_AUTO) == 0
        return tm, ("pull" if path == "device pull" else None)
    tm = X.team(False, host_fold=(path == "host fold"), npes=npes)
    if path == "host getmem":
        assert L.osgpu_set_host_path(osgpu.HOST_GETMEM) == 0
        assert L.osgpu_set_host_chunk_bytes(2048) == 0
        return tm, "getmem"
    return tm, "host_fold"


def _restore():
    L = osgpu.load()
    L.osgpu_set_path(osgpu.PATH_AUTO)
    L.osgpu_set_host_path(-1)
    L.osgpu_set_host_chunk_bytes(-1)
    L.osgpu_set_host_fold_max_bytes(-1)


def run_case(case, paths=PATHS, npes=X.NPES):
    """`case` by every path of `paths`: each member's targets equal the oracle
    bit for bit; every path leaves the same bytes; the path taken; every byte
    outside the targets -- the sources, the bytes round each target, the whole
    heap of a PE outside the set -- unchanged; pSync back at 0
    (Team._on_members); long double padding zero."""
    what = f"{case.door} {case.t} {case.op} n={case.n}" + (" no index sources" if case.null else "")
    mask = case.target_mask()
    first = {}
    try:
        for path in paths:
            tm, ran = _team_for(path, npes)
            ran = case.team_path() if ran is None else ran
            for pe in range(npes):
                tm.fill(pe, 0, case.bytes, 0xC3)
                for off, arr in case.writes[pe]:
                    tm.write(pe, off, arr)
            before = {pe: tm.read(pe, 0, case.bytes) for pe in range(npes)}
            X.run_door(tm, case)
            _restore()
            for pe in range(npes):
                w = f"{what} [{path}] PE {pe}"
                after = tm.read(pe, 0, case.bytes)
                if pe not in case.members:
                    assert np.array_equal(after, before[pe]), f"{w}: not a member, yet written"
                    continue
                for off, want, tt in case.wants[pe]:
                    got = after[off:off + len(want) * X.esize(tt)]
                    view = got.view(np.longdouble if tt == "longdouble" else X.dtype(tt))
                    bad = X.same_bits(tt, view, want)
                    assert bad is None, f"{w}: element {bad} at offset {off} differs from the oracle"
                    if tt == "longdouble":
                        assert not got.reshape(-1, 16)[:, 10:].any(), f"{w}: long double padding"
                d = G.first_diff(after[~mask], before[pe][~mask])
                assert d is None, f"{w}: a byte outside the targets was written"
                assert tm.last_paths[pe] == ran, (w, tm.last_paths)
                if pe in first:
                    assert np.array_equal(after[mask], first[pe]), \
                        f"{w}: not the bytes of [{paths[0]}]"
                else:
                    first[pe] = after[mask].copy()
    finally:
        _restore()


def door_case(door, t, op, null=False):
    n = X.n_collective(door, t)
    lens = [X.n_small(t), 0, n] if door == "many" else None
    return X.DoorCase(door, t, op, n, 0x10C + X.esize(t), null=null, lens=lens)


DOOR = [(d, t) for d in X.DOORS for t in X.door_types(d)]


@pytest.mark.parametrize("door,t", DOOR, ids=[f"{d}-{t}" for d, t in DOOR])
def test_door_every_op_every_path(torch_cuda, door, t):
    for op in X.ops_of(t):
        if door == "loc" and op not in ("max", "min"):
            continue
        run_case(door_case(door, t, op))
        if door == "loc" and op == "max":      # once per type without index sources
            run_case(door_case(door, t, op, null=True))


# ------------------------------------------------------ c. eight members
@pytest.mark.parametrize("t,op", X.P8_PAIRS, ids=lambda x: x)
def test_eight_members_heaviest_instantiations(torch_cuda, t, op):
    for door in ("scan_inc", "scan_exc", "uniform"):
        n = X.n_tile(X._DOOR_KERNEL[door], t, 8)
        case = X.DoorCase(door, t, op, n, 0x3A7 + 8, npes=8, start=0, log=0, size=8)
        run_case(case, paths=("device auto",), npes=8)
