"""half / bfloat16 reduce-to-all on the GPU, bit-compared to the numpy
restatement (tests/support/half_ref.py): the device arithmetic exhaustively,
every combine and team kernel form at its smallest shapes, the NaN tile
recompute, and every path of the entry points with its path code.
"""
import ctypes

import numpy as np
import pytest

import osgpu
from support import half_ref as R
from support.gpu_doors import stream, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PAIRS = [(t, o) for t in R.TYPES for o in R.OPS]


def _dev(torch, arr, pad=64):
    """arr's bytes on the GPU with `pad` spare bytes in front and behind."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = np.full(raw.size + 2 * pad, 0x5A, np.uint8)
    buf[pad:pad + raw.size] = raw
    return torch.from_numpy(buf).to("cuda:0")


def _host(torch, buf, off, n):
    torch.cuda.synchronize()
    return buf[off:off + 2 * n].cpu().numpy().view(np.uint16).copy()


def _mismatch(got, want):
    bad = np.flatnonzero(got != want)
    return (f"{bad.size} of {want.size} differ; first at {bad[0]}: got "
            f"{got[bad[0]]:#06x} want {want[bad[0]]:#06x}") if bad.size else ""


# ----------------------------------------------------- exhaustive arithmetic

_EX = {}


def _exhaustive_inputs(t):
    """a = all 65536 patterns x b = 128 table patterns: 8 Mi elements."""
    if t not in _EX:
        tb = R.special_table(t, 128)
        a = np.tile(np.arange(65536, dtype=np.uint32).astype(np.uint16), tb.size)
        b = np.repeat(tb, 65536)
        _EX[t] = (a, b, {})
    return _EX[t]


@pytest.mark.parametrize("t,op", PAIRS)
def test_exhaustive_device_arithmetic(torch_cuda, t, op):
    """One launch of the 2-input combine over every first operand x 128
    second operands (the vector form: the packed / f32-routed fast fold, and
    the exact fold of every vector with a NaN), and one of the
    element-granular kernel (the exact fold alone) on the same data."""
    torch = torch_cuda
    a, b, cache = _exhaustive_inputs(t)
    if op not in cache:
        cache[op] = R.op2(t, op, a, b)
    want = cache[op]
    da, db = _dev(torch, a), _dev(torch, b)
    out = torch.zeros(a.size * 2 + 128, dtype=torch.uint8, device="cuda:0")
    osgpu.combine(t, op, out.data_ptr() + 64, [da.data_ptr() + 64, db.data_ptr() + 64], a.size,
                  stream(torch))
    msg = _mismatch(_host(torch, out, 64, a.size), want)
    assert not msg, f"vector form {t} {op}: {msg}"
    out.zero_()
    # b at another 16-byte phase: the element-granular kernel
    db2 = _dev(torch, b, pad=66)
    osgpu.combine(t, op, out.data_ptr() + 64, [da.data_ptr() + 64, db2.data_ptr() + 66], a.size,
                  stream(torch))
    msg = _mismatch(_host(torch, out, 64, a.size), want)
    assert not msg, f"element-granular form {t} {op}: {msg}"


# ------------------------------------------------------------ combine shapes

_values = R.order_values


NS = [0, 1, 7, 8, 9, 15]


def _combine_ns(K):
    # elements of one tile (combine.hip): K = 1 runs combine_vec_kernel (256
    # lanes x 4 vectors), K >= 2 the LDS form (64 x U vectors)
    tile = (256 * 4 if K == 1 else 64 * (2 if K == 2 else 4)) * 8
    return NS + [tile - 1, tile, tile + 1, tile * 3 + 5]


@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_combine_shapes(torch_cuda, t, K):
    """Every n and base offset for sum and max; target aliasing source 0;
    one source at another 16-byte phase."""
    torch = torch_cuda
    nmax = max(_combine_ns(K))
    src = [_values(t, nmax, 100 * K + k) for k in range(K)]
    dev = [_dev(torch, s) for s in src]
    dev_odd = _dev(torch, src[-1], pad=72)  # 8 bytes off the others' phase
    out = torch.zeros(nmax * 2 + 128, dtype=torch.uint8, device="cuda:0")
    for op in ("sum", "max"):
        for n in _combine_ns(K):
            for off in (0, 2, 6, 14):  # bytes, shared by every array: head / tail lanes
                o2 = off // 2
                m = min(n, nmax - o2)
                want = R.fold(t, op, list(range(K)), [s[o2:o2 + m] for s in src])
                out.fill_(0xA5)
                osgpu.combine(t, op, out.data_ptr() + 64 + off,
                              [d.data_ptr() + 64 + off for d in dev], m, stream(torch))
                got = _host(torch, out, 64 + off, m)
                assert not _mismatch(got, want), (t, op, K, n, off, _mismatch(got, want))
                raw = out.cpu().numpy()
                assert (raw[:64 + off] == 0xA5).all() and (raw[64 + off + 2 * m:] == 0xA5).all()
            if K >= 2 and n:
                want = R.fold(t, op, list(range(K)), [s[:n] for s in src])
                out.fill_(0)
                ptrs = [d.data_ptr() + 64 for d in dev[:-1]] + [dev_odd.data_ptr() + 72]
                osgpu.combine(t, op, out.data_ptr() + 64, ptrs, n, stream(torch))
                got = _host(torch, out, 64, n)
                assert not _mismatch(got, want), (t, op, K, n, "phase", _mismatch(got, want))
    # target aliasing source 0
    n = _combine_ns(K)[-1]
    d0 = _dev(torch, src[0])
    osgpu.combine(t, "sum", d0.data_ptr() + 64, [d0.data_ptr() + 64] + [d.data_ptr() + 64 for d in dev[1:]],
                  n, stream(torch))
    want = R.fold(t, "sum", list(range(K)), [s[:n] for s in src])
    got = _host(torch, d0, 64, n)
    assert not _mismatch(got, want), (t, K, "alias", _mismatch(got, want))


@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_nan_tile_recompute(torch_cuda, t, op):
    """One NaN-producing pair in exactly one vector of a multi-tile call and
    one in an edge element: the NaN is the exact one, the rest unchanged."""
    torch = torch_cuda
    inf, ninf, zero = (0x7C00, 0xFC00, 0x0000) if t == "half" else (0x7F80, 0xFF80, 0x0000)
    n = 128 * 8 * 3 + 5
    a, b = _values(t, n, 7), _values(t, n, 8)
    fin = (0x3C00 if t == "half" else 0x3F80)
    a = np.where((a & 0x7FFF) >= (0x7800 if t == "half" else 0x7F00), fin, a).astype(np.uint16)
    b = np.where((b & 0x7FFF) >= (0x7800 if t == "half" else 0x7F00), fin, b).astype(np.uint16)
    base = R.op2(t, op, a, b)
    assert not R.isnan(t, base).any()
    x, y = (inf, ninf) if op == "sum" else (zero, inf)
    for i in (128 * 8 + 19, n - 2):  # inside the second tile; in the tail
        a[i], b[i] = x, y
    want = R.op2(t, op, a, b)
    nan = np.flatnonzero(R.isnan(t, want))
    assert list(nan) == [128 * 8 + 19, n - 2]
    assert all(want[i] == R.DEFNAN[t] for i in nan)
    da, db = _dev(torch, a), _dev(torch, b)
    out = torch.zeros(n * 2 + 128, dtype=torch.uint8, device="cuda:0")
    osgpu.combine(t, op, out.data_ptr() + 64, [da.data_ptr() + 64, db.data_ptr() + 64], n,
                  stream(torch))
    got = _host(torch, out, 64, n)
    assert not _mismatch(got, want), _mismatch(got, want)
    keep = np.ones(n, bool)
    keep[nan] = False
    assert np.array_equal(got[keep], base[keep])


# ---------------------------------------------------------------------- team

@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("P", [2, 3, 5, 7, 8])
def test_team_kernel(torch_cuda, t, P):
    """osgpu_team_combine_shape, local and remote shapes: every member's
    target in its own fold order; head, whole vectors (more than one tile)
    and tail."""
    torch = torch_cuda
    # 3 head elements (base offset 10 bytes), one tile of the register form
    # (256 * 4 vectors) and of the LDS form (64) + 5 vectors, 6 tail elements
    n = 3 + 8 * (1024 + 64 + 5) + 6
    src = [_values(t, n, 300 + p) for p in range(P)]
    # where the order shows in the last bit: the last member holds 1, the
    # others half-ulp terms ((t + t) + 1 against (1 + t) + t); and, for two
    # members (a + b = b + a), two NaNs whose payloads tell the first operand
    one, tie = (0x3C00, 0x1000) if t == "half" else (0x3F80, 0x3B80)
    for p in range(P):
        src[p][:64] = one if p == P - 1 else tie
    src[0][64:72], src[1][64:72] = (0x7C01, 0xFE02) if t == "half" else (0x7F81, 0xFFC2)
    for op in ("sum", "max", "prod", "min"):
        want = R.to_all(t, op, src)
        if op == "sum":
            assert any(not np.array_equal(want[0], w) for w in want[1:]), \
                "the inputs must make the fold orders differ"
        for remote in (False, True):
            ins = [_dev(torch, s, pad=74) for s in src]
            outs = [torch.zeros(n * 2 + 160, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
            osgpu.team_combine(t, op, [o.data_ptr() + 74 for o in outs],
                               [i.data_ptr() + 74 for i in ins], n, stream(torch), remote=remote)
            for q in range(P):
                got = _host(torch, outs[q], 74, n)
                assert not _mismatch(got, want[q]), (t, op, P, remote, q, _mismatch(got, want[q]))


# -------------------------------------------------------------- entry points

_TEAMS = {}


def _team(device):
    from support import team as T
    if device not in _TEAMS:
        _TEAMS[device] = T.Team(4, 1 << 20, device=device)
    tm = _TEAMS[device]
    tm.activate()
    return tm


def _run(tm, t, op, toff, soff, n, PE_start=0, logPE_stride=0, PE_size=None, ext=False):
    PE_size = tm.npes if PE_size is None else PE_size
    members = [PE_start + (i << logPE_stride) for i in range(PE_size)]
    pwrk = (ctypes.c_byte * 4096)()
    if ext:
        fn = tm.lib.osgpu_reduce_ext
        call = lambda pe: fn(osgpu.type_code(t), osgpu.OPS.index(op), tm.ptr(pe, toff),
                             tm.ptr(pe, soff), n, PE_start, logPE_stride, PE_size,
                             ctypes.addressof(pwrk), tm.psync_ptr(pe))
    else:
        fn = osgpu.ext_reduce(t, op)
        call = lambda pe: fn(tm.ptr(pe, toff), tm.ptr(pe, soff), n, PE_start, logPE_stride,
                             PE_size, ctypes.addressof(pwrk), tm.psync_ptr(pe))
    tm._on_members(members, call)
    return members


def _check_call(tm, t, op, n, want_path, PE_start=0, logPE_stride=0, PE_size=None, in_place=False,
                ext=False, seed=0):
    src = [_values(t, max(n, 1), 500 + seed + pe) for pe in range(tm.npes)]
    toff = 0 if in_place else 1 << 19
    for pe in range(tm.npes):
        tm.write(pe, 0, src[pe])
        if not in_place:
            tm.fill(pe, toff, 2 * max(n, 8), 0xA5)
    members = _run(tm, t, op, toff, 0, n, PE_start, logPE_stride, PE_size, ext)
    assert all(tm.last_paths[pe] == want_path for pe in members), (tm.last_paths, want_path)
    msrc = [src[pe][:n] for pe in members]
    want = R.to_all(t, op, msrc)
    for i, pe in enumerate(members):
        got = tm.read(pe, toff, 2 * n).view(np.uint16)
        assert not _mismatch(got, want[i]), (t, op, n, want_path, pe, _mismatch(got, want[i]))
    for pe in range(tm.npes):
        if pe not in members and not in_place:
            assert (tm.read(pe, toff, 2 * max(n, 8)) == 0xA5).all()


N_EP = 8 * 700 + 3


@pytest.mark.parametrize("t,op", PAIRS)
def test_entry_points_device_team(torch_cuda, t, op):
    tm = _team(True)
    _check_call(tm, t, op, N_EP, "team")
    _check_call(tm, t, op, N_EP, "team", PE_start=1, logPE_stride=0, PE_size=3, ext=True)
    _check_call(tm, t, op, 1000, "team", PE_start=0, logPE_stride=1, PE_size=2)


@pytest.mark.parametrize("t", R.TYPES)
def test_entry_points_device_other_paths(torch_cuda, t):
    tm = _team(True)
    L = tm.lib
    for op in ("sum", "min"):
        # overlap (target == source) cannot take the team form: pull
        _check_call(tm, t, op, N_EP, "pull", in_place=True)
        _check_call(tm, t, op, 0, "barrier_only")
        _check_call(tm, t, op, 77, "pull", PE_start=2, PE_size=1)
        L.osgpu_set_path(osgpu.PATH_PULL)
        try:
            _check_call(tm, t, op, N_EP, "pull")
            _check_call(tm, t, op, 1001, "pull", PE_start=1, PE_size=3)
        finally:
            L.osgpu_set_path(osgpu.PATH_AUTO)
        # forced RCCL (no communicator, and no row for these types): the exact kernels
        L.osgpu_set_path(osgpu.PATH_RCCL)
        try:
            _check_call(tm, t, op, N_EP, "team")
        finally:
            L.osgpu_set_path(osgpu.PATH_AUTO)
    L.osgpu_finalize()
    L.osgpu_set_stage_bytes(65536)
    L.osgpu_set_team_exchange(1)
    try:
        for op in ("sum", "max"):
            _check_call(tm, t, op, 40_000 + 5, "team_push")
            _check_call(tm, t, op, 999, "team_push", PE_start=0, logPE_stride=1, PE_size=2)
    finally:
        L.osgpu_set_team_exchange(-1)
        L.osgpu_finalize()
        L.osgpu_set_stage_bytes(-1)


@pytest.mark.parametrize("t", R.TYPES)
def test_entry_points_host_heaps(torch_cuda, t):
    tm = _team(False)
    for op in ("sum", "prod", "max"):
        tm.host_fold = True
        tm.activate()
        _check_call(tm, t, op, 1024, "host_fold")
        _check_call(tm, t, op, 1024, "host_fold", PE_start=1, PE_size=3, ext=True)
        tm.host_fold = False
        tm.activate()
        with osgpu.host_path("staged"):
            _check_call(tm, t, op, 65536, "staged")
        with osgpu.host_path("getmem"):
            _check_call(tm, t, op, 4099, "getmem")


def test_checksum_of_half_equals_short(torch_cuda):
    torch = torch_cuda
    v = _values("half", 100_003, 9)
    d = _dev(torch, v)
    torch.cuda.synchronize()
    for mode in (osgpu.CK_HASH, osgpu.CK_SUM, osgpu.CK_XOR):
        want = osgpu.checksum("short", mode, d.data_ptr() + 64, v.size)
        assert osgpu.checksum("half", mode, d.data_ptr() + 64, v.size) == want
        assert osgpu.checksum("bfloat16", mode, d.data_ptr() + 64, v.size) == want
