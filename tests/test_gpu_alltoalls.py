"""GPU parity of the strided all-to-all (shmem_alltoalls32/64) against the
numpy restatement of the OpenSHMEM 1.4 definition (tests/support/
alltoalls_ref.py), called through the C ABI by threads-as-PEs, and of the raw
strided launcher (osgpu_copy_strided) against numpy slicing.

Device heaps take the COPY path (copy.hip's strided kernel over peer
pointers), host heaps GETMEM under every host-path setting.  Every byte of
every member's target region is compared: the strided elements, the gaps
between them (filled with random bytes before the call) and 256-byte margins
on both sides; pSync must come back at SHMEM_SYNC_VALUE (checked by Team).
The fatal argument errors (dst < 1, sst < 1) need no GPU:
tests/test_alltoalls_ref.py checks them in a child process."""
import os
import re

import numpy as np
import pytest

import osgpu
from support import alltoalls_ref as AR
from support import team as T

pytestmark = pytest.mark.gpu

MARGIN = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shipped_shape():
    """(threads per workgroup, U per form) the strided kernel ships with,
    read from csrc/copy.hip."""
    src = open(os.path.join(ROOT, "test-resilient-osss-ucx_amd", "csrc", "copy.hip")).read()
    threads = int(re.search(r"constexpr int kThreads = (\d+);", src).group(1))
    u = re.search(r"constexpr int kStridedU\[F_NFORMS\] = \{(\d+), (\d+), (\d+)\};", src)
    return threads, [int(x) for x in u.groups()]


THREADS, U = _shipped_shape()
# A workgroup tile is THREADS * U units: 16-byte vectors in the gather and
# scatter forms (4 elements of 32 bits, 2 of 64), elements when both sides are
# strided.  The largest tile in elements is the 32-bit vector forms', so
# three of those plus a ragged 77 spans at least three tiles of every form at
# both widths: 3 * 256 * 2 * 4 + 77 = 6221 with the shipped U = 2.
BIG = 3 * THREADS * max(U) * 4 + 77
SIZES = [1, 2, 7, 1000, 4099, BIG]
STRIDES = [(1, 2), (2, 1), (1, 3), (3, 1), (2, 3), (5, 2), (1, 17), (17, 1), (33, 33)]
SETS = [  # (npes, PE_start, logPE_stride, PE_size); the last: more than kMaxCopySegs pieces
    (1, 0, 0, 1), (2, 0, 0, 2), (8, 0, 0, 8), (8, 1, 1, 3), (6, 2, 0, 3), (12, 0, 0, 12),
]
ids_set = lambda s: "P%d_s%d_l%d_n%d" % s


def _call(tm, bits, tgt_off, src_off, dst, sst, nelems, setdef):
    _, start, log, size = setdef
    fn = osgpu.coll_strided(bits)
    members = AR.active_set(start, log, size)
    tm._on_members(members, lambda pe: fn(tm.ptr(pe, tgt_off), tm.ptr(pe, src_off), dst, sst,
                                          nelems, start, log, size, tm.psync_ptr(pe)))
    return members


def _run_case(device, bits, setdef, dst, sst, nelems, seed=1, src_phase=0, tgt_phase=0,
              want_path="copy"):
    """One call on a fresh team: random sources, a random target region
    (margins and gaps included), every byte compared afterwards."""
    npes, start, log, size = setdef
    esz = bits // 8
    sb = AR.extent_bytes(size, nelems, sst, esz)
    tb = AR.extent_bytes(size, nelems, dst, esz)
    src_off = src_phase
    tgt_off = T._align(src_off + sb + MARGIN) + MARGIN + tgt_phase
    tm = T.Team(npes, tgt_off + tb + MARGIN, device=device)
    src, tgt = {}, {}
    for pe in range(npes):
        rng = np.random.default_rng(seed * 131 + pe)
        src[pe] = rng.integers(0, 256, sb, dtype=np.uint8)
        tgt[pe] = rng.integers(0, 256, tb + 2 * MARGIN, dtype=np.uint8)
        tm.write(pe, src_off, src[pe])
        tm.write(pe, tgt_off - MARGIN, tgt[pe])
    inner = {pe: t[MARGIN:] for pe, t in tgt.items()}
    out = AR.alltoalls_fast(src, inner, esz, dst, sst, nelems, start, log, size)
    members = _call(tm, bits, tgt_off, src_off, dst, sst, nelems, setdef)
    assert set(tm.last_coll_paths.values()) == {want_path}, tm.last_coll_paths
    for pe in range(npes):
        want = tgt[pe].copy()
        if pe in members:
            want[MARGIN:] = out[pe]
        got = tm.read(pe, tgt_off - MARGIN, want.size)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (pe, dst, sst, nelems, bad[:8], got[bad[:8]], want[bad[:8]])
    return tm


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("strides", STRIDES, ids=lambda s: "d%d_s%d" % s)
def test_three_pes_every_stride_and_size(bits, strides):
    for nelems in SIZES:
        _run_case(True, bits, (3, 0, 0, 3), strides[0], strides[1], nelems, seed=nelems + bits)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("setdef", SETS, ids=ids_set)
def test_other_sets_reduced_strides(bits, setdef):
    """One stride pair per form; P = 12 has more pieces than one launch
    takes (kMaxCopySegs = 8), so the pieces go out in two batches."""
    for dst, sst in ((1, 3), (17, 1), (2, 3)):
        for nelems in SIZES:
            _run_case(True, bits, setdef, dst, sst, nelems, seed=nelems + bits + dst)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("setdef", [(3, 0, 0, 3), (8, 1, 1, 3)], ids=ids_set)
def test_unit_strides_delegate_to_alltoall(bits, setdef):
    """dst = sst = 1 is shmem_alltoall: same bytes, same path, at a size of
    the one-launch form and at one past the fused limit."""
    npes, start, log, size = setdef
    esz = bits // 8
    for nelems in (1000, (1 << 20) // esz // size + 5):
        nb = nelems * esz * size
        tgt_off = T._align(nb + MARGIN) + MARGIN
        results = []
        for strided in (False, True):
            tm = T.Team(npes, tgt_off + nb + MARGIN, device=True)
            for pe in range(npes):
                rng = np.random.default_rng(7 * nelems + pe)
                tm.write(pe, 0, rng.integers(0, 256, nb, dtype=np.uint8))
                tm.write(pe, tgt_off - MARGIN, rng.integers(0, 256, nb + 2 * MARGIN, dtype=np.uint8))
            if strided:
                _call(tm, bits, tgt_off, 0, 1, 1, nelems, setdef)
            else:
                tm.run_coll("alltoall", bits, tgt_off, 0, nelems, PE_start=start,
                            logPE_stride=log, PE_size=size)
            results.append((dict(tm.last_coll_paths),
                            [tm.read(pe, tgt_off - MARGIN, nb + 2 * MARGIN) for pe in range(npes)]))
        (p0, r0), (p1, r1) = results
        assert p0 == p1 and set(p1.values()) <= {"copy", "fused_copy"}, (p0, p1)
        for a, b in zip(r0, r1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("phase", [4, 8, 12])
def test_dword_phases_of_the_contiguous_side(phase):
    """32-bit gather (target contiguous) and scatter (source contiguous)
    with the contiguous side 4, 8 and 12 bytes past a 16-byte boundary: the
    elements before the first and after the last whole vector."""
    for nelems in (1, 2, 3, 5, 1000, 4099):
        _run_case(True, 32, (3, 0, 0, 3), 1, 3, nelems, seed=phase + nelems, tgt_phase=phase)
        _run_case(True, 32, (3, 0, 0, 3), 3, 1, nelems, seed=phase + nelems, src_phase=phase)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_source_is_target(bits, device):
    """source and target are the SAME symmetric object: every peer must
    read its pre-call bytes."""
    esz, P = bits // 8, 3
    for dst, sst, nelems in ((2, 3, 1001), (3, 1, 1001), (1, 2, 77), (2, 2, 4099)):
        span = max(AR.extent_bytes(P, nelems, sst, esz), AR.extent_bytes(P, nelems, dst, esz))
        tm = T.Team(P, MARGIN + span + MARGIN, device=device)
        obj = {}
        for pe in range(P):
            obj[pe] = np.random.default_rng(nelems + pe).integers(0, 256, span + 2 * MARGIN,
                                                                  dtype=np.uint8)
            tm.write(pe, 0, obj[pe])
        inner = {pe: o[MARGIN:] for pe, o in obj.items()}
        out = AR.alltoalls_fast(inner, inner, esz, dst, sst, nelems, 0, 0, P)
        with osgpu.host_path("getmem"):
            _call(tm, bits, MARGIN, MARGIN, dst, sst, nelems, (P, 0, 0, P))
        assert set(tm.last_coll_paths.values()) == {"copy" if device else "getmem"}
        for pe in range(P):
            want = obj[pe].copy()
            want[MARGIN:] = out[pe]
            assert np.array_equal(tm.read(pe, 0, want.size), want), (pe, dst, sst)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_interleaved_source_and_target(bits, device):
    """One array per PE: the target is its even elements, the source its
    odd elements, dst = sst = 2.  The spans overlap though no element is
    shared; peers must see pre-call bytes and the odd elements stay."""
    esz, P = bits // 8, 3
    for nelems in (1, 7, 2049):
        span = AR.extent_bytes(P, nelems, 2, esz) + esz    # target span + the last odd element
        tm = T.Team(P, MARGIN + span + MARGIN, device=device)
        obj = {}
        for pe in range(P):
            obj[pe] = np.random.default_rng(nelems * 3 + pe).integers(0, 256, span + 2 * MARGIN,
                                                                      dtype=np.uint8)
            tm.write(pe, 0, obj[pe])
        srcs = {pe: o[MARGIN + esz:] for pe, o in obj.items()}
        tgts = {pe: o[MARGIN:] for pe, o in obj.items()}
        out = AR.alltoalls_fast(srcs, tgts, esz, 2, 2, nelems, 0, 0, P)
        with osgpu.host_path("getmem"):
            _call(tm, bits, MARGIN, MARGIN + esz, 2, 2, nelems, (P, 0, 0, P))
        assert set(tm.last_coll_paths.values()) == {"copy" if device else "getmem"}
        for pe in range(P):
            want = obj[pe].copy()
            want[MARGIN:] = out[pe]
            assert np.array_equal(tm.read(pe, 0, want.size), want), (pe, nelems)


@pytest.mark.parametrize("mode", ["getmem", "staged"])
def test_host_heaps_take_getmem(mode):
    """Host heaps: correct and on GETMEM under both settings (a strided
    call has no STAGED form); also with a chunk far below one block's span."""
    L = osgpu.load()
    with osgpu.host_path(mode):
        _run_case(False, 64, (3, 0, 0, 3), 2, 3, 3001, seed=11, want_path="getmem")
        assert L.osgpu_set_host_chunk_bytes(4096) == 0
        try:
            _run_case(False, 64, (3, 0, 0, 3), 2, 3, 3001, seed=12, want_path="getmem")
            _run_case(False, 32, (8, 1, 1, 3), 1, 17, 1000, seed=13, want_path="getmem")
        finally:
            L.osgpu_set_host_chunk_bytes(-1)


# ------------------------------------------------------------ raw launcher

def _strided_want(dst, src, esz, do, ds, so, ss, n):
    """numpy slicing: n elements of esz from byte so of src (ss apart) to
    byte do of dst (ds apart), in place on dst (uint8 arrays)."""
    dt = np.uint32 if esz == 4 else np.uint64
    d = dst[do:do + ((n - 1) * ds + 1) * esz].view(dt)
    s = src[so:so + ((n - 1) * ss + 1) * esz].view(dt)
    d[::ds] = s[::ss]


@pytest.mark.parametrize("esz", [4, 8])
def test_raw_launcher_matches_numpy_slicing(esz):
    """osgpu_copy_strided on one buffer: every stride pair at every size as
    separate segments (more than 8: several launches), sources and
    destinations at every dword phase; nothing outside the strided elements
    may change."""
    import torch
    rng = np.random.default_rng(esz)
    cases = [(ds, ss, n) for (ds, ss) in STRIDES for n in SIZES]
    sbytes = sum(((n - 1) * ss + 1) * esz + 64 for _, ss, n in cases) + 64
    dbytes = sum(((n - 1) * ds + 1) * esz + 64 for ds, _, n in cases) + 64
    src_h = rng.integers(0, 256, sbytes, dtype=np.uint8)
    dst_h = rng.integers(0, 256, dbytes, dtype=np.uint8)
    src = torch.from_numpy(src_h).cuda()
    dst = torch.from_numpy(dst_h).cuda()
    want = dst_h.copy()
    a = dict(dsts=[], dst_strides=[], srcs=[], src_strides=[], nelems=[])
    so = do = 16
    for i, (ds, ss, n) in enumerate(cases):
        sp, dp = so + esz * (i % (16 // esz)), do + esz * ((i // 3) % (16 // esz))
        _strided_want(want, src_h, esz, dp, ds, sp, ss, n)
        a["dsts"].append(dst.data_ptr() + dp)
        a["srcs"].append(src.data_ptr() + sp)
        a["dst_strides"].append(ds)
        a["src_strides"].append(ss)
        a["nelems"].append(n)
        so += (((n - 1) * ss + 1) * esz + 64) // 16 * 16
        do += (((n - 1) * ds + 1) * esz + 64) // 16 * 16
    torch.cuda.synchronize()
    osgpu.copy_strided(esz, **a)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("u", [2, 4, 8])
@pytest.mark.parametrize("nt", [0, 1])
def test_every_compiled_shape_moves_the_same_bytes(monkeypatch, u, nt):
    """The shapes tools/strided_rate.py compares (U in flight per lane x
    plain / non-temporal strided side, chosen through a test hook) are all
    in the library: each must copy exactly what the shipped one does, at a
    size of three tiles of its own and a ragged remainder."""
    import ctypes
    import torch
    monkeypatch.setenv("OSGPU_TEST_HOOKS", "1")
    L = osgpu.load()
    L.osgpu_test_strided_shape.argtypes = [ctypes.c_int] * 3
    assert L.osgpu_test_strided_shape(-1, u, nt) == 0, L.osgpu_last_error()
    try:
        for esz in (4, 8):
            n = 3 * THREADS * u * (16 // esz) + 77
            rng = np.random.default_rng(u * 2 + nt)
            src_h = rng.integers(0, 256, n * 3 * esz + 64, dtype=np.uint8)
            for ds, ss in ((1, 3), (3, 1), (2, 3)):
                dst_h = rng.integers(0, 256, n * 3 * esz + 64, dtype=np.uint8)
                src, dst = torch.from_numpy(src_h).cuda(), torch.from_numpy(dst_h).cuda()
                want = dst_h.copy()
                _strided_want(want, src_h, esz, 16 + esz, ds, 16, ss, n)
                torch.cuda.synchronize()
                osgpu.copy_strided(esz, [dst.data_ptr() + 16 + esz], [ds], [src.data_ptr() + 16],
                                   [ss], [n])
                torch.cuda.synchronize()
                assert np.array_equal(dst.cpu().numpy(), want), (esz, ds, ss)
    finally:
        assert L.osgpu_test_strided_shape(-1, 0, 0) == 0


def test_raw_launcher_refuses_bad_arguments():
    import torch
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    EINVAL = -1
    ok = dict(dsts=[p], dst_strides=[2], srcs=[p + 512], src_strides=[1], nelems=[8])
    assert osgpu.copy_strided(4, check=False, **ok) == 0
    assert osgpu.copy_strided(8, check=False, **ok) == 0
    for eb in (0, 1, 2, 16):
        assert osgpu.copy_strided(eb, check=False, **ok) == EINVAL
    for key, val in (("dst_strides", [0]), ("src_strides", [0]), ("dst_strides", [-1]),
                     ("src_strides", [-3])):
        assert osgpu.copy_strided(4, check=False, **dict(ok, **{key: val})) == EINVAL
    assert osgpu.copy_strided(4, check=False, **dict(ok, dsts=[p + 2])) == EINVAL
    assert osgpu.copy_strided(8, check=False, **dict(ok, srcs=[p + 512 + 4])) == EINVAL
    assert osgpu.copy_strided(4, check=False, **dict(ok, srcs=[p + 512 + 4])) == 0
    assert b"osgpu_copy_strided" in osgpu.load().osgpu_last_error()
    torch.cuda.synchronize()
    assert not buf.any()


def test_offsets_past_4gib():
    """64-bit elements, nelems = 3, a stride of 2^28 + 1 elements: the byte
    offset of element 2 is 2 * (2^28 + 1) * 8 > 2^32.  Gather (contiguous
    target) and the mirror scatter, on one allocation of just over 4 GiB
    that is never filled: only the three elements are written and read."""
    import torch
    stride = 2 ** 28 + 1
    far = 2 * stride * 8
    assert far > 2 ** 32
    try:
        big = torch.empty(far + 8 + 256, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:
        pytest.skip(f"no {far >> 20} MiB allocation: {e}")
    small = torch.zeros(64, dtype=torch.int64, device="cuda")
    vals = [0x1111111122222222, 0x3333333344444444, 0x5555555566666666]
    words = big.view(torch.int64)
    for k, v in enumerate(vals):
        words[k * stride] = v
    torch.cuda.synchronize()
    osgpu.copy_strided(8, [small.data_ptr() + 8], [1], [big.data_ptr()], [stride], [3])
    torch.cuda.synchronize()
    assert small.tolist()[:5] == [0] + vals + [0]
    for k in range(3):
        words[k * stride] = 0
    torch.cuda.synchronize()
    osgpu.copy_strided(8, [big.data_ptr()], [stride], [small.data_ptr() + 8], [1], [3])
    torch.cuda.synchronize()
    assert [int(words[k * stride]) for k in range(3)] == vals
