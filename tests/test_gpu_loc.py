"""Max / min with location on the GPU: osgpu_team_loc (team_loc_vec_kernel,
team_loc_scalar_kernel, csrc/team.hip) and osgpu_reduce_loc on device and host
heaps.

1. The raw launcher at tile edges: every pair, P in {1, 2, 3, 5, 8}, ndst in
   {1, P}, n in {0, 1, g-1, g, g+1, T-1, T, T+1, 2T+g+1} with g the kernel's
   group and T = 256 g its tile; every value and index array EXACTLY n
   elements between guard bands (tests/support/guarded.py); bit for bit.
2. Phases: all pointers one element on (a common head), one value source
   shifted alone, index pointers at +4 bytes, one value target shifted alone
   (the last three: the element-granular kernel).
3. The form without index sources: member numbers {1, 3, 5}, and 8 descending.
4. The value targets are osgpu_team_uniform's bytes (osgpu_compare on the GPU).
5. Multi-launch under osgpu_test_max_launch_threads.
6. The collective on device heaps (TEAM), P in {2, 3, 8}, n = 3 T + g + 1; the
   strided set (1, 1, 3) of 8 PEs without index sources.
7. The pull forms: OSGPU_PATH_PULL, in place, a target outside the heap,
   9 members, one member.
8. Host heaps: host fold, GETMEM with a small chunk, a forced STAGED.
9. Two processes on one GPU (tests/support/loc_mp_worker.py).
10. A seeded fuzz of 30 calls.

Expected values and indices: tests/support/loc_cases.py (the oracle's value,
the closed form's index; the inputs are checked there to tell a "first holder
wins" or "last holder wins" kernel from a right one).
"""
import ctypes
import os

import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import guarded as G
from support import loc_cases as C
from support.gpu_doors import small_launches, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


_POOL = {}


def nmax(t):
    return 3 * C.tile_elems(t) + C.group(t) + 1


def pool(t, op):
    """The tie inputs of 8 members at the longest length any test uses, and
    the expected (value, index) of their first P members: computed once."""
    if (t, op) not in _POOL:
        vals, locs = C.tie_case(t, op, 8, nmax(t), 0x10C + C.esize(t))
        for P in (3, 5):
            C.assert_discriminating(t, op, vals[:P], locs[:P])
        _POOL[(t, op)] = (vals, locs, {})
    return _POOL[(t, op)]


def want(t, op, P, n, member_locs=None):
    vals, locs, memo = pool(t, op)
    key = (P, None if member_locs is None else tuple(member_locs))
    if key not in memo:
        idx = locs[:P] if member_locs is None else C.const_indices(member_locs, nmax(t))
        memo[key] = C.expected(t, op, vals[:P], idx)
    v, i = memo[key]
    return v[:n], i[:n]


def lengths(t):
    g, T = C.group(t), C.tile_elems(t)
    return sorted({0, 1, g - 1, g, g + 1, T - 1, T, T + 1, 2 * T + g + 1})


class Batch(D.LauncherBatch):
    """Cases of one (type, op): a case's targets are its ndst value targets,
    then its ndst index targets; its sources the values, then the indices."""

    def __init__(self, t, op):
        super().__init__(t)
        self.op = op
        self.vals, self.locs, _ = pool(t, op)

    def add(self, P, ndst, n, what, vsp=None, lsp=None, vdp=None, ldp=None, member_locs=None):
        """vsp / lsp / vdp / ldp: the 16-byte phases of the value sources, index
        sources, value targets and index targets (default 0)."""
        ph = lambda a, k: 0 if a is None else a[k]
        vs = [self.arena.add(n * self.s, ph(vsp, p), self.vals[p][:n]) for p in range(P)]
        ls = [] if member_locs is not None else [
            self.arena.add(n * 4, ph(lsp, p), self.locs[p][:n]) for p in range(P)]
        vd = [self.arena.add(n * self.s, ph(vdp, q)) for q in range(ndst)]
        ld = [self.arena.add(n * 4, ph(ldp, q)) for q in range(ndst)]
        self.case(vs + ls, vd + ld, what, op=self.op, P=P, ndst=ndst, n=n, member_locs=member_locs)

    def call(self, c, sp):
        osgpu.team_loc(self.t, self.op, D.ptrs(c.dsts[:c.ndst]), D.ptrs(c.dsts[c.ndst:]),
                       D.ptrs(c.srcs[:c.P]), D.ptrs(c.srcs[c.P:]) or None, c.n,
                       member_locs=c.member_locs, stream=sp)

    def out_type(self, c, q):
        return self.t if q < c.ndst else "int"

    def want(self, c, q):
        return want(self.t, self.op, c.P, c.n, c.member_locs)[q >= c.ndst]


# ------------------------------------------------------------ 1. lengths
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_launcher_lengths(torch_cuda, t, op):
    b = Batch(t, op)
    for P in (1, 2, 3, 5, 8):
        for ndst in sorted({1, P}):
            for n in lengths(t):
                b.add(P, ndst, n, "aligned")
    b.launch(torch_cuda).check()


# ------------------------------------------------------------- 2. phases
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_launcher_phases(torch_cuda, t, op):
    s, g, T = C.esize(t), C.group(t), C.tile_elems(t)
    b = Batch(t, op)
    for P, ndst in ((2, 2), (3, 1), (8, 8)):
        for n in (g - 1, g + 1, T + 1, 2 * T + g + 1):
            # every pointer one element on: 16 - s and 12, one common head of g - 1 ... 1
            b.add(P, ndst, n, "all pointers shifted by one element",
                  vsp=[s % 16] * P, lsp=[4] * P, vdp=[s % 16] * ndst, ldp=[4] * ndst)
            one = [0] * P
            one[P - 1] = s
            b.add(P, ndst, n, f"value source {P - 1} shifted alone", vsp=one)
            b.add(P, ndst, n, "index pointers at +4 bytes", lsp=[4] * P, ldp=[4] * ndst)
            tgt = [0] * ndst
            tgt[ndst - 1] = s
            b.add(P, ndst, n, f"value target {ndst - 1} shifted alone", vdp=tgt)
    b.launch(torch_cuda).check()


# ------------------------------------------------- 3. no index sources
@pytest.mark.parametrize("t,op", [("short", "max"), ("float", "min"), ("double", "max"),
                                  ("bfloat16", "min"), ("long", "min"), ("int", "max")],
                         ids=lambda x: x)
def test_launcher_member_locs(torch_cuda, t, op):
    g, T = C.group(t), C.tile_elems(t)
    b = Batch(t, op)
    for n in (1, g + 1, T + 1, 2 * T + g + 1):
        for ndst in (1, 3):
            b.add(3, ndst, n, "member_locs 1 3 5", member_locs=[1, 3, 5])
            b.add(3, ndst, n, "member_locs 1 3 5, a head", member_locs=[1, 3, 5],
                  vsp=[C.esize(t)] * 3, vdp=[C.esize(t)] * ndst, ldp=[4] * ndst)
        for ndst in (1, 8):
            b.add(8, ndst, n, "descending member_locs", member_locs=list(range(17, 9, -1)))
    b.launch(torch_cuda).check()


def test_launcher_bad_arguments(torch_cuda):
    a = G.Arena()
    bufs = [a.add(64) for _ in range(36)]
    a.upload(torch_cuda)
    p = [g.ptr for g in bufs]
    vd, ld, vs, ls = p[:9], p[9:18], p[18:27], p[27:]
    bad = [("int", "sum", 2, 2, True), ("longdouble", "max", 2, 2, True),
           ("complexf", "max", 2, 2, True), ("int", "max", 9, 9, True), ("int", "max", 3, 2, True),
           ("int", "max", 2, 1, None)]
    for t, op, P, D, has in bad:
        rc = osgpu.team_loc(t, op, vd[:D], ld[:D], vs[:P], ls[:P] if has else None, 4, check=False)
        assert rc == -1, (t, op, P, D)          # OSGPU_EINVAL
    torch_cuda.cuda.synchronize()
    a.download()
    for g in bufs:
        g.assert_unchanged("a refused call")


# ------------------------------------------------------ 4. value identity
@pytest.mark.parametrize("t,op", [("float", "max"), ("bfloat16", "min")], ids=lambda x: x)
def test_values_are_the_uniform_reduce(torch_cuda, t, op):
    torch = torch_cuda
    P, n, s = 8, 2 * C.tile_elems(t) + C.group(t) + 1, C.esize(t)
    vals, locs, _ = pool(t, op)
    a = G.Arena()
    vs = [a.add(n * s, 0, vals[p][:n]) for p in range(P)]
    ls = [a.add(n * 4, 0, locs[p][:n]) for p in range(P)]
    vd, ld, ud = ([a.add(n * k) for _ in range(P)] for k in (s, 4, s))
    a.upload(torch)
    sp = D.stream(torch)
    osgpu.team_loc(t, op, [g.ptr for g in vd], [g.ptr for g in ld], [g.ptr for g in vs],
                   [g.ptr for g in ls], n, stream=sp)
    osgpu.team_uniform(t, op, [g.ptr for g in ud], [g.ptr for g in vs], n, stream=sp)
    torch.cuda.synchronize()
    for q in range(P):
        bad, first = osgpu.compare(vd[q].ptr, ud[q].ptr, n * s, stream=sp)
        assert bad == 0, f"{t} {op}: value target {q} differs from osgpu_team_uniform's at byte {first}"
    a.download()
    wv, wi = want(t, op, P, n)
    assert np.array_equal(ld[0].data().view(np.int32), wi)


# --------------------------------------------------------- 5. multi-launch
@pytest.mark.parametrize("t,op", [("half", "max"), ("int", "min"), ("double", "max")],
                         ids=lambda x: x)
def test_launcher_multi_launch(torch_cuda, small_launches, t, op):
    """3 tiles + a group + 1 under a limit of 512 threads (2 tiles) a launch:
    equal to the single launch and to the expected arrays; a common head adds
    the edges to the first launch."""
    s, g, T = C.esize(t), C.group(t), C.tile_elems(t)
    res = []
    for limit in (0, 512):
        small_launches(limit)
        b = Batch(t, op)
        for P, ndst in ((2, 2), (8, 1), (8, 8)):
            b.add(P, ndst, 3 * T + g + 1, f"limit {limit}")
            b.add(P, ndst, 3 * T + g + 1, f"limit {limit} edges", vsp=[s] * P, lsp=[4] * P,
                  vdp=[s] * ndst, ldp=[4] * ndst)
        b.add(3, 3, 3 * T + 1, f"limit {limit} member_locs", member_locs=[1, 3, 5])
        b.launch(torch_cuda).check()
        res.append([d.data().copy() for c in b.cases for d in c.dsts])
    for one, many in zip(*res):
        assert np.array_equal(one, many)


# ---------------------------------------------------- 6-8. the collective
def _layout(t, n, shift=0):
    """Offsets of source, index source, target, index target (each area 4 KiB
    aligned, the targets `shift` elements on) and the heap size."""
    s = C.esize(t)
    area = (n * max(s, 4) + 4095) // 4096 * 4096 + 4096
    return 0, area, 2 * area + shift * s, 3 * area + shift * 4, 4 * area + 4096


def _collective(t, op, npes, n, seed, PE_start=0, log=0, PE_size=None, path="team", null=False,
                shift=0, in_place=False, device=True, host_fold=False, outside=False, ref=None):
    """One call on a fresh team; checks every member's two results, the bytes
    round them, the path and (in Team._on_members) pSync.  Returns the bytes
    the first member received.  outside: the targets are device memory outside
    the registered heaps."""
    from support import team as T
    PE_size = npes if PE_size is None else PE_size
    s = C.esize(t)
    soff, lsoff, toff, ltoff, hb = _layout(t, n, shift)
    if in_place:
        toff, ltoff = soff, lsoff
    tm = T.Team(npes, hb, device=device, host_fold=host_fold)
    vals, locs = C.tie_values(t, npes, n, seed), C.tie_indices(npes, n, seed)
    for pe in range(npes):
        tm.fill(pe, 0, hb, 0xC3)
        tm.write(pe, soff, vals[pe])
        if not null:
            tm.write(pe, lsoff, locs[pe])
    before = {pe: tm.read(pe, 0, hb) for pe in range(npes)}
    members = C.member_pes(PE_start, log, PE_size)
    idx = C.const_indices(members, n) if null else [locs[pe] for pe in members]
    wv, wi = C.expected(t, op, [vals[pe] for pe in members], idx)
    what = f"{t} {op} P={PE_size} n={n} null={null}"
    if outside:
        import torch
        ext = torch.full((npes, 2, n * 8 + 64), 0xC3, dtype=torch.uint8, device="cuda:0")
        fn = tm.osgpu.reduce_loc(t, op)
        pwrk = (ctypes.c_byte * 4096)()
        tm._on_members(members, lambda pe: fn(
            ext[pe, 0].data_ptr(), ext[pe, 1].data_ptr(), tm.ptr(pe, soff),
            None if null else tm.ptr(pe, lsoff), n, PE_start, log, PE_size,
            ctypes.addressof(pwrk), tm.psync_ptr(pe)))
        torch.cuda.synchronize()
        back = ext.cpu().numpy()
    else:
        C.run(tm, t, op, toff, ltoff, soff, None if null else lsoff, n, PE_start, log, PE_size)
    first = None
    for pe in range(npes):
        after = tm.read(pe, 0, hb)
        if pe not in members:
            assert np.array_equal(after, before[pe]), f"{what}: PE {pe} is not a member"
            continue
        w = f"{what} PE {pe}"
        if outside:
            gv, gi = back[pe, 0][:n * s], back[pe, 1][:n * 4]
            assert (back[pe, 0][n * s:] == 0xC3).all() and (back[pe, 1][n * 4:] == 0xC3).all(), w
            assert np.array_equal(after, before[pe]), f"{w}: the heap changed"
        else:
            gv, gi = after[toff:toff + n * s], after[ltoff:ltoff + n * 4]
            mask = np.ones(hb, bool)
            mask[toff:toff + n * s] = False
            mask[ltoff:ltoff + n * 4] = False
            assert np.array_equal(after[mask], before[pe][mask]), f"{w}: bytes outside the targets"
        bad = C.same_bits(t, gv.view(C.dtype(t)), wv)
        assert bad is None, f"{w}: value {bad} differs"
        gi = gi.view(np.int32)
        assert np.array_equal(gi, wi), f"{w}: index {int(np.flatnonzero(gi != wi)[0])} differs"
        if path is not None:
            assert tm.last_paths[pe] == path, (w, tm.last_paths)
        first = (gv.copy(), gi.copy()) if first is None else first
    if ref is not None:
        assert np.array_equal(first[0], ref[0]) and np.array_equal(first[1], ref[1]), \
            f"{what}: not the bytes of the team result"
    return first


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, op, P):
    """Every shard has a partial tile and the last a tail."""
    n = 3 * C.tile_elems(t) + C.group(t) + 1
    _collective(t, op, P, n, 0xD0 + P)
    _collective(t, op, P, C.group(t) + 1, 0xD0 + P, null=True)


def test_collective_strided_set_without_index_sources(torch_cuda):
    for t, op in (("double", "max"), ("short", "min"), ("half", "max")):
        n = 3 * C.tile_elems(t) + C.group(t) + 1
        _collective(t, op, 8, n, 5, PE_start=1, log=1, PE_size=3, null=True)
        _collective(t, op, 8, 1001, 6, PE_start=1, log=1, PE_size=3)


def test_collective_target_sub_view(torch_cuda):
    """Targets an odd number of elements into their arrays: still one common
    head for 4-byte types, none for 2- and 8-byte ones."""
    for t, op in (("short", "min"), ("int", "max"), ("double", "min")):
        _collective(t, op, 3, 1001, 0xD3, shift=3)


def test_collective_pull_forms(torch_cuda):
    for t, op, n in (("float", "max", 1001), ("short", "min", 2 * C.tile_elems("short") + 3),
                     ("long", "max", 777)):
        ref = _collective(t, op, 3, n, 0xE0)
        nref = _collective(t, op, 3, n, 0xE0, null=True)
        with D.forced_path(osgpu.PATH_PULL):
            _collective(t, op, 3, n, 0xE0, path="pull", ref=ref)
            _collective(t, op, 3, n, 0xE0, path="pull", null=True, ref=nref)
        _collective(t, op, 3, n, 0xE0, path="pull", in_place=True, ref=ref)
        _collective(t, op, 3, n, 0xE0, path="pull", outside=True, ref=ref)
        _collective(t, op, 3, n, 0xE0, path="pull", outside=True, null=True, ref=nref)
    # 9 members: two launches, the pair fed back; both index forms
    for t, op in (("float", "max"), ("bfloat16", "min"), ("longlong", "max")):
        _collective(t, op, 9, 1001, 27, path="pull")
        _collective(t, op, 9, 1001, 27, path="pull", null=True)
        _collective(t, op, 9, 130, 28, path="pull", in_place=True)


def test_collective_single_member(torch_cuda):
    _collective("int", "max", 1, 1001, 5, path="pull")
    _collective("double", "min", 4, 11, 6, PE_start=2, PE_size=1, path="pull", null=True)
    _collective("half", "max", 1, 77, 8, path="pull", in_place=True)


@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path; a
    forced STAGED takes GETMEM), the chunk below the array size; a strided
    set, in place, one member, 9 members, both index forms."""
    cases = [("double", "max", 3, 0, 0, 3, 1001, False, False), ("short", "min", 2, 0, 0, 2, 5, False, True),
             ("float", "min", 8, 1, 1, 3, 700, False, True), ("int", "max", 3, 0, 0, 3, 1001, True, False),
             ("half", "max", 3, 0, 0, 3, 1501, False, False), ("long", "min", 1, 0, 0, 1, 9, False, False),
             ("bfloat16", "min", 9, 0, 0, 9, 333, False, False), ("float", "max", 9, 0, 0, 9, 333, False, True),
             ("float", "max", 8, 0, 0, 8, 1001, False, False)]
    with D.host_heaps(path) as (force, team, ran):
        for t, op, npes, start, log, size, n, ov, null in cases:
            force()
            _collective(t, op, npes, n, 0xD0 + size, start, log, size, path=ran, null=null,
                        in_place=ov, **team)


# ------------------------------------------------------------ 9. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the kernel
    writes a peer's two targets through a mapping of another process's memory
    (tests/support/loc_mp_worker.py starts nothing itself; the ranks are fresh
    child processes of this test)."""
    D.run_ranks("loc_mp_worker.py", tmp_path, "LOC_MP_OK")


# -------------------------------------------------------------------- 10. fuzz
def test_fuzz_30_calls(torch_cuda):
    seed = int(os.environ.get("LOC_FUZZ_SEED", "20261021"))
    rng = np.random.default_rng(seed)
    for i in range(30):
        t, op = C.PAIRS[int(rng.integers(len(C.PAIRS)))]
        P = int(rng.integers(1, 10))
        n = int(rng.integers(1, 5001))
        shift = int(rng.integers(0, C.group(t)))
        null = bool(rng.integers(2))
        overlap = bool(rng.integers(4) == 0)
        team = 2 <= P <= 8 and not overlap
        what = f"seed {seed} call {i}: {t} {op} P={P} n={n} shift={shift} null={null} overlap={overlap}"
        with D.named(what):
            _collective(t, op, P, n, seed + i, shift=0 if overlap else shift, in_place=overlap,
                        null=null, path="team" if team else "pull")
