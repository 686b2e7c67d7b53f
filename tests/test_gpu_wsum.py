"""The float-accumulated half / bfloat16 sum on the GPU: osgpu_team_wsum
(team_wsum_vec_kernel, team_wsum_scalar_kernel, csrc/team.hip) and
osgpu_reduce_wsum on device and host heaps.  g = 8 elements a group, T = 256 g.

1. The raw launcher at tile edges: both types x both out_types, P in {1, 2, 3,
   5, 8}, ndst in {1, P}, with and without carry, n in {0, 1, g-1, g, g+1,
   T-1, T, T+1, 2T+g+1}; every array EXACTLY n elements between guard bands
   (tests/support/guarded.py); bit for bit tests/support/wsum_ref.py.
2. Phases: all 16-bit pointers at +2 bytes and all float pointers at +4 (a
   common head of 7: the vector kernel), one source at +2 alone, float pointers
   at +8 with 16-bit ones at 0, one target shifted alone (the last three: the
   element-granular kernel).
3. The NaN and overflow table at P in {2, 8}, in both kernels.
4. Carry: dsts[0] == carry with a float target; a three-chunk chain (8 + 8 + 1
   sources) whose middle chunk goes carry -> carry equals the 17-member sum.
5. Multi-launch under osgpu_test_max_launch_threads.
6. The collective on device heaps (TEAM), P in {2, 3, 8}, n = 3 T + g + 1, both
   out_types; the strided set (1, 1, 3) of 8 PEs.
7. The pull forms: OSGPU_PATH_PULL, overlapping ranges, a target outside the
   heap, 9 members (the carry, with a 16-bit and with a float target), one.
8. Host heaps: host fold, GETMEM with a small chunk at 9 members, a forced STAGED.
9. Two processes on one GPU (tests/support/wsum_mp_worker.py).
10. A seeded fuzz of 30 calls.

The inputs are checked (wsum_cases.pool, tests/test_wsum_ref.py) to tell this
sum from the per-step one for every P >= 3 used here.
"""
import os

import numpy as np
import pytest

import osgpu
from support import gpu_doors as D
from support import guarded as G
from support import wsum_cases as C
from support import wsum_ref as W
from support.gpu_doors import small_launches, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

g, T = W.GROUP, W.TILE
LENGTHS = sorted({0, 1, g - 1, g, g + 1, T - 1, T, T + 1, 2 * T + g + 1})


class Batch(D.LauncherBatch):
    """Cases of one (type, out_type): a case's sources are its P 16-bit arrays,
    then the float carry if it has one; its targets the ndst arrays of out_t."""

    def __init__(self, t, out_t, srcs=None, carry=None):
        super().__init__(t)
        self.out_t, self.osz = out_t, C.out_size(out_t)
        self.pool, self.cpool = (C.pool(t)[:2]) if srcs is None else (srcs, carry)
        self.own = srcs is not None

    def add(self, P, ndst, n, what, carry=False, sp=None, dp=None, cp=0):
        """sp / dp / cp: the 16-byte phases of the sources, targets and carry."""
        ph = lambda a, k: 0 if a is None else a[k]
        vs = [self.arena.add(n * 2, ph(sp, p), self.pool[p][:n]) for p in range(P)]
        cb = [self.arena.add(n * 4, cp, self.cpool[:n])] if carry else []
        vd = [self.arena.add(n * self.osz, ph(dp, q)) for q in range(ndst)]
        self.case(vs + cb, vd, what, out=self.out_t, P=P, ndst=ndst, n=n, carry=carry)

    def call(self, c, sp):
        osgpu.team_wsum(self.t, self.out_t, D.ptrs(c.dsts), D.ptrs(c.srcs[:c.P]), c.n,
                        carry=c.srcs[c.P].ptr if c.carry else None, stream=sp)

    def out_type(self, c, q):
        return "float" if self.out_t == "float" else self.t

    def want(self, c, q):
        if self.own:
            return W.wsum(self.t, self.out_t, [s[:c.n] for s in self.pool[:c.P]],
                          carry=self.cpool[:c.n] if c.carry else None)
        return C.want(self.t, self.out_t, c.P, c.n, c.carry)

    def check_case(self, c, what):
        D.targets_identical(c, what)


# ------------------------------------------------------------ 1. lengths
@pytest.mark.parametrize("t,out_t", W.PAIRS, ids=lambda x: x)
def test_launcher_lengths(torch_cuda, t, out_t):
    b = Batch(t, out_t)
    for P in (1, 2, 3, 5, 8):
        for ndst in sorted({1, P}):
            for carry in (False, True):
                for n in LENGTHS:
                    b.add(P, ndst, n, "aligned", carry=carry)
    b.launch(torch_cuda).check()


# ------------------------------------------------------------- 2. phases
@pytest.mark.parametrize("t,out_t", W.PAIRS, ids=lambda x: x)
def test_launcher_phases(torch_cuda, t, out_t):
    wide = out_t == "float"
    b = Batch(t, out_t)
    for P, ndst in ((2, 2), (3, 1), (8, 8)):
        for carry in (False, True):
            for n in (g - 1, g + 1, T + 1, 2 * T + g + 1):
                b.add(P, ndst, n, "16-bit pointers at +2, float pointers at +4: a head of 7",
                      carry=carry, sp=[2] * P, dp=[4 if wide else 2] * ndst, cp=4)
                one = [0] * P
                one[P - 1] = 2
                b.add(P, ndst, n, f"source {P - 1} at +2 alone", carry=carry, sp=one)
                b.add(P, ndst, n, "float pointers at +8, 16-bit pointers at 0", carry=carry,
                      dp=[8 if wide else 0] * ndst, cp=8)
                tgt = [0] * ndst
                tgt[ndst - 1] = 4 if wide else 2
                b.add(P, ndst, n, f"target {ndst - 1} shifted alone", carry=carry, dp=tgt)
    b.launch(torch_cuda).check()


# ------------------------------------------------ 3. NaNs and overflow
@pytest.mark.parametrize("t,out_t", W.PAIRS, ids=lambda x: x)
def test_launcher_nan_and_overflow_table(torch_cuda, t, out_t):
    for P in (2, 8):
        srcs = W.nan_table(t, P)
        n = len(srcs[0])
        carry = W.accumulate(t, [np.roll(s, 11) for s in srcs])  # NaNs and infinities in the carry
        b = Batch(t, out_t, srcs, carry)
        for ndst in (1, P):
            for cy in (False, True):
                b.add(P, ndst, n, "table, vector kernel", carry=cy)
                b.add(P, ndst, n, "table, a head of 7", carry=cy, sp=[2] * P,
                      dp=[4 if out_t == "float" else 2] * ndst, cp=4)
                one = [0] * P
                one[0] = 2
                b.add(P, ndst, n, "table, element-granular kernel", carry=cy, sp=one)
        b.launch(torch_cuda).check()
        if P == 8 and t == "bfloat16":
            # the overflow of the float accumulator, then -inf: the default NaN
            col = [k for k in range(n) if all(s[k] == 0x7F7F for s in srcs[:7]) and srcs[7][k] == 0xFF80]
            assert col, "the table lost its overflow column"
            want = b.want(b.cases[0], 0)
            assert int(want[col[0]]) == (0xFFC00000 if out_t == "float" else 0xFFC0)


# --------------------------------------------------------------- 4. carry
@pytest.mark.parametrize("t", W.TYPES)
def test_target_is_the_carry(torch_cuda, t):
    """out_type float, ndst = 1, dsts[0] == carry: in both kernels."""
    srcs, carry, _ = C.pool(t)
    a = G.Arena()
    cases = []
    for P in (1, 3, 8):
        for n in (g + 1, 2 * T + g + 1):
            for sp in (0, 2):   # sources at +2 against the carry at 0: element-granular
                vs = [a.add(n * 2, sp, srcs[p][:n]) for p in range(P)]
                cases.append((P, n, vs, a.add(n * 4, 0, carry[:n])))
    a.upload(torch_cuda)
    sp = D.stream(torch_cuda)
    for P, n, vs, cb in cases:
        osgpu.team_wsum(t, "float", [cb.ptr], D.ptrs(vs), n, carry=cb.ptr, stream=sp)
    torch_cuda.cuda.synchronize()
    a.download()
    for P, n, vs, cb in cases:
        what = f"{t} P={P} n={n} source phase {vs[0].phase}"
        assert np.array_equal(cb.data().view(np.uint32), C.want(t, "float", P, n, True)), what
        cb.assert_guards(what)
        for v in vs:
            v.assert_unchanged(what)


@pytest.mark.parametrize("t,out_t", W.PAIRS, ids=lambda x: x)
def test_three_chunk_chain_equals_17_members(torch_cuda, t, out_t):
    srcs, _, _ = C.pool(t)
    n = 2 * T + g + 1
    a = G.Arena()
    vs = [a.add(n * 2, 0, srcs[p][:n]) for p in range(17)]
    acc = a.add(n * 4)
    out = a.add(n * C.out_size(out_t))
    a.upload(torch_cuda)
    sp = D.stream(torch_cuda)
    osgpu.team_wsum(t, "float", [acc.ptr], D.ptrs(vs[:8]), n, stream=sp)
    osgpu.team_wsum(t, "float", [acc.ptr], D.ptrs(vs[8:16]), n, carry=acc.ptr, stream=sp)
    osgpu.team_wsum(t, out_t, [out.ptr], D.ptrs(vs[16:]), n, carry=acc.ptr, stream=sp)
    torch_cuda.cuda.synchronize()
    a.download()
    whole = W.wsum(t, out_t, [s[:n] for s in srcs])
    assert np.array_equal(out.data().view(C.out_dtype(out_t)), whole)
    assert np.array_equal(acc.data().view(np.uint32), W.accumulate(t, [s[:n] for s in srcs[:16]]))
    out.assert_guards("chain target")
    acc.assert_guards("chain carry")


# --------------------------------------------------------- 5. multi-launch
@pytest.mark.parametrize("t,out_t", [("half", "half"), ("bfloat16", "float")], ids=lambda x: x)
def test_launcher_multi_launch(torch_cuda, small_launches, t, out_t):
    """3 tiles + a group + 1 under a limit of 512 threads (2 tiles) a launch:
    equal to the single launch and to the expected arrays; a common head adds
    the edges to the first launch."""
    res = []
    n = 3 * T + g + 1
    for limit in (0, 512):
        small_launches(limit)
        b = Batch(t, out_t)
        for P, ndst in ((2, 2), (8, 1), (8, 8)):
            for carry in (False, True):
                b.add(P, ndst, n, f"limit {limit}", carry=carry)
                b.add(P, ndst, n, f"limit {limit} edges", carry=carry, sp=[2] * P,
                      dp=[4 if out_t == "float" else 2] * ndst, cp=4)
        b.launch(torch_cuda).check()
        res.append([d.data().copy() for c in b.cases for d in c.dsts])
    for one, many in zip(*res):
        assert np.array_equal(one, many)


# ---------------------------------------------------- 6-8. the collective
def _collective(t, out_t, npes, n, seed, PE_start=0, log=0, PE_size=None, path="team", shift=0,
                overlap=False, device=True, host_fold=False, outside=False, ref=None):
    """One call on a fresh team; checks every member's target against
    wsum_ref, that all members hold the same bytes, the bytes round the
    target, non-members' heaps, the path and (in Team._on_members) pSync.
    Returns the first member's target bytes.  overlap: the target starts on the
    source's first byte; outside: the targets are device memory outside the
    registered heaps."""
    from support import team as TM
    PE_size = npes if PE_size is None else PE_size
    osz = C.out_size(out_t)
    soff, toff, hb = C.layout(n, out_t, shift)
    if overlap:
        toff = soff
    tm = TM.Team(npes, hb, device=device, host_fold=host_fold)
    srcs = C.mixed_inputs(t, npes, n, seed)
    for pe in range(npes):
        tm.fill(pe, 0, hb, 0xC3)
        tm.write(pe, soff, srcs[pe])
    before = {pe: tm.read(pe, 0, hb) for pe in range(npes)}
    members = [PE_start + (i << log) for i in range(PE_size)]
    want = W.wsum(t, out_t, [srcs[pe] for pe in members])
    what = f"{t} -> {out_t} P={PE_size} n={n}"
    if outside:
        import torch
        ext = torch.full((npes, n * osz + 64), 0xC3, dtype=torch.uint8, device="cuda:0")
        C.run(tm, t, out_t, lambda pe: ext[pe].data_ptr(), soff, n, PE_start, log, PE_size)
        torch.cuda.synchronize()
        back = ext.cpu().numpy()
    else:
        C.run(tm, t, out_t, lambda pe: tm.ptr(pe, toff), soff, n, PE_start, log, PE_size)
    first = None
    for pe in range(npes):
        after = tm.read(pe, 0, hb)
        if pe not in members:
            assert np.array_equal(after, before[pe]), f"{what}: PE {pe} is not a member"
            continue
        w = f"{what} PE {pe}"
        if outside:
            got = back[pe][:n * osz]
            assert (back[pe][n * osz:] == 0xC3).all(), f"{w}: bytes after the target"
            assert np.array_equal(after, before[pe]), f"{w}: the heap changed"
        else:
            got = after[toff:toff + n * osz]
            assert np.array_equal(after[:toff], before[pe][:toff]), f"{w}: bytes before the target"
            assert np.array_equal(after[toff + n * osz:], before[pe][toff + n * osz:]), \
                f"{w}: bytes after the target"
        gv = got.view(C.out_dtype(out_t))
        bad = np.flatnonzero(gv != want)
        assert bad.size == 0, f"{w}: element {int(bad[0]) if bad.size else 0} differs"
        if path is not None:
            assert tm.last_paths[pe] == path, (w, tm.last_paths)
        first = got.copy() if first is None else first
        assert np.array_equal(got, first), f"{w}: not the bytes of the first member"
    if ref is not None:
        assert np.array_equal(first, ref), f"{what}: not the bytes of the team result"
    return first


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("t,out_t", W.PAIRS, ids=lambda x: x)
def test_collective_device_heaps(torch_cuda, t, out_t, P):
    """Every shard has a partial tile and the last a tail."""
    _collective(t, out_t, P, 3 * T + g + 1, 0xD0 + P)
    _collective(t, out_t, P, g + 1, 0xD0 + P)


def test_collective_strided_set(torch_cuda):
    for t, out_t in W.PAIRS:
        _collective(t, out_t, 8, 3 * T + g + 1, 5, PE_start=1, log=1, PE_size=3)
        _collective(t, out_t, 8, 1001, 6, PE_start=1, log=1, PE_size=3, shift=3)


def test_collective_pull_forms(torch_cuda):
    for (t, out_t), n in zip(W.PAIRS, (1001, 2 * T + 3, 777, 4099)):
        ref = _collective(t, out_t, 3, n, 0xE0)
        with D.forced_path(osgpu.PATH_PULL):
            _collective(t, out_t, 3, n, 0xE0, path="pull", ref=ref)
        _collective(t, out_t, 3, n, 0xE0, path="pull", overlap=True, ref=ref)
        _collective(t, out_t, 3, n, 0xE0, path="pull", outside=True, ref=ref)
        # 9 members: two launches, the float accumulator carried (in scratch for
        # a 16-bit target, in the target itself for a float one)
        _collective(t, out_t, 9, 1001, 27, path="pull")
        _collective(t, out_t, 9, 130, 28, path="pull", overlap=True)
        _collective(t, out_t, 17, 2 * T + 1, 29, path="pull")


def test_collective_single_member(torch_cuda):
    _collective("half", "half", 1, 1001, 5, path="pull")
    _collective("bfloat16", "float", 4, 11, 6, PE_start=2, PE_size=1, path="pull")
    _collective("half", "float", 1, 77, 8, path="pull", overlap=True)
    _collective("bfloat16", "bfloat16", 1, 77, 8, path="pull", overlap=True)


@pytest.mark.parametrize("path", ["host_fold", "getmem", "staged"])
def test_collective_host_heaps(torch_cuda, path):
    """Host fold and GETMEM (forced by the fold limit / osgpu_set_host_path; a
    forced STAGED takes GETMEM), the chunk below the array size; a strided
    set, overlapping ranges, one member, 9 members."""
    cases = [("half", "half", 3, 0, 0, 3, 1001, False), ("bfloat16", "float", 2, 0, 0, 2, 5, False),
             ("bfloat16", "bfloat16", 8, 1, 1, 3, 700, False), ("half", "float", 3, 0, 0, 3, 1001, True),
             ("bfloat16", "bfloat16", 3, 0, 0, 3, 1501, True), ("half", "half", 1, 0, 0, 1, 9, False),
             ("bfloat16", "bfloat16", 9, 0, 0, 9, 2333, False), ("half", "float", 9, 0, 0, 9, 2333, False),
             ("bfloat16", "float", 8, 0, 0, 8, 1001, False)]
    with D.host_heaps(path) as (force, team, ran):
        for t, out_t, npes, start, log, size, n, ov in cases:
            force()
            _collective(t, out_t, npes, n, 0xD0 + size, start, log, size, path=ran, overlap=ov,
                        **team)


# ------------------------------------------------------------ 9. two processes
def test_two_processes_one_gpu(torch_cuda, tmp_path):
    """2 ranks, one process each, heaps made by osgpu_heap_create: the kernel
    writes a peer's target through a mapping of another process's memory
    (tests/support/wsum_mp_worker.py starts nothing itself; the ranks are fresh
    child processes of this test)."""
    D.run_ranks("wsum_mp_worker.py", tmp_path, "WSUM_MP_OK")


# -------------------------------------------------------------------- 10. fuzz
def test_fuzz_30_calls(torch_cuda):
    seed = int(os.environ.get("WSUM_FUZZ_SEED", "20261021"))
    rng = np.random.default_rng(seed)
    for i in range(30):
        t, out_t = W.PAIRS[int(rng.integers(len(W.PAIRS)))]
        P = int(rng.integers(1, 11))
        n = int(rng.integers(1, 5001))
        shift = int(rng.integers(0, g))
        overlap = bool(rng.integers(4) == 0)
        pull = bool(rng.integers(5) == 0)
        team = 2 <= P <= 8 and not overlap and not pull
        what = f"seed {seed} call {i}: {t} -> {out_t} P={P} n={n} shift={shift} overlap={overlap} pull={pull}"
        with D.named(what):
            if pull:
                with D.forced_path(osgpu.PATH_PULL):
                    _collective(t, out_t, P, n, seed + i, shift=0 if overlap else shift,
                                overlap=overlap, path="pull")
            else:
                _collective(t, out_t, P, n, seed + i, shift=0 if overlap else shift,
                            overlap=overlap, path="team" if team else "pull")
