"""Guard bands and tile edges: what the kernels write OUTSIDE their target.

Every kernel is a scalar head, whole 16-byte vectors in tiles of V, a scalar
tail, and above the launch limit several launches over shifted pointers
(kernel_common.hpp vec_split / edge_index / for_each_tile_run).  A `<` for a
`<=`, a tail stored as a whole vector or a run one tile too long gives a
correct target plus stray bytes beside it.  Here every output sits between
16 KiB guard bands of a position-varying pattern (tests/support/guarded.py),
every source too, and the sizes are the tile edges themselves:

  set A  nvec in {0, 1, V-1, V, V+1 for V = 128, 256, 1024, 2047..2049}
         whole vectors, one launch;
  set B  nvec = 256 j + d, 1 <= j <= 33, d in {-1, 0, +1}, under the
         2048-thread launch hook: every run boundary of every form +-1;

each with a ragged tail of 0, 1 and W-1 elements (W = 16 / element size),
at every common 16-byte phase of the element size (a head of 1..W-1
elements; n = head + nvec W + tail, so the kernel's own nvec is the set's),
and at one mismatched phase pair for the element-granular kernels.

Per case: the target bit-exact against the oracle's left-to-right fold (the
team forms: every member's own order), both bands of every output intact,
every source -- payload and bands -- bitwise what was uploaded; long double:
bytes 10..15 of every written slot zero from inputs whose padding is
garbage.  Expected values are folded once per (type, op) at the largest
size and sliced: the fold is element-wise.  Cases of one (type, phase) share
one set of source buffers and run in batches: one upload, the launches, one
synchronize and one download per batch.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import osgpu
from support import guarded as G
from support import half_ref as R
from support.gpu_doors import small_launches, stream, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LD_ON_GPU = True
SET_A = [0, 1, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
SET_B = [256 * j + d for j in range(1, 34) for d in (-1, 0, 1)]
KS_A = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17]
KS_B = [1, 2, 3, 6, 8, 9]
NPOOL = 17                # inputs per type: the largest K
ARENA_BYTES = 48 << 20    # a batch is flushed past this

TYPES = [t for t in O.TYPES if LD_ON_GPU or t != "longdouble"] + list(R.TYPES)


# ------------------------------------------------------------ types and sizes
def esize(t):
    if t in R.TYPES:
        return 2
    return 16 if t == "longdouble" else np.dtype(O.NP_DTYPE[t]).itemsize


def ops_of(t):
    return list(R.OPS) if t in R.TYPES else [op for op in O.OPS if O.has_op(t, op)]


def nmax(t):
    return (max(SET_B) + 2) * (16 // esize(t))


def common_phases(t):
    """Every 16-byte phase the element size admits, inputs and output alike."""
    s = esize(t)
    return [(p, p) for p in range(0, 16, s)]


def mixed_phases(t):
    """(input phase, output phase) pairs that differ, or that no vector form
    takes: the element-granular kernels.  16-byte elements can only sit 8
    bytes off; long double there is the scalar soft-float kernel, with the
    output at the same phase (test_longdouble_8byte_aligned_arrays) or not."""
    s = esize(t)
    if t == "longdouble":
        return [(8, 8), (8, 0)]
    return [(s if s < 16 else 8, 0)]


def sizes(t, nvecs, phase_in, phase_out, one=False):
    """Element counts whose vector split has nvec of `nvecs` whole vectors
    after the head the phase gives, with a tail of 0, 1 and W-1 elements."""
    s = esize(t)
    W = 16 // s
    head = (16 - phase_in) // s if phase_in == phase_out and phase_in % 16 and W > 1 else 0
    tails = sorted({0, 1, W - 1}) if W > 1 else [0]
    ns = {head + v * W + r for v in nvecs for r in tails}
    if one:
        ns.add(1)
    return sorted(ns)


def ops_at(t, k):
    """Every op at K = 2, 3, 8; elsewhere sum plus the others in rotation,
    dealt out so that K = 9, 16 and 17 together hold every one."""
    ops = ops_of(t)
    if k in (2, 3, 8):
        return ops
    others = [o for o in ops if o != "sum"]
    if k >= 9:
        mine = others[[9, 16, 17].index(k)::3]
        return ["sum"] + (mine or [others[k % len(others)]])
    return ["sum", others[[1, 4, 5, 6, 7].index(k) % len(others)]]


def test_every_type_op_pair_appears_at_nine_or_more_inputs():
    for t in TYPES:
        assert {op for k in (9, 16, 17) for op in ops_at(t, k)} == set(ops_of(t)), t
        for k in KS_A:
            assert ops_at(t, k)[0] == "sum" and len(ops_at(t, k)) >= 2, (t, k)


# ------------------------------------------------------ inputs and references
_POOL, _FOLD, _TEAM = {}, {}, {}


def pool(t):
    """NPOOL inputs of nmax(t) elements: edge values (NaN payloads, signed
    zeros, infinities, subnormals, wrap-around); long double with non-zero
    garbage in bytes 10..15 of every slot."""
    if t not in _POOL:
        n = nmax(t)
        arrs = []
        for j in range(NPOOL):
            if t in R.TYPES:
                rng = np.random.default_rng(0xB0D5 + j)
                a = rng.integers(0, 1 << 16, size=n, dtype=np.uint32).astype(np.uint16)
                tab = R.special_table(t)
                pick = rng.random(n) < 0.125
                a[pick] = tab[rng.integers(0, tab.size, size=int(pick.sum()))]
            else:
                a = O.gen_input(t, n, 0xB0D5 + 131 * j, "edge").copy()
                if t == "longdouble":
                    rows = a.view(np.uint8).reshape(-1, 16)
                    i = np.arange(n * 6, dtype=np.int64).reshape(-1, 6)
                    rows[:, 10:] = ((i * 29 + 7 * j) % 255 + 1).astype(np.uint8)
                    assert rows[:, 10:].all()
            arrs.append(a)
        _POOL[t] = arrs
    return _POOL[t]


def op2(t, op, a, b):
    return R.op2(t, op, a, b) if t in R.TYPES else O.op_elementwise(t, op, a, b)


def folded(t, op, k):
    """op(...op(in[0], in[1])..., in[k-1]) over the whole pool arrays."""
    if (t, op) not in _FOLD:
        p = pool(t)
        acc, accs = p[0], [p[0]]
        for j in range(1, NPOOL):
            acc = op2(t, op, acc, p[j])
            accs.append(acc)
        _FOLD[t, op] = accs
    return _FOLD[t, op][k - 1]


def team_folded(t, op, P):
    """Every member's result over the pool's first P arrays, own fold order."""
    if (t, op, P) not in _TEAM:
        _TEAM[t, op, P] = O.to_all(t, op, pool(t)[:P])
    return _TEAM[t, op, P]


def check_out(t, g, want, what):
    """Output g: bands intact, payload bit-exact; long double padding zero."""
    g.assert_guards(what)
    got = g.data()
    if t == "longdouble":
        rows = got.reshape(-1, 16)
        bad = np.flatnonzero((rows[:, :10] != O.value_bytes(want)).any(axis=1))
        assert bad.size == 0, f"{what}: elements {bad[:8]} differ from the oracle"
        pad = np.flatnonzero(rows[:, 10:].any(axis=1))
        assert pad.size == 0, (f"{what}: bytes 10..15 of elements {pad[:8]} are not zero: "
                               f"{rows[pad[0], 10:]}")
        return
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    d = G.first_diff(got, wb)
    assert d is None, f"{what}: element {d // esize(t)} of {want.size} differs from the oracle"


class Batch:
    """Cases of one (type, input phase) over one shared set of guarded
    sources; flush(): upload, launch every case, one synchronize, one
    download, check every output, then every shared source."""

    def __init__(self, torch, t, phase_in, nsrc, nelem):
        self.torch, self.t, self.phase_in, self.nsrc = torch, t, phase_in, nsrc
        self.nelem, self.s = nelem, esize(t)
        self._open()

    def _open(self):
        self.arena = G.Arena()
        p = pool(self.t)
        self.src = [self.arena.add(self.nelem * self.s, self.phase_in, p[j][:self.nelem])
                    for j in range(self.nsrc)]
        self.cases = []

    def out(self, n, phase):
        return self.arena.add(n * self.s, phase)

    def own_source(self, j, n, phase):
        """A copy of input j of exactly n elements (an in-place target)."""
        return self.arena.add(n * self.s, phase, pool(self.t)[j][:n])

    def add(self, launch, checks):
        """launch(stream) enqueues the case; checks() runs after the download."""
        self.cases.append((launch, checks))
        if self.arena.size > ARENA_BYTES:
            self.flush()

    def flush(self):
        if self.cases:
            self.arena.upload(self.torch)
            sp = stream(self.torch)
            for launch, _ in self.cases:
                launch(sp)
            self.torch.cuda.synchronize()
            self.arena.download()
            for _, checks in self.cases:
                checks()
            for j, g in enumerate(self.src):
                g.assert_unchanged(f"{self.t}: shared source {j} (phase {self.phase_in}) "
                                   f"after {len(self.cases)} cases")
            self.arena.dev = None
        self._open()


# --------------------------------------------------------------- raw combine
def add_combine(b, op, k, n, phase_out, in_place):
    t = b.t
    what = (f"combine {t}/{op} K={k} n={n} phase in {b.phase_in} out {phase_out}"
            f"{' in place' if in_place else ''}")
    if in_place:
        out = b.own_source(0, n, phase_out)
        srcs = [out] + b.src[1:k]
    else:
        out = b.out(n, phase_out)
        srcs = b.src[:k]
    want = folded(t, op, k)[:n]
    b.add(lambda st: osgpu.combine(t, op, out.ptr, [g.ptr for g in srcs], n, st),
          lambda: check_out(t, out, want, what))


COMBINE_A = [(t, pi, po) for t in TYPES for pi, po in common_phases(t) + mixed_phases(t)]


@pytest.mark.parametrize("t,phase_in,phase_out", COMBINE_A, ids=lambda v: str(v))
def test_combine_tile_edges(torch_cuda, t, phase_in, phase_out):
    """osgpu_combine over set A: K = 1..9, 16, 17 (chunks of <= 8 inputs),
    every op at K = 2, 3, 8 and a rotation elsewhere, in place at K = 2, 9."""
    ns = sizes(t, SET_A, phase_in, phase_out, one=True)
    b = Batch(torch_cuda, t, phase_in, NPOOL, max(ns))
    for n in ns:
        for k in KS_A:
            for op in ops_at(t, k):
                add_combine(b, op, k, n, phase_out, False)
                if k in (2, 9):
                    add_combine(b, op, k, n, phase_out, True)
    b.flush()


COMBINE_B = [(t, pi, po) for t in ("short", "float", "double", "complexd")
             for pi, po in (common_phases(t)[0], (common_phases(t) + mixed_phases(t))[1])]


@pytest.mark.parametrize("t,phase_in,phase_out", COMBINE_B, ids=lambda v: str(v))
def test_combine_run_edges_multi_launch(torch_cuda, small_launches, t, phase_in, phase_out):
    """osgpu_combine over set B under the 2048-thread hook: runs of 2048,
    2560, 2048, 1536, 1280, 1024, 1024 vectors (LDS form, K = 2..8) and 8192
    (vector form), every boundary +-1 vector.  sum, and at K = 2 and 8 a
    second op (max; complex: prod).  (complexd's non-zero phase, 8, is the
    element-granular kernel's.)"""
    small_launches(2048)
    ns = sizes(t, SET_B, phase_in, phase_out)
    b = Batch(torch_cuda, t, phase_in, max(KS_B), max(ns))
    other = "max" if "max" in ops_of(t) else "prod"
    for n in ns:
        for k in KS_B:
            for op in ["sum"] + ([other] if k in (2, 8) else []):
                add_combine(b, op, k, n, phase_out, False)
    b.flush()


# ------------------------------------------------------------- team launcher
TEAM_PAIRS = [("double", "sum"), ("int", "xor"), ("float", "max"), ("complexf", "prod"),
              ("short", "min"), ("long", "and"), ("complexd", "sum")]


def add_team(b, op, P, n, phase_out, remote):
    t = b.t
    what = (f"team{' remote shape' if remote else ''} {t}/{op} P={P} n={n} "
            f"phase in {b.phase_in} out {phase_out}")
    outs = [b.out(n, phase_out) for _ in range(P)]
    want = team_folded(t, op, P)
    L = osgpu.load()

    def launch(st):
        S = (ctypes.c_void_p * P)(*[g.ptr for g in b.src[:P]])
        D = (ctypes.c_void_p * P)(*[g.ptr for g in outs])
        tc, oc = osgpu.type_code(t), osgpu.OPS.index(op)
        rc = (L.osgpu_team_combine_shape(tc, oc, P, D, S, n, st, 1) if remote else
              L.osgpu_team_combine(tc, oc, P, D, S, n, st))
        assert rc == 0, (what, L.osgpu_last_error())

    def checks():
        for q in range(P):
            check_out(t, outs[q], want[q][:n], f"{what} member {q}")

    b.add(launch, checks)


def team_phases(t):
    return common_phases(t) + mixed_phases(t)


TEAM_A = [(t, op, P, False) for t, op in TEAM_PAIRS for P in range(2, 9)] + \
         [(t, op, P, True) for t, op in TEAM_PAIRS for P in (2, 5, 6, 7, 8)]


@pytest.mark.parametrize("t,op,P,remote", TEAM_A, ids=lambda v: str(v))
def test_team_tile_edges(torch_cuda, t, op, P, remote):
    """osgpu_team_combine (and the remote shapes through
    osgpu_team_combine_shape(..., 1)) over set A: LDS form, register form and
    the G = 2 rounds; every one of the P outputs guarded and exact in its own
    fold order, every source intact."""
    for phase_in, phase_out in team_phases(t):
        ns = sizes(t, SET_A, phase_in, phase_out, one=True)
        b = Batch(torch_cuda, t, phase_in, P, max(ns))
        for n in ns:
            add_team(b, op, P, n, phase_out, remote)
        b.flush()


@pytest.mark.parametrize("P", [2, 5, 8])
@pytest.mark.parametrize("t,op", TEAM_PAIRS, ids=lambda v: str(v))
def test_team_run_edges_multi_launch(torch_cuda, small_launches, t, op, P):
    """The team kernels over set B under the 2048-thread hook (runs are
    whole multiples of the combine's), phase 0 and one non-zero phase."""
    small_launches(2048)
    for phase_in, phase_out in (team_phases(t)[0], team_phases(t)[1]):
        ns = sizes(t, SET_B, phase_in, phase_out)
        b = Batch(torch_cuda, t, phase_in, P, max(ns))
        for n in ns:
            add_team(b, op, P, n, phase_out, False)
        b.flush()


# ---------------------------------------------------------------- long double
LD = pytest.mark.skipif(not LD_ON_GPU, reason="long double runs on the GPU")


@LD
@pytest.mark.parametrize("P", [2, 8])
@pytest.mark.parametrize("phase", [0, 8], ids=["vec", "8byte"])
def test_longdouble_team_padding_and_bounds(torch_cuda, P, phase):
    """osgpu_team_combine on long double (ld_team_kernel, 16-byte aligned
    and 8-byte aligned forms), n up to 2049: guards, every member's own fold
    order, and zero in bytes 10..15 of every written slot although every
    input slot carries garbage there.  (The combine's vector and 8-byte
    kernels, in place too: test_combine_tile_edges[longdouble-...].)"""
    ns = sizes("longdouble", SET_A, phase, phase, one=True)
    b = Batch(torch_cuda, "longdouble", phase, P, max(ns))
    for n in ns:
        for op in ops_of("longdouble"):
            add_team(b, op, P, n, phase, False)
    b.flush()


@LD
@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
def test_longdouble_host_fold_padding(torch_cuda, op):
    """Host-heap calls small enough for the host fold (run_host_fold,
    host_fold.hip fold_ld): every member's written slots carry zero in bytes
    10..15 from inputs with garbage there, in place too and for an active
    set of one PE (whose target is only its own source); the bytes after the
    target keep their pattern; the path taken is the host fold."""
    from support import team as T
    t, npes = "longdouble", 4
    src_all = pool(t)
    heap = 2 * 2049 * 16 + 3 * 4096
    tm = T.Team(npes, heap, device=False, host_fold=True)
    for size in (1, 2, 3):
        for n in (1, 7, 257, 2049):
            nbytes = n * 16
            src = [src_all[pe][:n] for pe in range(npes)]
            want = O.to_all(t, op, src, 0, 0, size)
            for in_place in (False, True):
                toff = 0 if in_place else (nbytes + 4095) // 4096 * 4096
                band = G.pattern(toff + nbytes, 4096)
                for pe in range(npes):
                    tm.write(pe, 0, src[pe])
                    if not in_place:
                        tm.write(pe, toff, G.fill_pattern(nbytes))
                    tm.write(pe, toff + nbytes, band)
                tm.run(t, op, toff, 0, n, 0, 0, size)
                assert all(tm.last_paths[pe] == "host_fold" for pe in range(size)), tm.last_paths
                what = f"host fold longdouble/{op} PE_size={size} n={n} in_place={in_place}"
                for pe in range(npes):
                    raw = tm.read(pe, toff, nbytes + 4096)
                    assert np.array_equal(raw[nbytes:], band), f"{what}: PE {pe}: bytes after the target"
                    rows = raw[:nbytes].reshape(-1, 16)
                    if pe >= size:
                        keep = G.fill_pattern(nbytes) if not in_place else \
                            src[pe].view(np.uint8).reshape(-1)
                        assert np.array_equal(raw[:nbytes], keep), f"{what}: non-member PE {pe}"
                        continue
                    assert np.array_equal(rows[:, :10], O.value_bytes(want[pe])), f"{what}: PE {pe}"
                    pad = np.flatnonzero(rows[:, 10:].any(axis=1))
                    assert pad.size == 0, (f"{what}: PE {pe}: bytes 10..15 of elements {pad[:8]} "
                                           f"are not zero: {rows[pad[0], 10:]}")
                    if not in_place:
                        assert np.array_equal(tm.read(pe, 0, nbytes),
                                              src[pe].view(np.uint8).reshape(-1)), \
                            f"{what}: PE {pe}'s source was modified"
