"""x87_wave_cases.py -- TEST INFRASTRUCTURE: long double inputs for the x87
team folds (csrc/x87.hpp team_fold_sum_prod, team_fold_minmax) laid out wave
by wave.  Pure numpy and the oracle; nothing here touches a GPU.

On the host the folds choose their fast add (F_FULL, F_NEAR, F_SAME,
F_SAME_NEAR) per element; on the device wave_all() is a 64-lane ballot, so one
hard lane moves its whole wave to another mode.  ld_team_kernel's element index
is blockIdx * 256 + threadIdx: elements 64 r .. 64 r + 63 of arrays handed to
osgpu_team_combine are exactly one wave, whatever the pointers' alignment.  The
inputs here are therefore built in RUNS of 64 elements, every run of one class
(the mode its wave takes, wave_mode() restates the gate from the constants the
host build exports) and one density of EVENT lanes: none, a few (1..8, lanes 0
and 63 among them) or all 64.  The last run has 37 elements (inactive lanes in
the ballot).

An event is an input made to leave the run's fast add, or to sit on its edge:
see SUM_KINDS and PROD_KINDS.  Each is aimed at one fold -- member 0's (shared
by member 1) or the last member's, the two fold groups of fold_rounds -- and
sits in the first, a middle or the last member by turn, so the general op
starts in an early, a middle and the last round.  A cancellation is made
against the oracle's own running value of that fold.

Also here, shared by tests/test_x87_softfloat.py and the GPU twins
(tests/test_gpu_x87.py, tests/test_gpu_x87_waves.py): the random encodings and
operand pairs of the two-input tests, and the tie pool of the max / min fold.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle as O

BIAS, EMAX, TOP, ONES = 16383, 0x7FFF, 1 << 63, (1 << 64) - 1
RUN, TAIL = 64, 37


# ------------------------------------------------ encodings, both directions
def pack(m, e, s):
    """long double array of significands m, biased exponents e, sign bits s"""
    m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1)
    n = m.size
    se = (np.asarray(e).astype(np.uint64) | (np.asarray(s).astype(np.uint64) << np.uint64(15)))
    arr = np.zeros((n, 16), np.uint8)
    arr[:, :8] = m.view(np.uint8).reshape(n, 8)
    arr[:, 8:10] = se.astype(np.uint16).reshape(-1).view(np.uint8).reshape(n, 2)
    return arr.reshape(-1).view(np.longdouble)


def fields(x):
    """(significand uint64, biased exponent int64, sign int64) of a long double array"""
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1, 16)
    m = raw[:, :8].copy().view(np.uint64).reshape(-1)
    se = raw[:, 8:10].copy().view(np.uint16).reshape(-1).astype(np.int64)
    return m, se & EMAX, se >> 15


def is_normal(m, e):
    return (e >= 1) & (e < EMAX) & ((m >> np.uint64(63)) == 1)


def unordered(m, e):
    """fcomi's unordered operands: NaNs, unnormals, pseudo-infinities / NaNs;
    pseudo-denormals too (team_fold_minmax sends them to the compare fold)"""
    j = (m >> np.uint64(63)) == 1
    return np.where(e == 0, j, np.where(e == EMAX, m != np.uint64(TOP), ~j))


# ------------------------------------- the two-input tests' operands (shared)
def raw_random(n, seed, mode):
    r = O.splitmix64(seed, n)
    r2 = O.splitmix64(seed ^ 0x77, n)
    m = r.copy()
    e = r2 & np.uint64(0x7FFF)
    if mode == "normal":
        m |= np.uint64(1 << 63)
    elif mode == "near":       # operands within 2^65 of each other around 1
        e = np.uint64(16383) + (r2 % np.uint64(130)) - np.uint64(65)
        m |= np.uint64(1 << 63)
    elif mode == "low":        # denormal / pseudo-denormal / tiny normals
        e = r2 % np.uint64(70)
        m |= np.uint64(1 << 63) * ((r2 >> np.uint64(20)) & np.uint64(1))
    elif mode == "high":       # overflow range
        e = np.uint64(0x7FFF) - (r2 % np.uint64(70))
        m |= np.uint64(1 << 63)
    s = (r2 >> np.uint64(40)) & np.uint64(1)
    se = (e | (s << np.uint64(15))).astype(np.uint16)
    arr = np.zeros((n, 16), np.uint8)
    arr[:, :8] = m.view(np.uint8).reshape(n, 8)
    arr[:, 8:10] = se.view(np.uint8).reshape(n, 2)
    return arr.reshape(-1).view(np.longdouble)


def _pairs(where, n=60_000):
    r = O.splitmix64(77, 4 * n).reshape(4, n)
    base_e = {"unit": 16383, "underflow": 3, "overflow": 0x7FFE - 1}[where]
    diffs = np.array([0, 1, 2, 3, 29, 30, 31, 32, 62, 63, 64, 65, 66, 67, 70, 120, 200], np.int64)
    d = diffs[r[0] % np.uint64(diffs.size)]
    ea = np.full(n, base_e, np.int64) + (r[1] % np.uint64(3)).astype(np.int64) - 1
    eb = np.clip(ea - d, 1, 0x7FFE)
    # significands: random, or 2^63 + small, or 2^64 - small (seams of the
    # borrow / carry cases)
    kind = r[2] % np.uint64(3)
    small = r[3] & np.uint64(0xFF)
    top = np.uint64(1 << 63)
    ma = np.where(kind == 0, r[2] | top, np.where(kind == 1, top + small,
                                                  np.uint64((1 << 64) - 1) - small))
    mb = np.where(kind == 2, r[3] | top, np.where(kind == 1, np.uint64((1 << 64) - 1) - small,
                                                  top + small))
    sa = (r[1] >> np.uint64(7)) & np.uint64(1)
    sb = (r[1] >> np.uint64(9)) & np.uint64(1)

    def pack(m, e, s):
        arr = np.zeros((n, 16), np.uint8)
        arr[:, :8] = m.astype(np.uint64).view(np.uint8).reshape(n, 8)
        se = (e.astype(np.uint64) | (s << np.uint64(15))).astype(np.uint16)
        arr[:, 8:10] = se.view(np.uint8).reshape(n, 2)
        return arr.reshape(-1).view(np.longdouble)
    return pack(ma, ea, sa), pack(mb, eb, sb)


def _deep_cancel_pairs(gap, n=120_000, seed=41):
    """Opposite-sign normal pairs near 1 whose difference cancels 7 to 31
    leading bits of the top significand word (x87.hpp add_fast's normalise
    by ffbh of the top word and its funnel shift, every lz in 0..31):
    gap 0: b's top 32-bit significand word = a's +- k; gap 1: a's top word
    0x80000000 against b's 0xFFFFFFFF - k (2a - b is then about k * 2^32);
    k = 2^j + a random part below 2^j for j in 0..24 (k in 1..2^25), the low
    words random."""
    r = O.splitmix64(seed + gap, 5 * n).reshape(5, n)
    j = (r[0] % np.uint64(25)).astype(np.uint64)
    k = (np.uint64(1) << j) + (r[1] & ((np.uint64(1) << j) - np.uint64(1)))
    top = np.uint64(1 << 31)
    if gap == 0:
        ta = top + (r[2] >> np.uint64(33)) % (np.uint64(1 << 31) - np.uint64(1 << 26)) \
            + np.uint64(1 << 25)
        up = (r[3] & np.uint64(1)).astype(bool)
        tb = np.where(up, ta + k, ta - k)
        tb = np.minimum(tb, np.uint64(0xFFFFFFFF))
    else:
        ta = np.full(n, top, np.uint64)
        tb = np.uint64(0xFFFFFFFF) - k + np.uint64(1)
    ma = (ta << np.uint64(32)) | (r[3] >> np.uint64(32))
    mb = (tb << np.uint64(32)) | (r[4] & np.uint64(0xFFFFFFFF))
    ea = np.full(n, 16383, np.uint64) + (r[2] & np.uint64(3)) - np.uint64(1)
    eb = ea - np.uint64(gap)
    sa = (r[4] >> np.uint64(40)) & np.uint64(1)
    sb = sa ^ np.uint64(1)

    def pack(m, e, sg):
        arr = np.zeros((n, 16), np.uint8)
        arr[:, :8] = m.astype(np.uint64).view(np.uint8).reshape(n, 8)
        arr[:, 8:10] = (e | (sg << np.uint64(15))).astype(np.uint16).view(np.uint8).reshape(n, 2)
        return arr.reshape(-1).view(np.longdouble)
    return pack(ma, ea, sa), pack(mb, eb, sb)


def tie_pairs(n=100_000):
    """Operands with the same exponent and the same top 32 significand bits:
    low words random, equal or one apart, both sign pairings."""
    r = O.splitmix64(61, 4 * n).reshape(4, n)
    hi = (r[0] | np.uint64(1 << 63)) & np.uint64(0xFFFFFFFF00000000)
    lo_a = r[1] & np.uint64(0xFFFFFFFF)
    kind = r[2] % np.uint64(3)
    lo_b = np.where(kind == 0, r[3] & np.uint64(0xFFFFFFFF),
                    np.where(kind == 1, lo_a, (lo_a + np.uint64(1)) & np.uint64(0xFFFFFFFF)))
    e = np.full(n, 16383, np.uint64) + (r[2] >> np.uint64(8)) % np.uint64(40) - np.uint64(20)
    sa = (r[3] >> np.uint64(40)) & np.uint64(1)
    sb = np.where((r[3] >> np.uint64(41)) & np.uint64(3) == 0, sa, sa ^ np.uint64(1))

    def pack(m, sg):
        arr = np.zeros((n, 16), np.uint8)
        arr[:, :8] = m.astype(np.uint64).view(np.uint8).reshape(n, 8)
        arr[:, 8:10] = (e | (sg << np.uint64(15))).astype(np.uint16).view(np.uint8).reshape(n, 2)
        return arr.reshape(-1).view(np.longdouble)
    return pack(hi | lo_a, sa), pack(hi | lo_b, sb)


def equal_opposite_operands(per_mode=20_000):
    """(a, -a): every kind of encoding, every other significand a power of two
    (a + a then carries out of the 64 bits exactly)."""
    a = np.concatenate([raw_random(per_mode, 31, m) for m in ("normal", "near", "low", "high",
                                                              "any")])
    raw = O.value_bytes(a).reshape(-1, 10).copy()
    raw[::2, :7] = 0            # every other significand a power of two (2^63):
    raw[::2, 7] = 0x80          # a + a carries out of the 64 bits exactly
    a = O.from_value_bytes("longdouble", raw.reshape(-1))
    neg = O.value_bytes(a).reshape(-1, 10).copy()
    neg[:, 9] ^= 0x80
    b = O.from_value_bytes("longdouble", neg.reshape(-1))
    return a, b


def _tie_pool():
    pool = np.zeros((12, 10), np.uint8)

    def enc(m, e, sgn):
        b = np.zeros(10, np.uint8)
        b[:8] = np.frombuffer(np.uint64(m).tobytes(), np.uint8)
        b[8:10] = np.frombuffer(np.uint16(e | (sgn << 15)).tobytes(), np.uint8)
        return b
    vals = [(0, 0, 0), (0, 0, 1), (1 << 40, 0, 0), (1 << 40, 0, 1), (1 << 63, 0x7FFF, 0),
            (1 << 63, 0x7FFF, 1), (0xC000000000000000, 0x3FFF, 0), (0xC000000000000000, 0x3FFF, 1),
            (1 << 63, 1, 0), (1 << 63, 1, 1), (0x8000000000000001, 0x7FFE, 0),
            (0x8000000000000001, 0x7FFE, 1)]
    for i, v in enumerate(vals):
        pool[i] = enc(*v)
    return pool


# value bytes of the 12 values whose extremes tie across members: +0 against
# -0, equal denormals, infinities, duplicated normals
TIE_POOL = _tie_pool()


# ------------------------------------------------------------------ the gate
@functools.lru_cache(maxsize=None)
def gate():
    """(kNearSpread, kNearEmin, kNearEmax) as the host build of x87.hpp has them"""
    from support import team as T
    L = T.build_x87check()
    return tuple(int(L.x87check_gate(i)) for i in range(3))


def n_runs(n: int) -> int:
    return (n + RUN - 1) // RUN


def wave_mode(srcs, r: int) -> str:
    """The fold mode the device wave of run r takes on a sum of `srcs`
    (team_fold_sum_prod's choice with wave_all over the run's lanes)."""
    spread, lo, hi = gate()
    f = [fields(s[RUN * r:RUN * (r + 1)]) for s in srcs]
    m, e, s = (np.stack([x[i] for x in f]) for i in range(3))
    near = (is_normal(m, e).all(0) & (e.max(0) - e.min(0) <= spread) & (e.min(0) >= lo)
            & (e.max(0) <= hi)).all()
    same = (s == s[0]).all()
    return ("same_near" if near else "same") if same else ("near" if near else "full")


# ---------------------------------------------------------------- the layout
CLASSES = ("near", "same_near", "same", "full")
DENSITIES = ("none", "few", "all")
# the few event lanes of a class's two few-runs (and of the partial last run)
FEW = {"near": ((63,), (0, 1, 2, 30, 33, 61, 62, 63)),
       "same_near": ((0,), (0, 7, 8, 31, 32, 55, 56, 63)),
       "same": ((0, 9, 31, 32, 63), (1, 2, 16, 17, 40, 47, 62, 63)),
       "full": ((0, 21, 63), (0, 5, 6, 31, 32, 33, 62, 63))}
TAIL_EVENTS = (0, 17, TAIL - 1)

SUM_KINDS = {
    # zero: x = -(running value) exactly; cancel: x = -(running value)(1 + 2^-j u),
    # j in 20..63 (later rounds meet gaps above 30); tie: the running value's
    # exponent and top word, opposite sign, low word equal / one above / one
    # below / random; widest: P - 1 inputs 2^64 - small at the window's top, the
    # last-folded one at its bottom; topword: _deep_cancel_pairs (7..31 leading
    # bits cancel: the near add's own normalising shifts); wrap: the sum is
    # 2^64 - 2^-d, all ones rounded up to the next power of two
    "near": ("zero", "cancel", "tie", "widest", "topword", "wrap"),
    # carry: 2^64 - small twice
    "same_near": ("widest", "carry", "wrap"),
    # grid: the running sum lands on the denormal grid and later becomes normal
    # again; seam: _pairs' exponent gaps of 62..65 (outside add_fast)
    "same": ("qnan", "snan", "inf", "denormal", "pseudo", "unnormal", "overflow", "grid", "seam"),
    "full": ("qnan", "snan", "inf", "denormal", "pseudo", "unnormal", "overflow", "grid", "seam"),
}
PROD_KINDS = ("underflow", "overflow", "wrap", "zeroinf", "qnan", "snan")


def sum_runs():
    """[(class, repeat, density, event lanes)] of the whole runs: every (class,
    density) twice -- the smallest count; 64 lanes of the "all" runs hold every
    event kind in every member position."""
    out = []
    for rep in (0, 1):
        for cls in CLASSES:
            for dens in DENSITIES:
                lanes = {"none": (), "few": FEW[cls][rep], "all": tuple(range(RUN))}[dens]
                out.append((cls, rep, dens, lanes))
    return out


N_SUM = RUN * len(sum_runs()) + TAIL
N_PROD = RUN * 6 + TAIL
N_MINMAX = RUN * 6 + TAIL


class _Lanes:
    """P x n fields, one lane settable at a time in Python integers."""

    def __init__(self, P, n, seed):
        self.P, self.n = P, n
        self.rng = np.random.default_rng(seed)
        self.M = np.zeros((P, n), np.uint64)
        self.E = np.zeros((P, n), np.int64)
        self.S = np.zeros((P, n), np.int64)
        self.event = np.zeros(n, bool)
        self.kind = np.full(n, "", dtype=object)

    def get(self, p, i):
        return int(self.M[p, i]), int(self.E[p, i]), int(self.S[p, i])

    def put(self, p, i, m, e, s):
        assert 0 <= m <= ONES and 0 <= e <= EMAX and s in (0, 1)
        self.M[p, i], self.E[p, i], self.S[p, i] = np.uint64(m), e, s

    def put_ld(self, p, i, x):
        m, e, s = fields(x)
        self.put(p, i, int(m[0]), int(e[0]), int(s[0]))

    def rand64(self):
        return int(self.rng.integers(0, 1 << 63)) * 2 + int(self.rng.integers(0, 2))

    def arrays(self):
        return [np.ascontiguousarray(pack(self.M[p], self.E[p], self.S[p])) for p in range(self.P)]

    def fold(self, op, i, members):
        """the oracle's fold of lane i over `members`, in that order"""
        if len(members) == 1:
            return self.get(members[0], i)
        srcs = [pack([self.M[p, i]], [self.E[p, i]], [self.S[p, i]]) for p in members]
        m, e, s = fields(O.to_all("longdouble", op, srcs)[0])
        return int(m[0]), int(e[0]), int(s[0])

    def aim(self, c, nk):
        """Event number c of a class with nk kinds: (the member that holds it,
        the fold order it is aimed at, its place k in that order).  The
        member is the first, a middle, the last by turn; the fold member 0's,
        then the last member's."""
        P = self.P
        posm = (0, P // 2, P - 1)[(c // nk) % 3]
        q = 0 if (c // (3 * nk)) % 2 == 0 else P - 1
        order = [q] + [p for p in range(P) if p != q]
        return posm, order, order.index(posm)

    def running(self, op, i, order, k):
        """what the fold `order` holds when it meets its k-th operand; for
        k = 0 (the operand starts the fold) the operand it meets first"""
        return self.get(order[1], i) if k == 0 else self.fold(op, i, order[:k])


def _base_significands(L, seed):
    """random significands (J set) and signs of every member: raw_random's"""
    for p in range(L.P):
        m, _, s = fields(raw_random(L.n, seed + 13 * p, "normal"))
        L.M[p], L.S[p] = m, s


def _wrap_operand(pm, pe, ps, lo):
    """x with (pm, pe) + x = 2^64 - 2^-d: all ones rounded up.  None where it
    has no such x above exponent lo."""
    g = (1 << 64) - pm
    if g < 2:
        return None
    d = 64 - (g - 1).bit_length()
    if not 1 <= d <= 20 or pe - d < lo:
        return None
    return (g << d) - 1, pe - d, ps


def _sum_event(L, i, cls, kind, c, lo, spread, pools):
    nk = len(SUM_KINDS[cls])
    posm, order, k = L.aim(c, nk)
    P, rng = L.P, L.rng
    ls = int(L.S[0, i]) if cls in ("same", "same_near") else None   # the lane's one sign
    sgn = ls if ls is not None else int(rng.integers(0, 2))
    if kind in ("zero", "cancel", "tie", "wrap"):
        pm, pe, ps = L.running("sum", i, order, k)
        if kind == "wrap":
            x = _wrap_operand(pm, pe, ps, lo)
            if x is not None:
                return L.put(posm, i, *x)
            kind = "zero" if cls == "near" else "carry"
        if kind == "zero":
            return L.put(posm, i, pm, pe, ps ^ 1)
        if kind == "cancel":
            j = 20 + int(rng.integers(0, 44))
            u = np.longdouble(int(rng.integers(1, 1 << 53))) / np.longdouble(2.0 ** 53)
            v = pack([pm], [pe], [ps])
            return L.put_ld(posm, i, -v * (np.longdouble(1) + np.ldexp(np.longdouble(1), -j) * u))
        if kind == "tie":
            low = pm & 0xFFFFFFFF
            low = (low, (low + 1) & 0xFFFFFFFF, (low - 1) & 0xFFFFFFFF,
                   int(rng.integers(0, 1 << 32)))[(c // nk) % 4]
            return L.put(posm, i, (pm & ~0xFFFFFFFF) | low, pe, ps ^ 1)
    if kind == "carry":         # 2^64 - small twice, adjacent in the fold
        other = order[k - 1] if k else order[1]
        e = int(L.E[posm, i])
        for p in (posm, other):
            L.put(p, i, ONES - int(rng.integers(0, 256)), e, int(L.S[p, i]))
        return None
    if kind == "widest":        # the last-folded input at the bottom, the others at the top
        for p in range(P):
            L.put(p, i, ONES - int(rng.integers(0, 256)), lo + spread, sgn)
        return L.put(order[-1], i, L.rand64() | TOP, lo, ls if ls is not None else int(rng.integers(0, 2)))
    if kind == "topword":       # the fold's first add cancels 7..31 bits of the top word
        a, b = pools["deep"][c % 2]
        j = (c * 7919) % a.size
        for p, x in ((order[0], a), (order[1], b)):
            m, e, s = fields(x[j:j + 1])
            L.put(p, i, int(m[0]), int(e[0]) - BIAS + lo + 10, int(s[0]))
        return None
    if kind == "seam":          # the fold's first add meets a gap of 62..65
        a, b, idx = pools["seam"]
        j = int(idx[(c * 31) % idx.size])
        for p, x in ((order[0], a), (order[1], b)):
            m, e, s = fields(x[j:j + 1])
            L.put(p, i, int(m[0]), int(e[0]), ls if ls is not None else int(s[0]))
        return None
    if kind == "qnan":
        return L.put(posm, i, 0xC000000000000000 | int(rng.integers(1, 1 << 40)), EMAX, sgn)
    if kind == "snan":
        return L.put(posm, i, TOP | int(rng.integers(1, 1 << 40)), EMAX, sgn)
    if kind == "inf":
        return L.put(posm, i, TOP, EMAX, sgn)
    if kind == "denormal":
        return L.put(posm, i, (L.rand64() >> (1 + int(rng.integers(0, 20)))) | 1, 0, sgn)
    if kind == "pseudo":
        return L.put(posm, i, L.rand64() | TOP, 0, sgn)
    if kind == "unnormal":
        return L.put(posm, i, (L.rand64() & ~TOP) | 1, max(int(L.E[posm, i]), 1), sgn)
    if kind == "overflow":      # one sign, within two binades of overflow
        for p in range(P):
            L.put(p, i, int(L.M[p, i]), EMAX - 3 + int(rng.integers(0, 2)), sgn)
        return L.put(posm, i, ONES - int(rng.integers(0, 256)), EMAX - 1, sgn)
    assert kind == "grid", kind
    if ls is not None:          # one sign: denormals up to the member, small normals after
        for p in range(P):
            if p <= posm:
                L.put(p, i, (L.rand64() >> 1) | (1 << 60), 0, ls)
            else:
                L.put(p, i, int(L.M[p, i]), 1 + int(rng.integers(0, 20)), ls)
        return None
    for p in range(P):          # small normals; the member cancels the running sum
        L.put(p, i, int(L.M[p, i]), 3 + int(rng.integers(0, 23)), int(L.S[p, i]))   # onto the grid
    pm, pe, ps = L.running("sum", i, order, k)
    bit = max(63 - pe - (c // nk) % 3, 0)      # the difference's top bit: exponent 0, -1, -2
    delta = (1 << bit) + int(rng.integers(0, 1 << bit))
    return L.put(posm, i, pm + delta if pm + delta <= ONES else pm - delta, pe, ps ^ 1)


@functools.lru_cache(maxsize=None)
def sum_case(P: int):
    """(srcs, runs, event): P arrays of N_SUM elements; runs[r] = (class,
    repeat, density, lanes) with the partial last run appended; event[i]: the
    element was made an event lane (kind[i] names it)."""
    spread, gmin, gmax = gate()
    runs = sum_runs() + [("near", 2, "few", TAIL_EVENTS)]
    L = _Lanes(P, N_SUM, 0xA7E0 + P)
    _base_significands(L, 0x5100 + P)
    a, b = _pairs("unit")
    d = fields(a)[1] - fields(b)[1]
    plain = np.flatnonzero(~np.isin(d, (62, 63, 64, 65)))
    pools = {"deep": (_deep_cancel_pairs(0, 4096), _deep_cancel_pairs(1, 4096)),
             "seam": (a, b, np.flatnonzero(np.isin(d, (62, 63, 64, 65))))}
    # the near windows' lower ends: the gate's lower edge, its upper edge, around 1
    windows = (gmin, gmax - spread, BIAS - 12)
    counter = {cls: 0 for cls in CLASSES}
    rng = np.random.default_rng(0xBA5E + P)
    for r, (cls, rep, dens, lanes) in enumerate(runs):
        sl = slice(RUN * r, min(RUN * (r + 1), N_SUM))
        w = sl.stop - sl.start
        lo = windows[(r + rep) % 3]
        if cls in ("near", "same_near"):
            # 20 binades of the window's 25: a running sum (three binades up at
            # most) and an event's operand stay inside the gate
            L.E[:, sl] = lo + rng.integers(0, 20, (P, w))
        elif cls == "full" and rep == 1:
            # below the gate: normal, within its spread, exponents under kNearEmin.
            # One sign per lane (no running sum leaves the normal range by
            # itself) but for every eighth lane, random signs in the top binades
            L.E[:, sl] = gmin - 1 - spread + rng.integers(0, spread + 1, (P, w))
            mixed = np.arange(w) % 8 == 3
            L.E[:, sl][:, mixed] = gmin - 6 + rng.integers(0, 6, (P, int(mixed.sum())))
            L.S[:, sl] = np.where(mixed, L.S[:, sl], L.S[0, sl])
        elif cls == "full":
            L.E[:, sl] = BIAS - 20 + rng.integers(0, 41, (P, w))
            L.E[0, sl.start], L.E[1, sl.start + 1] = BIAS - 20, BIAS + 20   # wider than the spread
            L.E[1, sl.start], L.E[0, sl.start + 1] = BIAS + 20, BIAS - 20
        else:                   # same: _pairs' operands, gaps up to 200 binades
            for p in range(P):
                j = plain[(np.arange(w) * (p // 2 + 1) + 97 * r + 11 * p) % plain.size]
                m, e, _ = fields((a if p % 2 else b)[j])
                L.M[p, sl], L.E[p, sl] = m, e
        if cls in ("same", "same_near"):
            L.S[:, sl] = L.S[0, sl]
        for i in lanes:
            c = counter[cls]
            counter[cls] += 1
            kind = SUM_KINDS[cls][c % len(SUM_KINDS[cls])]
            L.event[sl.start + i], L.kind[sl.start + i] = True, kind
            _sum_event(L, sl.start + i, cls, kind, c, lo, spread, pools)
    return L.arrays(), runs, L.event, L.kind


def _prod_event(L, i, kind, c):
    posm, order, k = L.aim(c, len(PROD_KINDS))
    rng = L.rng
    first = order[0] if k else order[1]
    sgn = int(rng.integers(0, 2))
    if kind == "qnan":
        return L.put(posm, i, 0xC000000000000000 | int(rng.integers(1, 1 << 40)), EMAX, sgn)
    if kind == "snan":
        return L.put(posm, i, TOP | int(rng.integers(1, 1 << 40)), EMAX, sgn)
    if kind == "zeroinf":
        L.put(first, i, 0, 0, sgn)
        return L.put(posm, i, TOP, EMAX, int(rng.integers(0, 2)))
    if kind == "wrap":          # the product is 2^127 - r, r < 2^62: all ones rounded up
        for _ in range(64):
            pm = L.running("prod", i, order, k)[0]
            x = ((1 << 127) - 1) // pm
            if TOP <= x <= ONES and (1 << 127) - pm * x < (1 << 62):
                return L.put(posm, i, x, int(L.E[posm, i]), sgn)
            L.put(first, i, L.rand64() | TOP, int(L.E[first, i]), int(L.S[first, i]))
        raise AssertionError("no rounding carry found")
    t = int(rng.integers(0, 31))
    if kind == "underflow":     # 2^-8192 times 2^(-8191 - t): the denormal grid
        L.put(first, i, int(L.M[first, i]), 8191, int(L.S[first, i]))
        pe = L.running("prod", i, order, k)[1]
        L.put(posm, i, int(L.M[posm, i]), max(BIAS - pe - t, 1), sgn)
        if order[-1] not in (posm, first):      # and back to normal
            L.put(order[-1], i, int(L.M[order[-1], i]), BIAS + 8300, int(L.S[order[-1], i]))
        return None
    assert kind == "overflow", kind
    L.put(first, i, int(L.M[first, i]), BIAS + 8191, int(L.S[first, i]))
    pe = L.running("prod", i, order, k)[1]
    return L.put(posm, i, int(L.M[posm, i]), EMAX + BIAS - pe - 1 + t % 3, sgn)


@functools.lru_cache(maxsize=None)
def prod_case(P: int):
    """(srcs, event): factors in [1/2, 2) -- every product normal, all mul_fast
    -- in runs of no, a few (FEW["full"]) and 64 event lanes, twice, and 37."""
    L = _Lanes(P, N_PROD, 0x9D0D + P)
    _base_significands(L, 0x7200 + P)
    L.E[:] = BIAS - 1 + np.random.default_rng(0x7201 + P).integers(0, 2, (P, N_PROD))
    c = 0
    for r in range(n_runs(N_PROD)):
        dens = DENSITIES[r % 3]
        lanes = {"none": (), "few": FEW["full"][(r // 3) % 2], "all": tuple(range(RUN))}[dens]
        if r == n_runs(N_PROD) - 1:
            lanes = TAIL_EVENTS
        for i in lanes:
            kind = PROD_KINDS[c % len(PROD_KINDS)]
            L.event[RUN * r + i], L.kind[RUN * r + i] = True, kind
            _prod_event(L, RUN * r + i, kind, c)
            c += 1
    return L.arrays(), L.event, L.kind


@functools.lru_cache(maxsize=None)
def minmax_case(P: int):
    """(srcs, unordered lanes): draws of TIE_POOL, a narrower pool in a third
    of the elements (ties at every P), in runs with no unordered element, with
    a few (FEW["same"]) and with one in every element, twice, and 37."""
    n = N_MINMAX
    sp = O.value_bytes(raw_random(40 * n, 900, "any")).reshape(-1, 10)
    m, e, _ = fields(O.from_value_bytes("longdouble", sp.reshape(-1)))
    specials = sp[unordered(m, e)]
    raws = []
    for p in range(P):
        k = O.splitmix64(700 + p, n)
        raw = TIE_POOL[(k % np.uint64(12)).astype(np.int64)].copy()
        narrow = (k >> np.uint64(8)) % np.uint64(3) == 0
        raw[narrow] = TIE_POOL[((k[narrow] >> np.uint64(16)) % np.uint64(2)).astype(np.int64)]
        raws.append(raw)
    un = np.zeros(n, bool)
    for r in range(n_runs(n)):
        dens = DENSITIES[r % 3]
        lanes = {"none": (), "few": FEW["same"][(r // 3) % 2], "all": tuple(range(RUN))}[dens]
        if r == n_runs(n) - 1:
            lanes = TAIL_EVENTS
        for i in lanes:
            j = RUN * r + i
            raws[(j // 3) % P][j] = specials[(7 * j) % specials.shape[0]]
            un[j] = True
    return [np.ascontiguousarray(O.from_value_bytes("longdouble", x.reshape(-1))) for x in raws], un


def inputs(op: str, P: int):
    """the P input arrays of `op` ("sum", "prod", "max", "min")"""
    return {"sum": sum_case, "prod": prod_case}.get(op, minmax_case)(P)[0]


@functools.lru_cache(maxsize=None)
def want(op: str, P: int):
    """every member's expected target: the oracle's reduce-to-all"""
    return O.to_all("longdouble", op, inputs(op, P))
