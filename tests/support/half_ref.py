"""half_ref.py -- TEST INFRASTRUCTURE: numpy restatement of the half /
bfloat16 reduce-to-all arithmetic (include/osgpu_reduce.h Part 1c) on uint16
arrays of bit patterns.  No torch, no library code: widen (exact), ONE
float32 operation, integer round-to-nearest-even narrowing, the NaN rule at
the element's width, compare + select for max / min, and the fold.
"""
from __future__ import annotations

import numpy as np

TYPES = ("half", "bfloat16")
OPS = ("sum", "prod", "max", "min")
QUIET = {"half": 0x0200, "bfloat16": 0x0040}
DEFNAN = {"half": 0xFE00, "bfloat16": 0xFFC0}
EXPMASK = {"half": 0x7C00, "bfloat16": 0x7F80}


def _u16(x):
    return np.ascontiguousarray(x, dtype=np.uint16)


def isnan(t: str, x) -> np.ndarray:
    return (_u16(x) & 0x7FFF) > EXPMASK[t]


def widen(t: str, x) -> np.ndarray:
    """The float32 of every pattern (exact; NaN payloads shifted up)."""
    x = _u16(x).astype(np.uint32)
    if t == "bfloat16":
        return (x << 16).view(np.float32)
    s = (x & 0x8000) << 16
    e = (x >> 10) & 0x1F
    m = x & 0x3FF
    sub = (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)  # m * 2^-24, exact
    out = np.where(e == 0, sub, np.where(e == 31, 0x7F800000 | (m << 13),
                                         ((e + 112) << 23) | (m << 13)))
    return (s | out).astype(np.uint32).view(np.float32)


def narrow(t: str, f) -> np.ndarray:
    """Round-to-nearest-even narrowing of float32 values, in integers; NaNs
    narrow to some NaN (callers replace them)."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    if t == "bfloat16":
        r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
        nan = (u & 0x7FFFFFFF) > 0x7F800000
        return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)
    s = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    e = (a >> 23).astype(np.int64)
    m = a & 0x7FFFFF
    # normal results: drop 13 bits of the significand, the carry steps the exponent
    y = a - 0x38000000
    normal = (y + 0xFFF + ((y >> 13) & 1)) >> 13
    # below 2^-14: the 24-bit significand shifted right by 126 - e, kept bits RNE
    sig = np.where(e > 0, m | 0x800000, m)
    sh = np.clip(126 - np.maximum(e, 1), 0, 40).astype(np.uint64)
    q = sig >> sh
    rem = sig & ((np.uint64(1) << sh) - np.uint64(1))
    halfway = np.uint64(1) << (np.maximum(sh, 1) - np.uint64(1))
    up = (rem > halfway) | ((rem == halfway) & ((q & 1) == 1))
    tiny = q + up.astype(np.uint64)
    out = np.where(a > 0x7F800000, 0x7E00,
                   np.where(a >= 0x47800000, 0x7C00, np.where(a < 0x38800000, tiny, normal)))
    return (s | out).astype(np.uint16)


def op2(t: str, op: str, a, b) -> np.ndarray:
    """a OP b element-wise, a the first operand (the accumulator)."""
    a, b = _u16(a), _u16(b)
    fa, fb = widen(t, a), widen(t, b)
    with np.errstate(all="ignore"):
        if op == "max":
            return np.where(fa > fb, a, b)
        if op == "min":
            return np.where(fa < fb, a, b)
        r = (fa + fb) if op == "sum" else (fa * fb)
    assert r.dtype == np.float32
    out = narrow(t, r)
    na, nb = isnan(t, a), isnan(t, b)
    rule = np.where(na, a | QUIET[t], np.where(nb, b | QUIET[t], DEFNAN[t])).astype(np.uint16)
    return np.where(np.isnan(r), rule, out).astype(np.uint16)


def fold(t: str, op: str, order, sources) -> np.ndarray:
    """sources[order[0]] first, then the others in `order`, one rounding a step."""
    acc = _u16(sources[order[0]]).copy()
    for k in order[1:]:
        acc = op2(t, op, acc, sources[k])
    return acc


def member_order(q: int, P: int):
    """Fold order of member q of a P-member set: q first, the others ascending."""
    return [q] + [j for j in range(P) if j != q]


def to_all(t: str, op: str, sources):
    """Every member's result, each in its own fold order."""
    P = len(sources)
    return [fold(t, op, member_order(q, P), sources) for q in range(P)]


def special_table(t: str, n: int = 512, seed: int = 0x16B17) -> np.ndarray:
    """The fixed operand table: signed zeros, subnormal / normal extremes, 1,
    the largest finite, infinities, quiet and signalling NaNs with distinct
    payloads, every exponent's first and last significand, seeded random fill."""
    mbits = 10 if t == "half" else 7
    ebits = 5 if t == "half" else 8
    mmax = (1 << mbits) - 1
    emax = (1 << ebits) - 1
    one = ((emax >> 1) << mbits)
    pos = [0, 1, mmax, 1 << mbits, one, ((emax - 1) << mbits) | mmax, emax << mbits,
           (emax << mbits) | (1 << (mbits - 1)), (emax << mbits) | (1 << (mbits - 1)) | 5,
           (emax << mbits) | 1, (emax << mbits) | 0x15, (emax << mbits) | (mmax >> 1)]
    v = []
    for p in pos:
        v += [p, p | 0x8000]
    v = list(dict.fromkeys(v))
    ex = []
    for e in range(emax):
        for m in (0, mmax):
            ex += [(e << mbits) | m, 0x8000 | (e << mbits) | m]
    ex = [x for x in dict.fromkeys(ex) if x not in v]
    # a short table keeps an even sample of the exponents (the whole range,
    # not its low end) and at least a quarter of seeded random patterns
    room = max(0, n - n // 4 - len(v))
    if len(ex) > room:
        ex = [ex[(i * len(ex)) // room] for i in range(room)]
    v = (v + ex)[:n]
    rng = np.random.default_rng(seed)
    fill = rng.integers(0, 1 << 16, size=max(0, n - len(v)), dtype=np.uint32)
    return np.concatenate([np.array(v, dtype=np.uint32), fill]).astype(np.uint16)[:n]


def order_values(t: str, n: int, seed: int) -> np.ndarray:
    """Patterns whose sums depend on the fold order: ones, last-bit-scale
    terms, a large term, a few specials."""
    rng = np.random.default_rng(seed)
    if t == "half":
        pool = np.array([0x3C00, 0x1000, 0x1001, 0x9000, 0x6BFF, 0xEBFF, 0x0001, 0x83FF, 0x3C01,
                         0x7BFF, 0x0000, 0x8000, 0x4248, 0xB555], np.uint16)
    else:
        pool = np.array([0x3F80, 0x3B80, 0x3B81, 0xBB80, 0x7E7F, 0xFE7F, 0x0001, 0x807F, 0x3F81,
                         0x7F7F, 0x0000, 0x8000, 0x4049, 0xBEAB], np.uint16)
    v = pool[rng.integers(0, pool.size, size=n)]
    r = rng.integers(0, 1 << 16, size=n, dtype=np.uint32).astype(np.uint16)
    pick = rng.random(n) < 0.25
    r = np.where(isnan(t, r), 0x3C00 if t == "half" else 0x3F80, r).astype(np.uint16)
    return np.where(pick, r, v).astype(np.uint16)
