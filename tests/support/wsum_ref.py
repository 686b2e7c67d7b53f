"""wsum_ref.py -- TEST INFRASTRUCTURE: numpy restatement of the
float-accumulated half / bfloat16 sum (include/osgpu_reduce.h Part 1i) on bit
patterns.  No torch, no library code: half_ref.widen (exact), a stepwise
float32 add with the NaN rule applied on uint32 views, half_ref.narrow for
non-NaN accumulators and the header's truncation for NaN ones.

Also the inputs of the wsum tests: seeded order-sensitive values with elements
built in that tell this sum from the per-step one (half_ref.fold ascending),
and the NaN / overflow table.
"""
from __future__ import annotations

import numpy as np

from support import half_ref as R

TYPES = R.TYPES
PAIRS = [(t, o) for t in TYPES for o in (t, "float")]
QUIET32, DEFNAN32 = np.uint32(0x00400000), np.uint32(0xFFC00000)
GROUP = 8            # elements one lane step of team_wsum_vec_kernel covers
TILE = 256 * GROUP   # elements per tile: one group per lane of 256


def _u32(f) -> np.ndarray:
    return np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)


def isnan32(u) -> np.ndarray:
    return (np.asarray(u, np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def widen(t: str, x) -> np.ndarray:
    """uint32 patterns of the float32 of every 16-bit pattern, NaNs exact."""
    return R.widen(t, x).view(np.uint32).copy()


def add(acc, b) -> np.ndarray:
    """One float32 add of uint32 patterns, acc the first operand: a NaN
    accumulator stays quieted, else a NaN operand quieted, else inf - inf the
    negative default NaN."""
    acc, b = np.asarray(acc, np.uint32), np.asarray(b, np.uint32)
    with np.errstate(all="ignore"):
        r = acc.view(np.float32) + b.view(np.float32)
    assert r.dtype == np.float32
    ru = r.view(np.uint32)
    rule = np.where(isnan32(acc), acc | QUIET32, np.where(isnan32(b), b | QUIET32, DEFNAN32))
    return np.where(isnan32(ru), rule, ru).astype(np.uint32)


def narrow(t: str, acc) -> np.ndarray:
    """uint16 patterns: RNE for non-NaN accumulators, NaNs truncated."""
    acc = np.asarray(acc, np.uint32)
    nan = isnan32(acc)
    rne = R.narrow(t, np.where(nan, np.uint32(0), acc).astype(np.uint32).view(np.float32))
    if t == "bfloat16":
        cut = acc >> 16
    else:
        cut = ((acc >> 16) & 0x8000) | 0x7C00 | ((acc >> 13) & 0x3FF)
    return np.where(nan, cut, rne).astype(np.uint16)


def accumulate(t: str, sources, carry=None) -> np.ndarray:
    """The float accumulator (uint32 patterns) after all sources, ascending;
    carry (uint32 patterns): it starts the accumulator and sources[0] is added."""
    if carry is None:
        acc = widen(t, sources[0])
        rest = sources[1:]
    else:
        acc, rest = np.asarray(carry, np.uint32).copy(), sources
    for s in rest:
        acc = add(acc, widen(t, s))
    return acc


def wsum(t: str, out_t: str, sources, carry=None) -> np.ndarray:
    """The expected target: uint16 patterns (out_t == t) or uint32 patterns of
    the float accumulator (out_t == "float")."""
    acc = accumulate(t, sources, carry)
    return acc if out_t == "float" else narrow(t, acc)


def chunked(t: str, out_t: str, sources, chunk=8, float_carry=True) -> np.ndarray:
    """The fold in chunks of `chunk` sources.  float_carry: the accumulator is
    carried as it is (the library's way); False: it is rounded to 16 bits and
    widened again between chunks (a wrong builder's way)."""
    acc = None
    for lo in range(0, len(sources), chunk):
        acc = accumulate(t, sources[lo:lo + chunk], acc)
        if not float_carry and lo + chunk < len(sources):
            acc = widen(t, narrow(t, acc))
    return acc if out_t == "float" else narrow(t, acc)


def per_step(t: str, sources) -> np.ndarray:
    """What osgpu_reduce_uniform's sum gives: one rounding a step."""
    return R.fold(t, "sum", list(range(len(sources))), sources)


# ---------------------------------------------------------------- the inputs
_BIG = {"half": 0x6800, "bfloat16": 0x4380}   # 2048.0 / 256.0: ulp 2 in either format
_ONE = {"half": 0x3C00, "bfloat16": 0x3F80}


def inputs(t: str, P: int, n: int, seed: int):
    """P uint16 arrays of n patterns: half_ref.order_values (NaN-free but for
    its pool's specials), and every 5th element the pattern big, 1, 1, 1, ...
    whose float sum differs from the per-step one for P >= 3 (half 2048 + 1 +
    1 + 1 = 2052 against 2048, bfloat16 256 + 1 + 1 + 1 = 260 against 256)."""
    out = [R.order_values(t, n, seed + 7 * j).copy() for j in range(P)]
    k = np.arange(n) % 5 == 2
    for j in range(P):
        out[j][k] = _BIG[t] if j == 0 else _ONE[t]
    return out


def assert_discriminating(t: str, sources):
    """P >= 3: some element's float-accumulated sum, narrowed, is not the
    per-step sum's pattern."""
    if len(sources) < 3:
        return
    assert (wsum(t, t, sources) != per_step(t, sources)).any(), \
        f"{t} P={len(sources)}: the inputs do not tell the sums apart"


def nan_table(t: str, P: int):
    """P arrays: half_ref.special_table patterns with a NaN placed at each
    member position in turn (quiet and signalling), +-inf pairs at every pair
    of positions, and the accumulator overflow followed by -inf."""
    base = R.special_table(t, 96)
    fin = base[~R.isnan(t, base) & ((base & 0x7FFF) < R.EXPMASK[t])]
    mx = R.EXPMASK[t] - 1                      # the largest finite
    pinf, ninf = R.EXPMASK[t], R.EXPMASK[t] | 0x8000
    snan, qnan = R.EXPMASK[t] | 0x15, R.EXPMASK[t] | R.QUIET[t] | 5
    cols = []
    for j in range(P):                           # one NaN, at member j
        for nanv in (snan, qnan | 0x8000):
            col = [int(fin[(3 * j + i) % fin.size]) for i in range(P)]
            col[j] = nanv
            cols.append(col)
    for j in range(P):                           # two NaNs: member j's wins over the last's
        col = [int(fin[(5 * j + i) % fin.size]) for i in range(P)]
        col[P - 1] = qnan
        col[j] = snan | 0x8000 if j < P - 1 else qnan
        cols.append(col)
    for i in range(P):                           # +inf at i, -inf at j: the default NaN
        for j in range(P):
            if i != j:
                col = [_ONE[t]] * P
                col[i], col[j] = pinf, ninf
                cols.append(col)
    col = [mx] * P                               # overflow of the accumulator, then -inf
    col[P - 1] = ninf
    cols.append(col)
    cols.append([pinf] + [mx] * (P - 1))
    cols.append([int(x) for x in base[:P]])
    # the whole special table against itself rotated by the member
    arr = np.array(cols, np.uint16).T            # (P, ncols)
    rot = np.stack([np.roll(base, 7 * j) for j in range(P)])
    return [np.concatenate([arr[j], rot[j]]).astype(np.uint16) for j in range(P)]
