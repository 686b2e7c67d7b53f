"""loc_cases.py -- TEST INFRASTRUCTURE of the max / min with location tests
(osgpu_reduce_loc, osgpu_team_loc): inputs with ties and NaNs, expected values
and indices, and the PE-thread driver.

Expected VALUES are never a second fold: uniform_cases.value, i.e. the
reduce-to-all oracle at PE_start (half_ref.fold for the 16-bit types) -- the
identity include/osgpu_reduce.h Part 1h states.  Expected INDICES are the
header's closed form in numpy (index): among the members after the last member
holding a NaN in that element (or that last member alone when it is the last
of the set), the minimum index of those whose value compares equal to the
expected value.  literal_fold is the definition written out step by step; only
tests/test_loc_ref.py uses it, to check the closed form.
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from support import half_ref as R
from support import uniform_cases as U
from support.rscatter_cases import dtype, esize, inputs, same_bits  # noqa: F401  (shared helpers)

TYPES = ("short", "int", "long", "longlong", "float", "double", "half", "bfloat16")
OPS = ("max", "min")
PAIRS = [(t, op) for t in TYPES for op in OPS]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
TILE_GROUPS = 256    # groups per tile of team_loc_vec_kernel: one per lane (team.hip kLocBlock)

_F16 = {"half": [0xFC00, 0xBC00, 0x8000, 0x0000, 0x3C00, 0x7C00, 0x7E00],
        "bfloat16": [0xFF80, 0xBF80, 0x8000, 0x0000, 0x3F80, 0x7F80, 0x7FC0]}


def group(t: str) -> int:
    """Elements one lane step of the kernel covers: max(16 / size, 4)."""
    return max(16 // esize(t), 4)


def tile_elems(t: str) -> int:
    """Elements per tile of team_loc_vec_kernel: 256 groups."""
    return TILE_GROUPS * group(t)


def is_float(t: str) -> bool:
    return t in ("float", "double") or t in R.TYPES


def numeric(t: str, a) -> np.ndarray:
    """The values the comparisons see (16-bit patterns widened to float32)."""
    return R.widen(t, a) if t in R.TYPES else np.asarray(a)


def isnan(t: str, a) -> np.ndarray:
    if t in R.TYPES:
        return R.isnan(t, a)
    return np.isnan(a) if is_float(t) else np.zeros(np.shape(a), bool)


def alphabet(t: str) -> np.ndarray:
    """Floating types {-inf, -1, -0.0, +0.0, 1, +inf, NaN}; integers the
    type's minimum and maximum, -1, 0, 1."""
    if t in R.TYPES:
        return np.array(_F16[t], np.uint16)
    if is_float(t):
        return np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], dtype(t))
    ii = np.iinfo(dtype(t))
    return np.array([ii.min, -1, 0, 1, ii.max], dtype(t))


def tie_values(t: str, P: int, n: int, seed: int):
    """P arrays of n draws from the alphabet: ties, NaNs and signed zeros in
    most elements; every fourth element holds member 0's draw on every member
    but the first of a floating type's middle ones (a tie of all, or of all
    after a NaN)."""
    rng = np.random.default_rng(seed)
    a = alphabet(t)
    draws = [rng.integers(0, len(a), n) for _ in range(P)]
    same = np.arange(n) % 4 == 1
    for j in range(1, P):
        if not (is_float(t) and P >= 3 and j == 1):
            draws[j][same] = draws[0][same]
    return [a[d] for d in draws]


def tie_indices(P: int, n: int, seed: int):
    """P int32 arrays; element k takes pattern k mod 3: descending with the
    member; seeded random with duplicates and negatives; INT_MIN / INT_MAX at
    chosen members (the first member INT_MAX, a middle one INT_MIN or the last
    INT_MIN, by k) over small random ones."""
    rng = np.random.default_rng(seed ^ 0x10C)
    k = np.arange(n)
    small = [rng.integers(-4, 5, n).astype(np.int32) for _ in range(P)]
    out = []
    for j in range(P):
        a = small[j].copy()
        desc = (k % 3) == 0
        a[desc] = (10 * (P - j) + (k[desc] % 7)).astype(np.int32)
        ext = (k % 3) == 2
        if j == 0:
            a[ext & (k % 2 == 0)] = INT_MAX
        if j == P // 2:
            a[ext & (k % 4 == 1)] = INT_MIN
        if j == P - 1:
            a[ext & (k % 4 == 3)] = INT_MIN
        out.append(a)
    return out


def member_pes(PE_start=0, logPE_stride=0, PE_size=1):
    return O.active_set(PE_start, logPE_stride, PE_size)


def const_indices(member_locs, n: int):
    """The index arrays of the form without index sources."""
    return [np.full(n, m, np.int32) for m in member_locs]


def value(t: str, op: str, values):
    """The expected value array: the uniform reduce's (the oracle's)."""
    if len(values) == 1:
        return np.array(values[0], copy=True)
    return U.value(t, op, list(values))


def index(t: str, op: str, values, locs, want_value=None) -> np.ndarray:
    """The expected index array by the closed form."""
    P, n = len(values), len(values[0])
    v = value(t, op, values) if want_value is None else want_value
    f = np.stack([numeric(t, x) for x in values])
    nan = np.stack([isnan(t, x) for x in values])
    loc = np.stack([np.asarray(x, np.int64) for x in locs])
    j = np.arange(P)[:, None]
    last_nan = np.where(nan, j, -1).max(axis=0)
    with np.errstate(invalid="ignore"):
        holder = (j > last_nan[None, :]) & (f == numeric(t, v)[None, :])
    # the last member holds the NaN: it is the only candidate
    holder[P - 1, last_nan == P - 1] = True
    assert holder.any(axis=0).all(), "the expected value has no holder"
    return np.where(holder, loc, 2 ** 40).min(axis=0).astype(np.int32)


def expected(t: str, op: str, values, locs):
    v = value(t, op, values)
    return v, index(t, op, values, locs, v)


def literal_fold(t: str, op: str, values, locs):
    """(value array, index array) by the definition, one step per member."""
    P, n = len(values), len(values[0])
    f = [numeric(t, x) for x in values]
    v = np.array(values[0], copy=True)
    fv = np.array(f[0], copy=True)
    i = np.array(locs[0], np.int32, copy=True)
    for j in range(1, P):
        b, fb, ib = np.asarray(values[j]), f[j], np.asarray(locs[j], np.int32)
        with np.errstate(invalid="ignore"):
            keep = fv > fb if op == "max" else fv < fb
            tie = fv == fb
        i = np.where(keep, i, np.where(tie, np.minimum(i, ib), ib)).astype(np.int32)
        v = np.where(keep, v, b)
        fv = np.where(keep, fv, fb)
    return v, i


def assert_discriminating(t: str, op: str, values, locs):
    """P >= 3: some element's expected index is neither the FIRST nor the
    LAST holder's (a "first wins" / "last wins" kernel fails there), and for
    floating types some element has a NaN in a middle member."""
    P = len(values)
    if P < 3:
        return
    v, idx = expected(t, op, values, locs)
    f = np.stack([numeric(t, x) for x in values])
    nan = np.stack([isnan(t, x) for x in values])
    j = np.arange(P)[:, None]
    last_nan = np.where(nan, j, -1).max(axis=0)
    with np.errstate(invalid="ignore"):
        holder = (j > last_nan[None, :]) & (f == numeric(t, v)[None, :])
    some = holder.any(axis=0)
    first = np.where(holder, j, P).min(axis=0).clip(0, P - 1)
    last = np.where(holder, j, -1).max(axis=0).clip(0, P - 1)
    loc = np.stack([np.asarray(x, np.int32) for x in locs])
    k = np.arange(len(idx))
    odd = some & (idx != loc[first, k]) & (idx != loc[last, k])
    assert odd.any(), f"{t} {op} P={P}: every expected index is the first or last holder's"
    if is_float(t):
        assert nan[1:P - 1].any(), f"{t} {op} P={P}: no NaN in a middle member"


def tie_case(t: str, op: str, P: int, n: int, seed: int):
    """(values, indices) of the tie inputs, checked to discriminate."""
    vals, locs = tie_values(t, P, n, seed), tie_indices(P, n, seed)
    assert_discriminating(t, op, vals, locs)
    return vals, locs


def run(tm, t: str, op: str, target_off, loc_target_off, source_off, loc_source_off, nreduce: int,
        PE_start: int = 0, logPE_stride: int = 0, PE_size: int | None = None):
    """Every member of the set calls osgpu_reduce_loc on its own thread
    (tests/support/team.py Team); loc_source_off None: no index source."""
    if PE_size is None:
        PE_size = tm.npes
    members = O.active_set(PE_start, logPE_stride, PE_size)
    fn = tm.osgpu.reduce_loc(t, op)
    pwrk = (ctypes.c_byte * 4096)()
    tm._on_members(members, lambda pe: fn(
        tm.ptr(pe, target_off), tm.ptr(pe, loc_target_off), tm.ptr(pe, source_off),
        None if loc_source_off is None else tm.ptr(pe, loc_source_off), nreduce, PE_start,
        logPE_stride, PE_size, ctypes.addressof(pwrk), tm.psync_ptr(pe)))
    return members
