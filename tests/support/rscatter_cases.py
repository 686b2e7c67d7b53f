"""rscatter_cases.py -- TEST INFRASTRUCTURE of the reduce-scatter tests
(osgpu_reduce_scatter, osgpu_combine_shifted): inputs, expected values and the
PE-thread driver.

Expected values are never a second fold: the reduce-to-all oracle
(oracle.to_all, or tests/support/half_ref.py for half / bfloat16) runs over
the full P * n element sources and member m's block m is sliced out of
member m's result -- the identity include/osgpu_reduce.h Part 1d states.
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from support import half_ref as R

# the (type, op) pairs the issue names for the GPU tests
PAIRS = [("int", "sum"), ("short", "min"), ("double", "sum"), ("float", "prod"),
         ("complexf", "prod"), ("half", "sum"), ("long", "xor")]
SHIFT_U = 2          # vectors per lane per input of combine_shift_kernel (combine.hip OSGPU_SHIFT_U)
TILE_VECTORS = 64 * SHIFT_U


def esize(t: str) -> int:
    if t in R.TYPES:
        return 2
    return 16 if t == "longdouble" else np.dtype(O.NP_DTYPE[t]).itemsize


def dtype(t: str):
    return np.uint16 if t in R.TYPES else O.NP_DTYPE[t]


def inputs(t: str, op: str, npes: int, n: int, seed: int):
    """npes arrays of n elements: edge values mixed in (NaNs with payloads,
    signed zeros, infinities, extremes)."""
    if t in R.TYPES:
        return [np.where(np.arange(n) % 3 == 0, np.resize(R.special_table(t, 512, seed + pe), n),
                         R.order_values(t, n, seed * 131 + pe)).astype(np.uint16)
                for pe in range(npes)]
    dist = "edge" if t not in O.INT_TYPES else ("prod" if op == "prod" else "bits")
    return O.team_inputs(t, npes, n, seed, dist)


def fold_left(t: str, op: str, srcs):
    """srcs[0] op srcs[1] op ... left to right: the reduce-to-all of member 0."""
    if t in R.TYPES:
        return R.fold(t, op, list(range(len(srcs))), srcs)
    return O.to_all(t, op, list(srcs))[0]


def to_all(t: str, op: str, sources, PE_start=0, logPE_stride=0, PE_size=None):
    """Per-PE reduce-to-all results (None outside the active set)."""
    npes = len(sources)
    if PE_size is None:
        PE_size = npes
    if t not in R.TYPES:
        return O.to_all(t, op, list(sources), PE_start, logPE_stride, PE_size)
    members = O.active_set(PE_start, logPE_stride, PE_size)
    out = [None] * npes
    for pe in members:
        out[pe] = R.fold(t, op, O.fold_order(pe, PE_start, logPE_stride, PE_size), sources)
    return out


def expected(t: str, op: str, sources, nreduce: int, PE_start=0, logPE_stride=0, PE_size=None):
    """{pe: block m of member m's reduce-to-all over the P * nreduce sources}."""
    if PE_size is None:
        PE_size = len(sources)
    full = to_all(t, op, sources, PE_start, logPE_stride, PE_size)
    members = O.active_set(PE_start, logPE_stride, PE_size)
    return {pe: full[pe][m * nreduce:(m + 1) * nreduce].copy() for m, pe in enumerate(members)}


def same_bits(t: str, got: np.ndarray, want: np.ndarray):
    """Index of the first element whose value bytes differ, or None."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, esize(t))
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, esize(t))
    if t == "longdouble":
        g, w = g[:, :10], w[:, :10]
    bad = np.flatnonzero((g != w).any(axis=1))
    return None if bad.size == 0 else int(bad[0])


def run(tm, t: str, op: str, target_off, source_off: int, nreduce: int, PE_start: int = 0,
        logPE_stride: int = 0, PE_size: int | None = None):
    """Every member of the set calls osgpu_reduce_scatter on its own thread
    (tests/support/team.py Team); target_off: one offset, or {pe: offset}."""
    if PE_size is None:
        PE_size = tm.npes
    members = O.active_set(PE_start, logPE_stride, PE_size)
    fn = tm.osgpu.reduce_scatter(t, op)
    pwrk = (ctypes.c_byte * 4096)()
    toff = (lambda pe: target_off[pe]) if isinstance(target_off, dict) else (lambda pe: target_off)
    tm._on_members(members, lambda pe: fn(
        tm.ptr(pe, toff(pe)), tm.ptr(pe, source_off), nreduce, PE_start, logPE_stride, PE_size,
        ctypes.addressof(pwrk), tm.psync_ptr(pe)))
    return members
