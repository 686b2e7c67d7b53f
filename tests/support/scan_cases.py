"""scan_cases.py -- TEST INFRASTRUCTURE of the prefix-scan tests (osgpu_scan,
osgpu_team_scan): inputs, expected values and the PE-thread driver.

Expected values are never a second fold.  The inclusive result of member m
of the set (PE_start, logPE_stride, PE_size) is what the reduce-to-all oracle
(oracle.to_all) leaves at PE_start over the SUB-SET (PE_start, logPE_stride,
m + 1): member 0's fold order there is the ascending one, 0..m -- the identity
include/osgpu_reduce.h Part 1f states.  For half / bfloat16 it is
tests/support/half_ref.fold with the order 0..m.  The exclusive result is the
inclusive result of m - 1; member 0's is the op's identity (identity()).
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from support import half_ref as R
from support.rscatter_cases import dtype, esize, inputs, same_bits  # noqa: F401  (shared helpers)

# the (type, op) pairs the GPU tests run
PAIRS = [("int", "sum"), ("short", "min"), ("double", "sum"), ("float", "prod"),
         ("complexf", "prod"), ("half", "sum"), ("long", "xor")]
LDS_U = 1            # vectors per lane per member of team_scan_lds_kernel (team.hip OSGPU_TEAM_LDS_U)
TILE_VECTORS = 64 * LDS_U

_F16 = {"half": {"one": 0x3C00, "pinf": 0x7C00, "ninf": 0xFC00},
        "bfloat16": {"one": 0x3F80, "pinf": 0x7F80, "ninf": 0xFF80}}


def identity(t: str, op: str) -> np.ndarray:
    """One element holding the identity of (t, op): sum all-zero bits, prod 1,
    and all-one bits, or / xor 0, max the type's lowest value, min its highest."""
    if t in R.TYPES:
        v = {"sum": 0, "prod": _F16[t]["one"], "max": _F16[t]["ninf"], "min": _F16[t]["pinf"]}[op]
        return np.array([v], np.uint16)
    dt = np.dtype(O.NP_DTYPE[t])
    if t in O.INT_TYPES:
        info = np.iinfo(dt)
        v = {"sum": 0, "prod": 1, "and": -1, "or": 0, "xor": 0, "max": info.min, "min": info.max}[op]
        return np.array([v], dt)
    v = {"sum": 0.0, "prod": 1.0, "max": -np.inf, "min": np.inf}[op]
    out = np.zeros(1, dt)       # (long double: the padding bytes zero)
    out[0] = v
    return out


def inclusive(t: str, op: str, sources, PE_start=0, logPE_stride=0, PE_size=None):
    """[the inclusive result of member m for m < PE_size]."""
    if PE_size is None:
        PE_size = len(sources)
    members = O.active_set(PE_start, logPE_stride, PE_size)
    if t in R.TYPES:
        return [R.fold(t, op, members[:m + 1], sources) for m in range(PE_size)]
    return [O.to_all(t, op, list(sources), PE_start, logPE_stride, m + 1)[PE_start]
            for m in range(PE_size)]


def expected(t: str, op: str, sources, exclusive, PE_start=0, logPE_stride=0, PE_size=None):
    """{pe: what osgpu_scan leaves in member pe's target}."""
    if PE_size is None:
        PE_size = len(sources)
    members = O.active_set(PE_start, logPE_stride, PE_size)
    inc = inclusive(t, op, sources, PE_start, logPE_stride, PE_size)
    if not exclusive:
        return dict(zip(members, inc))
    n = np.asarray(sources[0]).size
    first = np.repeat(identity(t, op), n)
    return dict(zip(members, [first] + inc[:-1]))


def run(tm, t: str, op: str, exclusive, target_off, source_off: int, nreduce: int,
        PE_start: int = 0, logPE_stride: int = 0, PE_size: int | None = None):
    """Every member of the set calls osgpu_scan on its own thread
    (tests/support/team.py Team); target_off: one offset, or {pe: offset}."""
    if PE_size is None:
        PE_size = tm.npes
    members = O.active_set(PE_start, logPE_stride, PE_size)
    fn = tm.osgpu.scan(t, op, exclusive)
    pwrk = (ctypes.c_byte * 4096)()
    toff = (lambda pe: target_off[pe]) if isinstance(target_off, dict) else (lambda pe: target_off)
    tm._on_members(members, lambda pe: fn(
        tm.ptr(pe, toff(pe)), tm.ptr(pe, source_off), nreduce, PE_start, logPE_stride, PE_size,
        ctypes.addressof(pwrk), tm.psync_ptr(pe)))
    return members
