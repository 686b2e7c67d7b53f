"""uniform_cases.py -- TEST INFRASTRUCTURE of the uniform reduce-to-all tests
(osgpu_reduce_uniform, osgpu_team_uniform): expected values and the PE-thread
driver.

Expected values are never a second fold.  Every member of the set (PE_start,
logPE_stride, PE_size) receives what the reduce-to-all oracle (oracle.to_all)
leaves at PE_start -- the FIRST member, whose caller-first order is the
ascending one -- the identity include/osgpu_reduce.h Part 1g states.  For
half / bfloat16 it is tests/support/half_ref.fold with the members ascending.
Inputs, element sizes and the bit comparison are the scan's and the
reduce-scatter's.
"""
from __future__ import annotations

import ctypes

import oracle as O
from support import half_ref as R
from support.rscatter_cases import dtype, esize, inputs, same_bits  # noqa: F401  (shared helpers)
from support.scan_cases import PAIRS  # noqa: F401  (the (type, op) pairs the GPU tests run)

SUB_VECTORS = 64     # vectors per sub-tile of team_uniform_lds_kernel (team.hip kUniformSub)


def tile_elems(t: str, P: int) -> int:
    """Elements per member per tile of team_uniform_lds_kernel: 64 * P vectors."""
    return SUB_VECTORS * P * (16 // esize(t))


def value(t: str, op: str, sources, PE_start=0, logPE_stride=0, PE_size=None):
    """The one array every member receives."""
    if PE_size is None:
        PE_size = len(sources)
    if t in R.TYPES:
        return R.fold(t, op, O.active_set(PE_start, logPE_stride, PE_size), sources)
    return O.to_all(t, op, list(sources), PE_start, logPE_stride, PE_size)[PE_start]


def expected(t: str, op: str, sources, PE_start=0, logPE_stride=0, PE_size=None):
    """{pe: what osgpu_reduce_uniform leaves in member pe's target}."""
    if PE_size is None:
        PE_size = len(sources)
    v = value(t, op, sources, PE_start, logPE_stride, PE_size)
    return {pe: v for pe in O.active_set(PE_start, logPE_stride, PE_size)}


def caller_first(t: str, op: str, sources, pe, PE_start=0, logPE_stride=0, PE_size=None):
    """What the reduce-to-all leaves at member `pe`: its own source first."""
    if PE_size is None:
        PE_size = len(sources)
    if t in R.TYPES:
        return R.fold(t, op, O.fold_order(pe, PE_start, logPE_stride, PE_size), sources)
    return O.to_all(t, op, list(sources), PE_start, logPE_stride, PE_size)[pe]


def run(tm, t: str, op: str, target_off, source_off: int, nreduce: int, PE_start: int = 0,
        logPE_stride: int = 0, PE_size: int | None = None):
    """Every member of the set calls osgpu_reduce_uniform on its own thread
    (tests/support/team.py Team); target_off: one offset, or {pe: offset}."""
    if PE_size is None:
        PE_size = tm.npes
    members = O.active_set(PE_start, logPE_stride, PE_size)
    fn = tm.osgpu.reduce_uniform(t, op)
    pwrk = (ctypes.c_byte * 4096)()
    toff = (lambda pe: target_off[pe]) if isinstance(target_off, dict) else (lambda pe: target_off)
    tm._on_members(members, lambda pe: fn(
        tm.ptr(pe, toff(pe)), tm.ptr(pe, source_off), nreduce, PE_start, logPE_stride, PE_size,
        ctypes.addressof(pwrk), tm.psync_ptr(pe)))
    return members
