"""wsum_cases.py -- TEST INFRASTRUCTURE of the float-accumulated sum's GPU tests
(osgpu_reduce_wsum, osgpu_team_wsum): the shared input pool, the heap layout of
a call whose target may be wider than its source (gpu_doors.heap_layout assumes
targets of the source's type), and the PE-thread driver.  Expected values:
tests/support/wsum_ref.py.
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from support import half_ref as R
from support import wsum_ref as W

NMAX = 3 * W.TILE + W.GROUP + 1   # the longest array any test uses
NPOOL = 17                        # members of the pool (8 + 8 + 1: the three-chunk chain)


def out_size(out_t: str) -> int:
    return 4 if out_t == "float" else 2


def out_dtype(out_t: str):
    return np.uint32 if out_t == "float" else np.uint16


def mixed_inputs(t: str, P: int, n: int, seed: int):
    """wsum_ref.inputs (order-sensitive values, the elements that tell this sum
    from the per-step one) with every 7th element from half_ref.special_table
    (NaNs with payloads, infinities, extremes), rotated by the member."""
    out = W.inputs(t, P, n, seed)
    k = np.arange(n) % 7 == 3
    for j in range(P):
        out[j][k] = np.resize(np.roll(R.special_table(t, 512, seed + j), 5 * j), n)[k]
    return out


_POOL = {}


def pool(t: str):
    """(sources of NPOOL members at NMAX elements, a float carry: the
    accumulator of members 8..15), computed once and never changed."""
    if t not in _POOL:
        srcs = mixed_inputs(t, NPOOL, NMAX, 0x57 + len(t))
        for P in (3, 5, 8, 9, 17):
            W.assert_discriminating(t, srcs[:P])
        carry = W.accumulate(t, srcs[8:16])
        for a in srcs + [carry]:
            a.setflags(write=False)
        _POOL[t] = (srcs, carry, {})
    return _POOL[t]


def want(t: str, out_t: str, P: int, n: int, carry: bool):
    srcs, cv, memo = pool(t)
    key = (out_t, P, carry)
    if key not in memo:
        memo[key] = W.wsum(t, out_t, srcs[:P], carry=cv if carry else None)
    return memo[key][:n]


def layout(n: int, out_t: str, shift: int = 0):
    """(source offset, target offset, heap bytes): the target in its own 4 KiB
    aligned area behind the source, `shift` target elements on."""
    area = (n * 4 + 4095) // 4096 * 4096 + 4096
    return 0, area + shift * out_size(out_t), 2 * area + 4096


def run(tm, t: str, out_t: str, target_ptr, source_off: int, nreduce: int, PE_start: int = 0,
        logPE_stride: int = 0, PE_size: int | None = None):
    """Every member of the set calls osgpu_reduce_wsum on its own thread
    (tests/support/team.py Team); target_ptr(pe): its target's address."""
    if PE_size is None:
        PE_size = tm.npes
    members = O.active_set(PE_start, logPE_stride, PE_size)
    fn = tm.osgpu.reduce_wsum(t, out_t)
    pwrk = (ctypes.c_byte * 4096)()
    tm._on_members(members, lambda pe: fn(
        target_ptr(pe), tm.ptr(pe, source_off), nreduce, PE_start, logPE_stride, PE_size,
        ctypes.addressof(pwrk), tm.psync_ptr(pe)))
    return members
