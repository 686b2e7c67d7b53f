"""many_cases.py -- TEST INFRASTRUCTURE of the batched reduce-to-all tests
(osgpu_reduce_many, osgpu_combine_many): the counting PE-ops table, the heap
layout of a table of arrays, and the PE-thread drivers of the batched call
and of the loop of single calls it must equal.

Expected values are the reduce-to-all oracle's, entry by entry
(tests/support/rscatter_cases.py to_all / fold_left): the identity
include/osgpu_reduce.h Part 1e states.  There is no second oracle.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

import oracle as O
from support import rscatter_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
BC_PATH = os.path.join(HERE, "libbar_count.so")
MANY_U = 2           # vectors per lane per input of combine_many_kernel (combine.hip OSGPU_MANY_U)
TILE_VECTORS = 64 * MANY_U
MANY_SEGS = 16       # csrc/many_host.hpp kManySegs

_BC = None


def build_bar_count():
    src = os.path.join(HERE, "bar_count.c")
    if not os.path.exists(BC_PATH) or os.path.getmtime(BC_PATH) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", BC_PATH, src], check=True)


def bar_count():
    """tests/support/bar_count.c: bc_wrap(inner ops) -> counting ops, bc_calls(pe)."""
    global _BC
    if _BC is None:
        build_bar_count()
        B = ctypes.CDLL(BC_PATH)
        B.bc_wrap.restype = ctypes.c_void_p
        B.bc_wrap.argtypes = [ctypes.c_void_p]
        B.bc_calls.restype = ctypes.c_long
        _BC = B
    return _BC


class counted_barriers:
    """with counted_barriers(tm) as calls: the library's barriers go through
    the counting table over the team's PE services; calls(pe) is PE pe's
    count.  The team's own table is put back afterwards."""

    def __init__(self, tm):
        self.tm = tm

    def __enter__(self):
        B = bar_count()
        assert self.tm.lib.osgpu_set_pe_ops(B.bc_wrap(self.tm.pet.pet_ops())) == 0
        return B.bc_calls

    def __exit__(self, *exc):
        assert self.tm.lib.osgpu_set_pe_ops(self.tm.pet.pet_ops()) == 0
        return False


def _align(x, a=256):
    return (x + a - 1) // a * a


class Layout:
    """A table of arrays in one symmetric heap: entry i's source of lens[i]
    elements, then every target, each in its own 256-byte aligned area with
    256 bytes of filler behind it.  inplace: entries whose target IS their
    source; odd / sodd: {entry: elements} a target / source shifted off its
    area's start."""

    def __init__(self, t, lens, inplace=(), odd=None, sodd=None):
        self.t, self.s, self.lens = t, C.esize(t), list(lens)
        odd, sodd = odd or {}, sodd or {}
        off = 256
        self.soff, self.toff = [], []
        for i, n in enumerate(self.lens):
            self.soff.append(off + sodd.get(i, 0) * self.s)
            off += _align(n * self.s + sodd.get(i, 0) * self.s) + 256
        for i, n in enumerate(self.lens):
            if i in inplace:
                self.toff.append(self.soff[i])
                continue
            self.toff.append(off + odd.get(i, 0) * self.s)
            off += _align(n * self.s + odd.get(i, 0) * self.s) + 256
        self.bytes = off + 4096

    def target_mask(self):
        m = np.zeros(self.bytes, dtype=bool)
        for o, n in zip(self.toff, self.lens):
            m[o:o + n * self.s] = True
        return m


def run_many(tm, t, op, lay, PE_start=0, logPE_stride=0, PE_size=None):
    """Every member of the set calls osgpu_reduce_many once, on its own thread."""
    PE_size = tm.npes if PE_size is None else PE_size
    members = O.active_set(PE_start, logPE_stride, PE_size)
    fn = tm.osgpu.reduce_many(t, op)
    pwrk = (ctypes.c_byte * 4096)()
    tm._on_members(members, lambda pe: fn(
        [tm.ptr(pe, o) for o in lay.toff], [tm.ptr(pe, o) for o in lay.soff], lay.lens,
        PE_start, logPE_stride, PE_size, ctypes.addressof(pwrk), tm.psync_ptr(pe)))
    return members


def run_singles(tm, t, op, lay, PE_start=0, logPE_stride=0, PE_size=None):
    """The same table as len(lens) single reduce-to-all calls per member
    (shmem_<t>_<op>_to_all; osgpu_reduce_ext for half / bfloat16)."""
    PE_size = tm.npes if PE_size is None else PE_size
    members = O.active_set(PE_start, logPE_stride, PE_size)
    pwrk = (ctypes.c_byte * 4096)()
    if t in tm.osgpu.EXT_TYPES:
        tc, oc = tm.osgpu.type_code(t), tm.osgpu.OPS.index(op)
        one = lambda *a: tm.lib.osgpu_reduce_ext(tc, oc, *a)
    else:
        one = tm.osgpu.to_all(t, op)

    def body(pe):
        for to, so, n in zip(lay.toff, lay.soff, lay.lens):
            one(tm.ptr(pe, to), tm.ptr(pe, so), n, PE_start, logPE_stride, PE_size,
                ctypes.addressof(pwrk), tm.psync_ptr(pe))
    tm._on_members(members, body)
    return members


def sources(t, op, npes, lens, seed):
    """src[i][pe]: member pe's array of entry i."""
    return [C.inputs(t, op, npes, max(n, 0), seed + 7 * i) for i, n in enumerate(lens)]


def expected(t, op, src, PE_start=0, logPE_stride=0, PE_size=None):
    """want[i][pe]: the oracle's reduce-to-all of entry i (None for an empty entry)."""
    return [C.to_all(t, op, s, PE_start, logPE_stride, PE_size) if len(s[0]) else None
            for s in src]
