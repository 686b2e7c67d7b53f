"""alltoalls_ref.py -- TEST INFRASTRUCTURE: numpy restatement of the strided
all-to-all (shmem_alltoalls32/64) from the OpenSHMEM 1.4 definition, in the
style of oracle_coll.alltoall.  It never calls the library.

Every PE is a dict entry {pe: np.ndarray(uint8)} holding that PE's symmetric
object.  In elements of esz bytes, with me_idx the caller's index in the
active set and pe_j its j-th member, for j < PE_size and k < nelems:

    target_me[(j*nelems + k) * dst] = source_{pe_j}[(me_idx*nelems + k) * sst]

Every other byte of the target -- the gaps between the strided elements and
everything past the span -- keeps the value it had.

Where the reference's literal text (src/alltoall.c:26-55) differs, this is
the specification: the source block is indexed by the active-set index (the
reference uses proc.rank, :46), offsets are not truncated to int (:45-46),
and strides count elements (the sized iget the reference calls advances by
bytes, src/putget.h:204-205).
"""
from __future__ import annotations

import numpy as np


def active_set(PE_start: int, logPE_stride: int, PE_size: int):
    step = 1 << logPE_stride
    return [PE_start + i * step for i in range(PE_size)]


def extent_bytes(PE_size: int, nelems: int, stride: int, esz: int) -> int:
    """Bytes spanned by PE_size * nelems elements `stride` apart."""
    if PE_size * nelems == 0:
        return 0
    return ((PE_size * nelems - 1) * stride + 1) * esz


def alltoalls(sources: dict, targets: dict, esz: int, dst: int, sst: int, nelems: int,
              PE_start: int, logPE_stride: int, PE_size: int) -> dict:
    """Every member's target after the call, starting from targets[pe]."""
    assert esz in (4, 8) and dst >= 1 and sst >= 1
    pes = active_set(PE_start, logPE_stride, PE_size)
    out = {pe: targets[pe].copy() for pe in pes}
    for me_idx, me in enumerate(pes):
        for j, pe in enumerate(pes):
            for k in range(nelems):
                t = (j * nelems + k) * dst * esz
                s = (me_idx * nelems + k) * sst * esz
                out[me][t:t + esz] = sources[pe][s:s + esz]
    return out


def alltoalls_fast(sources: dict, targets: dict, esz: int, dst: int, sst: int, nelems: int,
                   PE_start: int, logPE_stride: int, PE_size: int) -> dict:
    """The same by numpy slicing (for the sizes the GPU tests use);
    tests/test_alltoalls_ref.py holds it to the loop above."""
    pes = active_set(PE_start, logPE_stride, PE_size)
    out = {pe: targets[pe].copy() for pe in pes}
    if nelems == 0:
        return out
    dt = np.uint32 if esz == 4 else np.uint64
    for me_idx, me in enumerate(pes):
        tn = (PE_size * nelems - 1) * dst + 1
        t = out[me][:tn * esz].view(dt)
        for j, pe in enumerate(pes):
            s0 = me_idx * nelems * sst
            sn = (nelems - 1) * sst + 1
            s = sources[pe][s0 * esz:(s0 + sn) * esz].view(dt)
            t[j * nelems * dst:j * nelems * dst + (nelems - 1) * dst + 1:dst] = s[::sst]
    return out
