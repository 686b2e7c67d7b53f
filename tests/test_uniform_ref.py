"""The uniform reduce-to-all's expected-value model without a GPU
(tests/support/uniform_cases.py): the first member's reduce-to-all by the
oracle, never a second fold.

* it equals the last member's inclusive scan (tests/support/scan_cases.py)
  for every (type, op) pair of the library, and on a strided active set;
* the discrimination condition: on the inputs the GPU tests use (n = 1001,
  seed 0xD0 + P, P in {3, 8}) the LAST member's caller-first reduce-to-all
  differs from the uniform value in at least one element for double sum,
  float prod, complexf prod, half sum and float max -- an implementation that
  reuses the caller-first kernels cannot pass the GPU tests.  Counts measured
  when this was written, of 1001 elements, P = 3 / P = 8: double sum 154 /
  266, float prod 274 / 408, complexf prod 678 / 684, half sum 69 / 137,
  float max 67 / 102.
"""
import numpy as np
import pytest

import oracle as O
from support import half_ref as R
from support import scan_cases as S
from support import uniform_cases as C

ALL = O.ALL_PAIRS + [(t, o) for t in R.TYPES for o in R.OPS]
DISCRIMINATING = [("double", "sum"), ("float", "prod"), ("complexf", "prod"), ("half", "sum"),
                  ("float", "max")]


def test_value_is_the_last_members_inclusive_scan():
    assert len(ALL) == 52
    P, n = 4, 67
    for t, op in ALL:
        src = C.inputs(t, op, P, n, 0x5CA + len(t))
        v = C.value(t, op, src)
        assert C.same_bits(t, v, S.inclusive(t, op, src)[P - 1]) is None, (t, op)
        want = C.expected(t, op, src)
        assert sorted(want) == list(range(P))
        assert all(C.same_bits(t, w, v) is None for w in want.values()), (t, op)


def test_strided_active_set():
    n = 33
    for t, op in (("double", "sum"), ("bfloat16", "prod"), ("short", "min"), ("longdouble", "sum")):
        src = C.inputs(t, op, 8, n, 99)
        want = C.expected(t, op, src, 1, 1, 3)
        assert sorted(want) == [1, 3, 5]
        # the same members packed into a contiguous set of 3 give the same fold
        packed = C.value(t, op, [src[1], src[3], src[5]])
        last = S.inclusive(t, op, src, 1, 1, 3)[2]
        for pe in (1, 3, 5):
            assert C.same_bits(t, want[pe], packed) is None
            assert C.same_bits(t, want[pe], last) is None


def test_written_out_case():
    src = [np.array([1, 2], np.int32), np.array([10, 20], np.int32), np.array([100, 200], np.int32)]
    want = C.expected("int", "sum", src)
    assert [want[p].tolist() for p in range(3)] == [[111, 222]] * 3
    # float: (1 + 1) + 2^24 is exact; the last member's (2^24 + 1) + 1 rounds twice to 2^24
    src = [np.array([1.0], np.float32), np.array([1.0], np.float32), np.array([2.0 ** 24], np.float32)]
    assert C.value("float", "sum", src)[0] == 2.0 ** 24 + 2
    assert C.caller_first("float", "sum", src, 2)[0] == 2.0 ** 24


@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("t,op", DISCRIMINATING, ids=lambda x: x)
def test_discrimination_condition(t, op, P):
    n = 1001
    src = C.inputs(t, op, P, n, 0xD0 + P)
    v = C.value(t, op, src)
    last = C.caller_first(t, op, src, P - 1)
    g = np.ascontiguousarray(last).view(np.uint8).reshape(n, -1)
    w = np.ascontiguousarray(v).view(np.uint8).reshape(n, -1)
    differ = int((g != w).any(axis=1).sum())
    print(f"{t} {op} P={P}: {differ} of {n} elements differ")
    assert differ >= 1
    # and member 0's caller-first result IS the uniform value
    assert C.same_bits(t, C.caller_first(t, op, src, 0), v) is None
