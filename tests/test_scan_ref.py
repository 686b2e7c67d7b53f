"""The prefix scan's expected-value model without a GPU
(tests/support/scan_cases.py): it is the reduce-to-all oracle over sub-sets,
never a second fold.

* the last member's inclusive result equals member 0's reduce-to-all for
  every golden (type, op) pair (and half / bfloat16);
* it differs from member 1's reduce-to-all on a seeded FP sum input: the
  order matters and the test can see it;
* a strided active set: members, not PE numbers, count;
* the exclusive result is the inclusive one shifted by a member, the identity
  first;
* the identity table against numpy (np.iinfo, +-inf, the half / bfloat16
  patterns): x op identity == x for values that are no NaN.
"""
import numpy as np

import oracle as O
from support import half_ref as R
from support import scan_cases as C

ALL = O.ALL_PAIRS + [(t, o) for t in R.TYPES for o in R.OPS]


def test_last_member_inclusive_is_member_0_reduce_to_all():
    P, n = 4, 67
    for t, op in ALL:
        src = C.inputs(t, op, P, n, 0x5CA + len(t))
        inc = C.inclusive(t, op, src)
        if t in R.TYPES:
            full0 = R.fold(t, op, list(range(P)), src)
        else:
            full0 = O.to_all(t, op, src)[0]
        assert C.same_bits(t, inc[P - 1], full0) is None, (t, op)
        assert C.same_bits(t, inc[0], np.asarray(src[0])) is None, (t, op)   # one member: a copy


def test_order_matters_and_the_model_sees_it():
    """FP sums depend on the order: the scan's ascending fold is member 0's,
    not the caller-first one of another member.  Member 2's (x2 + x0) + x1
    rounds differently on plain values; member 1's (x1 + x0) + x2 differs
    from (x0 + x1) + x2 only where x0 and x1 are both NaN -- the first
    operand's payload wins -- which the edge inputs hold."""
    P, n = 3, 4096
    for t in ("float", "double"):
        src = O.team_inputs(t, P, n, 0x0DE4, "wide")
        full = O.to_all(t, "sum", src)
        last = C.inclusive(t, "sum", src)[P - 1]
        assert C.same_bits(t, last, full[0]) is None
        assert C.same_bits(t, last, full[2]) is not None, t
        src = O.team_inputs(t, P, n, 0x0DE4, "edge")
        full = O.to_all(t, "sum", src)
        last = C.inclusive(t, "sum", src)[P - 1]
        assert C.same_bits(t, last, full[0]) is None
        assert C.same_bits(t, last, full[1]) is not None, t
    src = [R.order_values("half", n, 7 + pe) for pe in range(P)]
    last = C.inclusive("half", "sum", src)[P - 1]
    assert np.array_equal(last, R.fold("half", "sum", [0, 1, 2], src))
    assert not np.array_equal(last, R.fold("half", "sum", [2, 0, 1], src))


def test_strided_active_set():
    n = 33
    for t, op in (("double", "sum"), ("bfloat16", "prod"), ("short", "min")):
        src = C.inputs(t, op, 8, n, 99)
        for ex in (0, 1):
            want = C.expected(t, op, src, ex, 1, 1, 3)
            assert sorted(want) == [1, 3, 5]
        inc = C.expected(t, op, src, 0, 1, 1, 3)
        exc = C.expected(t, op, src, 1, 1, 1, 3)
        # the same members packed into a contiguous set of 3 give the same folds
        packed = C.inclusive(t, op, [src[1], src[3], src[5]])
        for m, pe in enumerate((1, 3, 5)):
            assert C.same_bits(t, inc[pe], packed[m]) is None
        assert C.same_bits(t, exc[3], inc[1]) is None and C.same_bits(t, exc[5], inc[3]) is None
        assert C.same_bits(t, exc[1], np.repeat(C.identity(t, op), n)) is None


def test_written_out_case():
    src = [np.array([1, 2], np.int32), np.array([10, 20], np.int32), np.array([100, 200], np.int32)]
    inc = C.expected("int", "sum", src, 0)
    exc = C.expected("int", "sum", src, 1)
    assert [inc[p].tolist() for p in range(3)] == [[1, 2], [11, 22], [111, 222]]
    assert [exc[p].tolist() for p in range(3)] == [[0, 0], [1, 2], [11, 22]]
    exc = C.expected("int", "min", src, 1)
    assert exc[0].tolist() == [2**31 - 1] * 2 and exc[2].tolist() == [1, 2]


def test_identity_table_against_numpy():
    for t in O.INT_TYPES:
        info = np.iinfo(O.NP_DTYPE[t])
        assert C.identity(t, "max")[0] == info.min and C.identity(t, "min")[0] == info.max
        assert C.identity(t, "and").view(np.uint8).tolist() == [0xFF] * C.esize(t)
        assert C.identity(t, "prod")[0] == 1
        for op in ("sum", "or", "xor"):
            assert not C.identity(t, op).view(np.uint8).any()
    for t in O.REAL_FP:
        assert C.identity(t, "max")[0] == -np.inf and C.identity(t, "min")[0] == np.inf
        assert C.identity(t, "prod")[0] == 1 and not C.identity(t, "sum").view(np.uint8).any()
    for t in O.CPLX:
        assert C.identity(t, "prod")[0] == 1 + 0j and not C.identity(t, "sum").view(np.uint8).any()
    assert [int(C.identity("half", o)[0]) for o in R.OPS] == [0, 0x3C00, 0xFC00, 0x7C00]
    assert [int(C.identity("bfloat16", o)[0]) for o in R.OPS] == [0, 0x3F80, 0xFF80, 0x7F80]
    for t in R.TYPES:
        assert R.widen(t, C.identity(t, "prod"))[0] == 1.0
        assert R.widen(t, C.identity(t, "max"))[0] == -np.inf
        assert R.widen(t, C.identity(t, "min"))[0] == np.inf
    # x op identity == x by the oracle's own element ops, for every pair
    n = 257
    for t, op in ALL:
        if t == "longdouble" or t in O.CPLX:  # (long double's edge inputs hold non-canonical
            continue     # x87 encodings; both kinds of identity are checked by value above)
        x = np.asarray(C.inputs(t, op, 1, n, 0x1D)[0])
        if t in R.TYPES:
            keep = ~R.isnan(t, x)
            if op == "sum":
                keep &= x != 0x8000     # +0 + -0 = +0: the identity is never an operand
            got = R.op2(t, op, np.repeat(C.identity(t, op), n), x)
            assert np.array_equal(got[keep], x[keep]), (t, op)
            continue
        got = O.op_elementwise(t, op, np.repeat(C.identity(t, op), n), x)
        keep = np.ones(n, bool) if t in O.INT_TYPES else ~np.isnan(x)
        if op == "sum" and t not in O.INT_TYPES:
            keep &= ~((x == 0) & np.signbit(x))     # +0 + -0 = +0: not an operand, as stated
        assert C.same_bits(t, got[keep], x[keep]) is None, (t, op)
