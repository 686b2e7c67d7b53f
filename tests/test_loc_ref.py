"""The max / min with location's expected-value model without a GPU
(tests/support/loc_cases.py): the value is the uniform reduce's (the oracle's,
never a second fold), the index the closed form of include/osgpu_reduce.h
Part 1h.

* the closed form equals a literal fold of the definition, in value bits and
  in index, on the tie inputs (ties, NaNs, signed zeros, INT_MIN / INT_MAX
  indices) and on `wide` seeded inputs, for all 16 pairs and P in {1, 2, 3, 8};
* the tie inputs discriminate (loc_cases.assert_discriminating, inside
  tie_case): a "first holder wins" or "last holder wins" index fails them;
* for integer types it equals numpy's argmax / argmin with the lowest-index
  tie-break (indices = member numbers);
* a few cases written out by hand.
"""
import numpy as np
import pytest

from support import loc_cases as C

N = 1531


@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("t,op", C.PAIRS, ids=lambda x: x)
def test_closed_form_is_the_literal_fold(t, op, P):
    for kind in ("tie", "wide"):
        if kind == "tie":
            vals, locs = C.tie_case(t, op, P, N, 0x71E + P)
        else:
            vals = C.inputs(t, op, P, N, 0x51DE + P)
            locs = C.tie_indices(P, N, 0x51DE + P)
        v, i = C.expected(t, op, vals, locs)
        lv, li = C.literal_fold(t, op, vals, locs)
        assert C.same_bits(t, v, lv) is None, (kind, "the oracle's value is not the fold's")
        assert np.array_equal(i, li), (kind, int(np.flatnonzero(i != li)[0]))
        assert i.dtype == np.int32


def test_pairs_and_group():
    assert len(C.PAIRS) == 16
    assert [C.group(t) for t in ("short", "half", "int", "float", "long", "double")] == [8, 8, 4, 4, 4, 4]
    assert C.tile_elems("bfloat16") == 2048 and C.tile_elems("double") == 1024


@pytest.mark.parametrize("t", ["short", "int", "long", "longlong"])
def test_integers_match_numpy_argmax(t):
    P, n = 8, 997
    vals = C.tie_values(t, P, n, 0xA56)
    pes = C.member_pes(0, 0, P)
    m = np.stack(vals)
    for op, arg in (("max", np.argmax), ("min", np.argmin)):
        v, i = C.expected(t, op, vals, C.const_indices(pes, n))
        assert np.array_equal(i, arg(m, axis=0))          # numpy: the first occurrence
        assert np.array_equal(v, m.max(axis=0) if op == "max" else m.min(axis=0))


def test_strided_member_numbers():
    assert C.member_pes(1, 1, 3) == [1, 3, 5]
    vals = [np.array([5, 1], np.int32), np.array([5, 9], np.int32), np.array([5, 9], np.int32)]
    v, i = C.expected("int", "max", vals, C.const_indices([1, 3, 5], 2))
    assert v.tolist() == [5, 9] and i.tolist() == [1, 3]


def test_written_out_cases():
    nan, f = np.nan, np.float32
    # a NaN in the middle hides what came before it; one at the end wins with its index
    vals = [np.array([9, 1, 1, 0.0], f), np.array([nan, nan, 1, -0.0], f), np.array([2, 1, nan, 0.0], f)]
    locs = [np.array([7, 7, 7, 7], np.int32), np.array([5, 5, 5, 3], np.int32),
            np.array([6, 6, 6, 9], np.int32)]
    v, i = C.expected("float", "max", vals, locs)
    assert v[0] == 2 and i[0] == 6
    assert v[1] == 1 and i[1] == 6
    assert np.isnan(v[2]) and i[2] == 6
    assert v[3] == 0 and i[3] == 3           # +0 == -0: the lowest index of the three
    lv, li = C.literal_fold("float", "max", vals, locs)
    assert np.array_equal(li, i) and C.same_bits("float", lv, v) is None
    # descending indices: min() chooses the LAST holder's
    vals = [np.array([4], np.int16)] * 3
    v, i = C.expected("short", "min", vals, [np.array([x], np.int32) for x in (30, 20, 10)])
    assert i.tolist() == [10]
    v, i = C.expected("short", "min", vals, [np.array([x], np.int32) for x in (C.INT_MAX, C.INT_MIN, 0)])
    assert i.tolist() == [C.INT_MIN]
