"""The float-accumulated half / bfloat16 sum's numpy definition
(tests/support/wsum_ref.py, include/osgpu_reduce.h Part 1i) against independent
routes, without a GPU:

* NaN-free seeded data: numpy.float16 <-> float32 conversions for half,
  torch.bfloat16 conversions for bfloat16, a plain float32 running sum;
* NaNs: the closed form -- the first NaN in member order quieted, or the
  default NaN for inf - inf, bfloat16's max + max + (-inf) included;
* the inputs of the GPU tests tell this sum from the per-step one for every
  (type, P >= 3) they use; a chunked fold with a float carry equals the
  unchunked one, a 16-bit carry does not.
"""
import numpy as np
import pytest

from support import half_ref as R
from support import wsum_ref as W

GPU_P = (3, 5, 8, 9, 17)   # the member counts >= 3 tests/test_gpu_wsum.py uses


def _finite(t, n, seed):
    """Seeded patterns without NaNs and infinities."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    bad = (x & 0x7FFF) >= R.EXPMASK[t]
    return np.where(bad, x & 0x83FF if t == "half" else x & 0x807F, x).astype(np.uint16)


def _independent(t, srcs):
    """(float32 accumulator, narrowed patterns) by numpy / torch conversions."""
    if t == "half":
        f = [s.view(np.float16).astype(np.float32) for s in srcs]
    else:
        import torch
        f = [torch.from_numpy(s.view(np.int16).copy()).view(torch.bfloat16).to(torch.float32).numpy()
             for s in srcs]
    acc = f[0].copy()
    with np.errstate(all="ignore"):
        for x in f[1:]:
            acc = (acc + x).astype(np.float32)
    if t == "half":
        with np.errstate(all="ignore"):
            out = acc.astype(np.float16).view(np.uint16)
    else:
        import torch
        out = torch.from_numpy(acc).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return acc, out


@pytest.mark.parametrize("t", W.TYPES)
@pytest.mark.parametrize("P", [1, 2, 3, 8, 17])
def test_nan_free_data_matches_independent_conversions(t, P):
    srcs = [_finite(t, 4096, 0x5EED + 31 * P + j) for j in range(P)]
    # small magnitudes too, so that sums stay finite and hit subnormal results
    srcs += []
    acc, out = _independent(t, srcs)
    keep = ~np.isnan(acc)   # inf - inf of an overflowed accumulator: the closed form's test
    assert keep.sum() > 3000
    assert np.array_equal(W.wsum(t, "float", srcs)[keep], acc.view(np.uint32)[keep])
    assert np.array_equal(W.wsum(t, t, srcs)[keep], out[keep])


@pytest.mark.parametrize("t", W.TYPES)
def test_every_pattern_widens_and_narrows_back(t):
    x = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(W.narrow(t, W.widen(t, x)), x)       # NaNs included: lossless
    assert np.array_equal(W.wsum(t, t, [x]), x)                # one member: a copy


@pytest.mark.parametrize("t", W.TYPES)
@pytest.mark.parametrize("P", [2, 3, 8])
def test_nan_closed_form(t, P):
    srcs = W.nan_table(t, P)
    got = W.wsum(t, t, srcs)
    gotf = W.wsum(t, "float", srcs)
    nan = np.stack([R.isnan(t, s) for s in srcs])
    first = np.where(nan, np.arange(P)[:, None], P).min(axis=0)
    has = first < P
    stack = np.stack(srcs)
    k = np.arange(stack.shape[1])
    want = stack[first.clip(0, P - 1), k] | R.QUIET[t]
    assert has.sum() >= 3 * P
    assert np.array_equal(got[has], want[has])
    assert np.array_equal(gotf[has], W.widen(t, want[has]))
    # without an input NaN a NaN result is the default one: inf - inf
    made = ~has & R.isnan(t, got)
    assert made.sum() >= P * (P - 1)
    assert (got[made] == R.DEFNAN[t]).all() and (gotf[made] == 0xFFC00000).all()
    # ... and nothing else is a NaN
    assert not W.isnan32(gotf[~has & ~made]).any()


def test_bfloat16_overflow_then_minus_inf():
    mx, ninf = 0x7F7F, 0xFF80
    srcs = [np.array([mx], np.uint16), np.array([mx], np.uint16), np.array([ninf], np.uint16)]
    assert W.accumulate("bfloat16", srcs[:2])[0] == 0x7F800000     # the float overflowed
    assert W.wsum("bfloat16", "bfloat16", srcs)[0] == 0xFFC0
    assert W.wsum("bfloat16", "float", srcs)[0] == 0xFFC00000
    # half cannot overflow a float accumulator: max + max + -inf is -inf
    h = [np.array([0x7BFF], np.uint16), np.array([0x7BFF], np.uint16), np.array([0xFC00], np.uint16)]
    assert W.wsum("half", "half", h)[0] == 0xFC00
    # the per-step sum overflows to +inf there: it gives the default NaN
    assert W.per_step("half", h)[0] == 0xFE00


def test_the_named_elements():
    for t, big, want, stepwise in (("half", 0x6800, 2052.0, 2048.0), ("bfloat16", 0x4380, 260.0, 256.0)):
        one = 0x3C00 if t == "half" else 0x3F80
        srcs = [np.array([v], np.uint16) for v in (big, one, one, one)]
        assert R.widen(t, W.wsum(t, t, srcs))[0] == want
        assert R.widen(t, W.per_step(t, srcs))[0] == stepwise
        assert W.wsum(t, "float", srcs).view(np.float32)[0] == R.widen(t, [big])[0] + 3.0


@pytest.mark.parametrize("t", W.TYPES)
@pytest.mark.parametrize("P", GPU_P)
def test_inputs_tell_the_sums_apart(t, P):
    for n in (W.GROUP + 1, W.TILE + 1):
        srcs = W.inputs(t, P, n, 0xA0 + P)
        W.assert_discriminating(t, srcs)
        assert not R.isnan(t, W.wsum(t, t, srcs)[np.arange(n) % 5 == 2]).any()


@pytest.mark.parametrize("t", W.TYPES)
@pytest.mark.parametrize("P", [9, 17])
def test_float_carry_is_exact_and_a_16_bit_carry_is_not(t, P):
    srcs = W.inputs(t, P, 4001, 0xCA + P)
    for out_t in (t, "float"):
        whole = W.wsum(t, out_t, srcs)
        assert np.array_equal(W.chunked(t, out_t, srcs, 8, float_carry=True), whole)
        assert (W.chunked(t, out_t, srcs, 8, float_carry=False) != whole).any()
    # a carry passed in by hand: the raw launcher's form
    mid = W.accumulate(t, srcs[:8])
    assert np.array_equal(W.wsum(t, t, srcs[8:], carry=mid), W.wsum(t, t, srcs))
