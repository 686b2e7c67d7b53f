"""The guard-band helper (tests/support/guarded.py) on a numpy stand-in for
the device buffer: the test of the test.  One flipped byte is reported at
its signed distance from the payload at each place that matters -- the first
and the last band byte, the byte just before the payload and the byte just
after it -- and an untouched buffer passes."""
import re

import numpy as np
import pytest

from support import guarded as G

SHAPES = [(0, 0), (1, 0), (16, 0), (10, 6), (4099 * 2, 2), (2049 * 16, 0), (2049 * 16 + 8, 8),
          (33 * 4096 + 3, 15)]


def _flipped(g, i):
    after = g.image.copy()
    after[i] ^= 0x40
    return after


@pytest.mark.parametrize("payload,phase", SHAPES)
@pytest.mark.parametrize("source", [False, True], ids=["output", "source"])
def test_one_flipped_band_byte_is_reported_at_its_offset(payload, phase, source):
    data = G.pattern(5, payload) if source else None
    g = G.Guarded(payload, phase, data)
    assert g.lo == G.GUARD + phase and g.hi == g.lo + payload
    assert g.lo >= G.GUARD and g.size - g.hi >= G.GUARD and g.lo % 16 == phase
    assert g.check(g.image.copy()) is None          # untouched: passes
    g.assert_guards("untouched", g.image.copy())
    g.assert_unchanged("untouched", g.image.copy())
    where = {0: -g.lo,                   # the first band byte
             g.size - 1: g.size - g.hi,  # the last band byte
             g.lo - 1: -1,               # the byte just before the payload
             g.hi: +1}                   # the byte just after it
    for i, want in where.items():
        after = _flipped(g, i)
        assert g.check(after) == want, (i, want)
        with pytest.raises(AssertionError, match=re.escape("byte %+d from the" % want)):
            g.assert_guards("flipped", after)
        with pytest.raises(AssertionError):
            g.assert_unchanged("flipped", after)


def test_payload_bytes_are_not_band_bytes():
    """A store inside the payload is no band fault (assert_guards passes)
    but is a modified source (assert_unchanged fails), at either end."""
    g = G.Guarded(64, 4)
    for i in (g.lo, g.hi - 1):
        after = _flipped(g, i)
        assert g.check(after) is None
        g.assert_guards("payload", after)
        with pytest.raises(AssertionError, match="payload byte %d of 64" % (i - g.lo)):
            g.assert_unchanged("payload", after)


def test_the_band_before_the_payload_is_reported_first():
    g = G.Guarded(32, 0)
    after = _flipped(g, g.hi + 7)
    after[g.lo - 3] ^= 1
    after[g.lo - 9] ^= 1
    assert g.check(after) == -9
    after[g.lo - 9] ^= 1
    after[g.lo - 3] ^= 1
    assert g.check(after) == +8


def test_patterns_vary_with_position_and_differ():
    """No constant byte, zero included, matches the band over a 16-byte
    vector, and the output fill is not the band pattern: a stray vector of
    any one byte, or of fill, is seen wherever it lands."""
    g = G.Guarded(4096, 0)
    band = g.image[:g.lo]
    for k in range(0, band.size - 16, 16):
        assert np.unique(band[k:k + 16]).size == 16
    assert np.array_equal(band, G.pattern(0, g.lo))
    assert np.array_equal(g.data(g.image), G.fill_pattern(4096))
    assert G.first_diff(g.data(g.image)[:16], G.pattern(g.lo, 16)) is not None


def test_arena_lays_buffers_out_without_overlap():
    a = G.Arena()
    bufs = [a.add(p, ph, None if k % 2 else G.pattern(k, p))
            for k, (p, ph) in enumerate(SHAPES)]
    img = a.image()
    assert img.size == a.size == sum(b.size for b in bufs)
    for b in bufs:
        assert b.off % 256 == 0
        assert np.array_equal(img[b.off:b.off + b.size], b.image)
    # a byte flipped in one buffer's band is that buffer's fault only
    img[bufs[3].off + bufs[3].hi] ^= 0xFF
    for k, b in enumerate(bufs):
        assert b.check(img[b.off:b.off + b.size]) == (+1 if k == 3 else None)


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        G.Guarded(16, 16)
    with pytest.raises(ValueError):
        G.Guarded(16, 0, np.zeros(15, np.uint8))
    with pytest.raises(ValueError):
        G.Guarded(16, 0).check(np.zeros(3, np.uint8))
