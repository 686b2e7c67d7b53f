"""guarded.py -- TEST INFRASTRUCTURE: device buffers with a guard band on
each side, so a store outside [target, target + nbytes) lands in the test's
own allocation and is seen.

A Guarded buffer is GUARD bytes of band, `phase` more band bytes (the payload
starts at that 16-byte phase), the payload, and at least GUARD bytes of band
again.  The bands hold a pattern that varies with position -- a constant
sentinel cannot see a stray store of the same byte, a zero fill cannot see a
stray zero -- and the payload of an output holds a second pattern, so an
element left unwritten shows too.  GUARD is 16 KiB: the largest tile any
kernel stores is 1024 vectors of 16 bytes (combine_vec_kernel,
team_vec_kernel, copy_vec_kernel: 256 lanes x U = 4), so a whole stray tile
stays inside the band.

An Arena lays many Guarded buffers out in ONE device allocation: one upload,
the launches, one synchronize and one download serve every buffer of a case
(or of a batch of cases).  Everything but Arena.upload / Arena.download is
plain numpy and is tested without a GPU (tests/test_guarded.py).
"""
from __future__ import annotations

import numpy as np

GUARD = 16 << 10
_ALIGN = 256  # arena offsets: every buffer starts at phase 0 of the pattern's period


def pattern(start: int, n: int) -> np.ndarray:
    """The band pattern at positions [start, start + n): (37 i + 11) mod 256."""
    i = np.arange(start, start + n, dtype=np.int64)
    return ((37 * i + 11) & 0xFF).astype(np.uint8)


def fill_pattern(n: int) -> np.ndarray:
    """What an output's payload holds before the call: (101 i + 173) mod 256."""
    i = np.arange(n, dtype=np.int64)
    return ((101 * i + 173) & 0xFF).astype(np.uint8)


_PAT = pattern(0, _ALIGN)
_FILL = fill_pattern(_ALIGN)


def _tiled(period: np.ndarray, n: int) -> np.ndarray:
    return np.tile(period, -(-n // period.size))[:n] if n else np.zeros(0, np.uint8)


def first_diff(a: np.ndarray, b: np.ndarray):
    """Index of the first differing byte of two equally long arrays, or None."""
    if a.shape != b.shape:
        raise ValueError("first_diff: shapes differ")
    if np.array_equal(a, b):
        return None
    return int(np.flatnonzero(a != b)[0])


class Guarded:
    """`payload` bytes at 16-byte phase `phase`; data: what the payload holds
    (a source's elements), None: the fill pattern (an output).

    image   the bytes to upload (bands, payload)
    lo, hi  the payload is image[lo:hi]
    ptr     device address of the payload (set by Arena.upload)
    after   the bytes read back (set by Arena.download)"""

    def __init__(self, payload: int, phase: int = 0, data=None):
        if not 0 <= phase < 16 or payload < 0:
            raise ValueError("Guarded: phase in [0, 16), payload >= 0")
        self.payload, self.phase = payload, phase
        self.lo = GUARD + phase
        self.hi = self.lo + payload
        self.size = (self.hi + GUARD + _ALIGN - 1) // _ALIGN * _ALIGN
        self.image = _tiled(_PAT, self.size).copy()
        if data is None:
            self.image[self.lo:self.hi] = _tiled(_FILL, payload)
        else:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            if raw.size != payload:
                raise ValueError("Guarded: data does not fill the payload")
            self.image[self.lo:self.hi] = raw
        self.off = self.ptr = self.after = None

    # ------------------------------------------------------------ checks
    def check(self, after=None):
        """The first byte of either band that differs from what was
        uploaded, as a signed distance from the payload: -k is k bytes
        before its first byte (-1: the byte just before it), +k is k bytes
        past its last byte (+1: the byte just after it).  None: both bands
        are intact.  The band before the payload is looked at first."""
        after = self.after if after is None else after
        if after.shape != self.image.shape:
            raise ValueError("Guarded.check: not this buffer's bytes")
        d = first_diff(after[:self.lo], self.image[:self.lo])
        if d is not None:
            return d - self.lo
        d = first_diff(after[self.hi:], self.image[self.hi:])
        if d is not None:
            return d + 1
        return None

    def assert_guards(self, what="", after=None):
        after = self.after if after is None else after
        d = self.check(after)
        if d is not None:
            i = self.lo + d if d < 0 else self.hi + d - 1
            raise AssertionError(
                f"{what}: byte {d:+d} from the {'start' if d < 0 else 'end'} of the "
                f"{self.payload}-byte payload (phase {self.phase}) was written: "
                f"{int(after[i]):#04x}, was {int(self.image[i]):#04x}")

    def assert_unchanged(self, what="", after=None):
        """Bands and payload are bitwise what was uploaded (a source)."""
        after = self.after if after is None else after
        self.assert_guards(what, after)
        d = first_diff(after[self.lo:self.hi], self.image[self.lo:self.hi])
        assert d is None, f"{what}: payload byte {d} of {self.payload} was modified"

    def data(self, after=None) -> np.ndarray:
        """The payload as read back."""
        after = self.after if after is None else after
        return after[self.lo:self.hi]


class Arena:
    """Guarded buffers in one device allocation."""

    def __init__(self):
        self.bufs = []
        self.size = 0
        self.dev = None

    def add(self, payload: int, phase: int = 0, data=None) -> Guarded:
        g = Guarded(payload, phase, data)
        g.off = self.size
        self.size += g.size
        self.bufs.append(g)
        return g

    def image(self) -> np.ndarray:
        img = np.empty(self.size, np.uint8)
        for g in self.bufs:
            img[g.off:g.off + g.size] = g.image
        return img

    def upload(self, torch):
        """One host-to-device copy of every buffer; sets every g.ptr."""
        self.dev = torch.from_numpy(self.image()).to("cuda:0")
        base = self.dev.data_ptr()
        assert base % _ALIGN == 0, "device allocations are 256-byte aligned"
        for g in self.bufs:
            g.ptr = base + g.off + g.lo
        return self

    def download(self):
        """One device-to-host copy of every buffer (after the caller's
        synchronize); sets every g.after."""
        back = self.dev.cpu().numpy()
        for g in self.bufs:
            g.after = back[g.off:g.off + g.size]
        return self
