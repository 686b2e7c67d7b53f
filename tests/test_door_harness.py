"""The shared harness of the reduce doors' GPU tests (tests/support/gpu_doors.py)
without a GPU: check_members() and LauncherBatch.check() pass a correct image
and raise on every defect they exist to see, each injected alone.

The images are the uniform reduce's (every member holds the same value): int
sum of 3 members, 5 elements, and long double sum of 2 members, 3 elements.
check_members() reads a stub team whose heaps are numpy arrays -- the members
and one PE outside the set; LauncherBatch.check() reads guarded buffers whose
download is made up here.
"""
import numpy as np
import pytest

from support import gpu_doors as D
from support import uniform_cases as C

IMAGES = [("int", 3, 5), ("longdouble", 2, 3)]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _value_bytes(t, a):
    """a's bytes as a correct call leaves them: long double padding zero."""
    raw = _bytes(a).copy()
    if t == "longdouble":
        raw.reshape(-1, 16)[:, 10:] = 0
    return raw


# ------------------------------------------------------------ check_members
class StubTeam:
    def __init__(self, heaps, path):
        self.heaps, self.npes = heaps, len(heaps)
        self.last_paths = {pe: path for pe in range(self.npes)}

    def read(self, pe, off, nbytes):
        return self.heaps[pe][off:off + nbytes].copy()


class Heaps:
    """P members and PE P outside the set, after a correct team call."""

    def __init__(self, t, P, n):
        self.t, self.P, self.n, self.s = t, P, n, C.esize(t)
        self.soff, self.toff, self.hb = D.heap_layout(t, n, n)
        src = C.inputs(t, "sum", P + 1, n, 0x5EED)
        self.want = C.expected(t, "sum", src, 0, 0, P)
        self.before = {}
        for pe in range(P + 1):
            self.before[pe] = np.full(self.hb, 0xC3, np.uint8)
            self.before[pe][self.soff:self.soff + n * self.s] = _bytes(src[pe])
        self.tm = StubTeam({pe: b.copy() for pe, b in self.before.items()}, "team")
        for pe in range(P):
            self.target(pe)[:] = _value_bytes(t, self.want[pe])

    def target(self, pe):
        return self.tm.heaps[pe][self.toff:self.toff + self.n * self.s]

    def check(self, extra=None):
        D.check_members(self.tm, self.t, self.want, self.n, self.toff, self.hb, self.before,
                        list(range(self.P)), "team", "harness", extra)


@pytest.fixture(params=IMAGES, ids=lambda x: x[0])
def heaps(request):
    return Heaps(*request.param)


def test_members_correct_image_passes(heaps):
    heaps.check()
    heaps.check(extra=D.same_bytes_as_first)


MEMBER_DEFECTS = {
    "an element's low bit in the last member's target":
        lambda h: h.target(h.P - 1).__setitem__(2 * h.s, h.target(h.P - 1)[2 * h.s] ^ 1),
    "the byte just before the target": lambda h: h.tm.heaps[1].__setitem__(h.toff - 1, 0),
    "the byte just after the target": lambda h: h.tm.heaps[0].__setitem__(h.toff + h.n * h.s, 0),
    "a byte of a non-member's heap": lambda h: h.tm.heaps[h.P].__setitem__(h.toff + 1, 0),
    "a source byte": lambda h: h.tm.heaps[1].__setitem__(h.soff + 3, h.tm.heaps[1][h.soff + 3] ^ 0x80),
    "another path": lambda h: h.tm.last_paths.__setitem__(h.P - 1, "pull"),
}


@pytest.mark.parametrize("defect", MEMBER_DEFECTS)
def test_members_defect_is_seen(heaps, defect):
    MEMBER_DEFECTS[defect](heaps)
    with pytest.raises(AssertionError):
        heaps.check()


def test_members_long_double_padding_is_seen():
    h = Heaps("longdouble", 2, 3)
    h.target(1)[16 + 12] = 1
    with pytest.raises(AssertionError, match="padding"):
        h.check()


def test_members_uniform_hook_sees_two_members_differ(heaps):
    """Member 1 expects, and holds, a value one byte off member 0's: every
    shared check passes, the uniform door's hook does not."""
    h = heaps
    h.want[1] = h.want[1].copy()
    _bytes(h.want[1])[0] ^= 1
    h.target(1)[:] = _value_bytes(h.t, h.want[1])
    h.check()
    with pytest.raises(AssertionError, match="first member"):
        h.check(extra=D.same_bytes_as_first)


# ------------------------------------------------------- LauncherBatch.check
class Batch(D.LauncherBatch):
    """The uniform launcher's batch; launch() is replaced by a made-up download."""

    def __init__(self, t, P, n):
        super().__init__(t)
        self.pool = C.inputs(t, "sum", P, n, 0x5EED)
        self.val = [C.value(t, "sum", self.pool) for _ in range(P)]
        srcs = [self.arena.add(n * self.s, 0, self.pool[p]) for p in range(P)]
        dsts = [self.arena.add(n * self.s, 0) for _ in range(P)]
        self.c = self.case(srcs, dsts, "harness", op="sum", P=P, n=n)
        back = self.arena.image()
        for g in self.arena.bufs:
            g.after = back[g.off:g.off + g.size]
        self.fill()

    def fill(self):
        for q, g in enumerate(self.c.dsts):
            g.data()[:] = _value_bytes(self.t, self.val[q])

    def want(self, c, q):
        return self.val[q]


class UniformBatch(Batch):
    check_case = staticmethod(D.targets_identical)


@pytest.fixture(params=IMAGES, ids=lambda x: x[0])
def image(request):
    return request.param


def test_batch_correct_image_passes(image):
    Batch(*image).check()
    UniformBatch(*image).check()


def _flip(buf, i):
    buf[i] ^= 1


BATCH_DEFECTS = {
    "an element's low bit in the last target": lambda c: _flip(c.dsts[-1].data(), 2 * (c.dsts[-1].payload // c.n)),
    "the byte just before a target": lambda c: _flip(c.dsts[0].after, c.dsts[0].lo - 1),
    "the byte just after a target": lambda c: _flip(c.dsts[1].after, c.dsts[1].hi),
    "a byte deep in a target's guard band": lambda c: _flip(c.dsts[1].after, 5),
    "a byte of a source's guard band": lambda c: _flip(c.srcs[0].after, c.srcs[0].hi + 100),
    "a source byte": lambda c: _flip(c.srcs[1].data(), 3),
}


@pytest.mark.parametrize("defect", BATCH_DEFECTS)
def test_batch_defect_is_seen(image, defect):
    b = Batch(*image)
    BATCH_DEFECTS[defect](b.c)
    with pytest.raises(AssertionError):
        b.check()


def test_batch_long_double_padding_is_seen():
    b = Batch("longdouble", 2, 3)
    b.c.dsts[0].data()[2 * 16 + 15] = 0x80
    with pytest.raises(AssertionError, match="padding"):
        b.check()


def test_batch_uniform_hook_sees_two_members_differ(image):
    for cls in (Batch, UniformBatch):
        b = cls(*image)
        b.val[1] = b.val[1].copy()
        _bytes(b.val[1])[0] ^= 1
        b.fill()
        if cls is Batch:
            b.check()
        else:
            with pytest.raises(AssertionError, match="different bytes"):
                b.check()
