"""The x87 team folds on the MI355X wave by wave: every fold mode of
csrc/x87.hpp team_fold_sum_prod (F_NEAR, F_SAME_NEAR, F_SAME, F_FULL, chosen by
a 64-lane ballot on the device, per element on the host), with no, a few and
64 lanes of the wave on the general op, at every member count 2..8 -- each its
own device code (dispatch_members, the fold groups split at P / 2, the
8-member sum's spills) -- and team_fold_minmax's pick among tied extremes.

Inputs: tests/support/x87_wave_cases.py, runs of 64 elements = one wave of
ld_team_kernel each; what they contain is asserted without a GPU, and the
host build of the same source is checked on them, in
tests/test_x87_wave_ref.py.  Expected values: the oracle's reduce-to-all.

a. osgpu_team_combine, sum / prod / max / min, 2..8 members, every array
   16-byte aligned (ld_team_kernel<.., VEC = true>) and every array 8 bytes
   off (VEC = false): every member's 10 value bytes, zero padding, guards.
b. osgpu.team_uniform (ld_uniform_kernel: the ascending fold by the
   two-operand add / mul, no fold modes) on the same inputs.
c. Device twins, through osgpu.combine, of the host's tie and
   equal-and-opposite operand tests.
d. One shmem_longdouble_<op>_to_all per op on a 3-member team, path "team":
   the kernel sees the heaps' addresses, the runs are no longer whole waves.
"""
import ctypes

import pytest

import osgpu
from support import gpu_doors as D
from support import team as T
from support import x87_wave_cases as W
from support.gpu_doors import torch_cuda  # noqa: F401  (fixture)
from test_gpu_x87 import _check

pytestmark = pytest.mark.gpu

OPS = ("sum", "prod", "max", "min")
MEMBERS = range(2, 9)


class WaveBatch(D.LauncherBatch):
    """Cases of one launcher ("team": osgpu_team_combine, "uniform":
    osgpu_team_uniform) on the wave inputs; the sources of one (inputs, P,
    phase) are uploaded once and shared by the ops that read them."""

    def __init__(self, kernel):
        super().__init__("longdouble")
        self.kernel = kernel
        self.sources = {}

    def add(self, op, P, phase):
        key = (op if op in ("sum", "prod") else "minmax", P, phase)
        if key not in self.sources:
            self.sources[key] = [self.arena.add(x.size * 16, phase, x) for x in W.inputs(op, P)]
        n = W.inputs(op, P)[0].size
        dsts = [self.arena.add(n * 16, phase) for _ in range(P)]
        self.case(self.sources[key], dsts, f"every array at phase {phase}", kernel=self.kernel,
                  op=op, P=P, n=n)

    def call(self, c, sp):
        d, s = D.ptrs(c.dsts), D.ptrs(c.srcs)
        if self.kernel == "uniform":
            osgpu.team_uniform("longdouble", c.op, d, s, c.n, stream=sp)
            return
        L = osgpu.load()
        rc = L.osgpu_team_combine(osgpu.type_code("longdouble"), osgpu.OPS.index(c.op), c.P,
                                  (ctypes.c_void_p * c.P)(*d), (ctypes.c_void_p * c.P)(*s), c.n, sp)
        assert rc == 0, (self.describe(c), L.osgpu_last_error())

    def want(self, c, q):
        return W.want(c.op, c.P)[0 if self.kernel == "uniform" else q]

    def check_case(self, c, what):
        if self.kernel == "uniform":
            D.targets_identical(c, what)


@pytest.mark.parametrize("P", MEMBERS)
def test_team_launcher_every_mode(torch_cuda, P):
    b = WaveBatch("team")
    for phase in (0, 8):
        for op in OPS:
            b.add(op, P, phase)
    b.launch(torch_cuda).check()


@pytest.mark.parametrize("P", MEMBERS)
def test_uniform_launcher(torch_cuda, P):
    b = WaveBatch("uniform")
    for phase in (0, 8):
        for op in OPS if P in (3, 8) else OPS[:2]:
            b.add(op, P, phase)
    b.launch(torch_cuda).check()


def test_device_tie_of_exponent_and_top_word(torch_cuda):
    a, b = W.tie_pairs(20_000)
    _check(torch_cuda, a, b)
    _check(torch_cuda, b, a)


def test_device_equal_and_opposite_operands(torch_cuda):
    a, b = W.equal_opposite_operands(4_000)
    _check(torch_cuda, a, a)
    _check(torch_cuda, a, b)
    _check(torch_cuda, b, a)


def test_collective_on_the_wave_inputs(torch_cuda):
    P, t = 3, "longdouble"
    n = max(W.inputs(op, P)[0].size for op in OPS)
    soff, toff, hb = D.heap_layout(t, n, n)
    tm = T.Team(P, hb, device=True)
    for op in OPS:
        src = W.inputs(op, P)
        n = src[0].size
        for pe in range(P):
            tm.fill(pe, 0, hb, 0xC3)
            tm.write(pe, soff, src[pe])
        before = {pe: tm.read(pe, 0, hb) for pe in range(P)}
        tm.run(t, op, toff, soff, n)
        D.check_members(tm, t, W.want(op, P), n, toff, hb, before, list(range(P)), "team",
                        f"to_all {t} {op} P={P} n={n}")
