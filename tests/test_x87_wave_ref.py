"""The wave-by-wave inputs of tests/support/x87_wave_cases.py, without a GPU.

a. What the device tests (tests/test_gpu_x87_waves.py) rely on is asserted
   here with the oracle alone: every run of 64 elements takes the fold mode
   its class names (wave_mode, the gate restated from the constants the host
   build exports), every mode has runs with no, a few and 64 event lanes, and
   the oracle's running values (the inclusive scan of the ascending fold, and
   of the last member's fold) show the events: exact zeros, running values far
   below the next operand, growth past every input, non-normal running values
   that become normal again, NaNs from the first, a middle and the last member.
b. The host build of csrc/x87.hpp (x87check_team: one element at a time, so
   every lane in its own mode) is bit-exact on the same inputs.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
from support import scan_cases as S
from support import team as T
from support import x87_wave_cases as W

MEMBERS = range(2, 9)


@pytest.fixture(scope="module")
def x87():
    return T.build_x87check()


def _scan(op, srcs, order):
    """[(significand, exponent, sign, normal)] of the running values of the
    fold of `srcs` in `order`, the oracle's"""
    out = []
    for x in S.inclusive("longdouble", op, [srcs[p] for p in order]):
        m, e, s = W.fields(x)
        out.append((m, e, s, W.is_normal(m, e)))
    return out


def _isnan(m, e):
    return (e == W.EMAX) & ((m << np.uint64(1)) != 0)


def test_gate_constants_are_the_headers(x87):
    spread, lo, hi = W.gate()
    assert 0 < spread < 30 and 30 <= lo < hi <= W.EMAX - 2     # the near adds' preconditions
    assert x87.x87check_gate(3) == -1


def test_layout():
    runs = W.sum_runs()
    for cls in W.CLASSES:
        for dens in W.DENSITIES:
            assert sum(1 for r in runs if r[0] == cls and r[2] == dens) == 2
    for cls in W.CLASSES:
        for lanes in W.FEW[cls]:
            assert 1 <= len(lanes) <= 8
    few = [lane for cls in W.CLASSES for lanes in W.FEW[cls] for lane in lanes]
    assert 0 in few and 63 in few and len({len(x) for c in W.CLASSES for x in W.FEW[c]}) >= 4
    assert W.N_SUM == 64 * 24 + 37


@pytest.mark.parametrize("P", MEMBERS)
def test_every_run_takes_its_mode_at_every_density(P):
    srcs, runs, event, kind = W.sum_case(P)
    assert all(s.size == W.N_SUM for s in srcs) and len(runs) == W.n_runs(W.N_SUM)
    whole = runs[:-1]
    modes = [W.wave_mode(srcs, r) for r in range(len(runs))]
    for r, (cls, rep, dens, lanes) in enumerate(runs):
        assert modes[r] == cls, f"run {r} ({cls}, {dens}) takes {modes[r]}"
    assert runs[-1][0] == "near" and W.N_SUM - 64 * len(whole) == 37
    asc = _scan("sum", srcs, list(range(P)))
    last = _scan("sum", srcs, [P - 1] + list(range(P - 1)))
    for mode in W.CLASSES:
        mine = [r for r in range(len(whole)) if modes[r] == mode]
        assert len(mine) >= 6
        lanes = [int(event[64 * r:64 * r + 64].sum()) for r in mine]
        assert sum(1 for c in lanes if c == 0) >= 2
        assert sum(1 for c in lanes if 1 <= c <= 8) >= 2
        assert sum(1 for c in lanes if c == 64) >= 1
        # a run without event lanes has none by the oracle either: every input
        # and running value normal, no running value 32 binades below its operands
        for r in mine:
            if event[64 * r:64 * r + 64].any():
                continue
            sl = slice(64 * r, 64 * r + 64)
            for scan in (asc, last):
                for j, (m, e, s, nrm) in enumerate(scan):
                    assert nrm[sl].all(), (mode, r, j)
                    if j:
                        assert (e[sl] + 32 > scan[j - 1][1][sl]).all(), (mode, r, j)
    # every kind of event in every class, at the first, a middle and the last member
    for cls in W.CLASSES:
        seen = {k for r, run in enumerate(runs) if run[0] == cls for k in kind[64 * r:64 * r + 64] if k}
        assert seen >= set(W.SUM_KINDS[cls]), (cls, seen)


@pytest.mark.parametrize("P", MEMBERS)
def test_sum_events_by_the_oracle(P):
    srcs, runs, event, kind = W.sum_case(P)
    f = [W.fields(s) for s in srcs]
    inc = _scan("sum", srcs, list(range(P)))
    near_runs = np.zeros(W.N_SUM, bool)
    for r, run in enumerate(runs):
        near_runs[64 * r:64 * r + 64] = run[0] in ("near", "same_near")
    # an exact zero after member 1
    zero = (inc[1][0] == 0) & (inc[1][1] == 0) & (f[0][0] != 0) & (f[1][0] != 0)
    assert zero.sum() > 0 and (zero & near_runs).sum() > 0
    assert not zero[~event].any()
    # a running value more than 30 binades below the next operand, inside a
    # wave of a near mode (two members have no later round there)
    far = np.zeros(W.N_SUM, bool)
    for j in range(1, P):
        far |= inc[j - 1][1] + 30 < f[j][1]
    assert far.sum() > 0
    if P > 2:
        assert (far & near_runs).sum() > 0
    # a result exponent above every input's
    emax = np.max([x[1] for x in f], axis=0)
    grown = inc[-1][3] & (inc[-1][1] > emax)
    assert grown.sum() > 0 and (grown & near_runs).sum() > 0
    # a non-normal running value (no NaN, no infinity) that is normal again later
    back = np.zeros(W.N_SUM, bool)
    for j in range(P - 1):
        low = ~inc[j][3] & (inc[j][1] == 0)
        for k in range(j + 1, P):
            back |= low & inc[k][3]
    if P > 2:                   # (two members: one add, no running value before the last)
        assert back.sum() > 0
    _nan_sources(P, f, inc)
    # (two members: x0 + x1 and x1 + x0 are the same add)
    # the order matters somewhere in every class: member 0's result against the last member's
    if P > 2:
        want = W.want("sum", P)
        differ = (O.value_bytes(want[0]).reshape(-1, 10) != O.value_bytes(want[P - 1]).reshape(-1, 10)).any(1)
        for cls in W.CLASSES:
            mask = np.zeros(W.N_SUM, bool)
            for r, run in enumerate(runs):
                mask[64 * r:64 * r + 64] = run[0] == cls
            assert (differ & mask).sum() > 0, cls


def _nan_sources(P, f, inc):
    """a NaN result from a NaN of the first, a middle and the last member"""
    out = _isnan(inc[-1][0], inc[-1][1])
    for p in {0, P // 2, P - 1}:
        assert (_isnan(f[p][0], f[p][1]) & out).sum() > 0, p


@pytest.mark.parametrize("P", MEMBERS)
def test_prod_events_by_the_oracle(P):
    srcs, event, kind = W.prod_case(P)
    f = [W.fields(s) for s in srcs]
    inc = _scan("prod", srcs, list(range(P)))
    last = _scan("prod", srcs, [P - 1] + list(range(P - 1)))
    assert {k for k in kind if k} == set(W.PROD_KINDS)
    # without an event every factor and every running product is normal: all mul_fast
    for scan in (inc, last):
        for m, e, s, nrm in scan:
            assert nrm[~event].all()
    assert all(W.is_normal(x[0], x[1])[~event].all() for x in f)
    for r in range(W.n_runs(W.N_PROD)):
        c = int(event[64 * r:64 * r + 64].sum())
        assert c == (0, len(W.FEW["full"][(r // 3) % 2]), 64)[r % 3] or r == W.n_runs(W.N_PROD) - 1
    final = [scan[-1] for scan in (inc, last)]
    # on the denormal grid; overflowed; all ones rounded up (a power of two
    # from factors that are none); 0 * inf
    assert any(((m != 0) & (e == 0) & (m >> np.uint64(63) == 0)).sum() > 0
               for scan in (inc, last) for m, e, s, nrm in scan)
    assert any(((e == W.EMAX) & (m == np.uint64(W.TOP))).sum() > 0 for m, e, s, nrm in final)
    pow2 = np.zeros(W.N_PROD, bool)
    for scan, order in ((inc, list(range(P))), (last, [P - 1] + list(range(P - 1)))):
        for j in range(1, P):
            pow2 |= scan[j][3] & (scan[j][0] == np.uint64(W.TOP)) & (scan[j - 1][0] != np.uint64(W.TOP)) \
                & (f[order[j]][0] != np.uint64(W.TOP))
    assert pow2.sum() > 0
    back = np.zeros(W.N_PROD, bool)
    for scan in (inc, last):
        for j in range(P - 1):
            for k in range(j + 1, P):
                back |= ~scan[j][3] & (scan[j][1] == 0) & (scan[j][0] != 0) & scan[k][3]
    if P > 2:
        assert back.sum() > 0
    _nan_sources(P, f, inc)
    defnan = (inc[-1][0] == np.uint64(0xC000000000000000)) & (inc[-1][1] == W.EMAX) & (inc[-1][2] == 1)
    assert (defnan & ~np.logical_or.reduce([_isnan(x[0], x[1]) for x in f])).sum() > 0


@pytest.mark.parametrize("P", MEMBERS)
def test_minmax_ties_reach_every_member(P):
    """Among the elements without an unordered operand, the highest member
    holding the extreme (x87.hpp team_fold_minmax's t1) is each of 0..P-1,
    alone and (from member 1 on) tied; and some tie's first and next-highest
    holders are different encodings (+0 and -0)."""
    srcs, un = W.minmax_case(P)
    f = [W.fields(s) for s in srcs]
    assert np.array_equal(un, np.logical_or.reduce([W.unordered(x[0], x[1]) for x in f]))
    for r in range(W.n_runs(W.N_MINMAX) - 1):
        c = int(un[64 * r:64 * r + 64].sum())
        assert c == (0, len(W.FEW["same"][(r // 3) % 2]), 64)[r % 3]
    v = np.stack(srcs)[:, ~un]
    raw = np.stack([O.value_bytes(s).reshape(-1, 10) for s in srcs])[:, ~un]
    for ext in (v.max(0), v.min(0)):
        holds = v == ext
        t1 = P - 1 - np.argmax(holds[::-1], axis=0)
        count = holds.sum(0)
        for p in range(P):
            assert ((t1 == p) & (count == 1)).any(), p
            if p:
                assert ((t1 == p) & (count > 1)).any(), p
        if P > 2:
            t0 = np.argmax(holds, axis=0)
            below = holds.copy()
            below[t1, np.arange(t1.size)] = False
            t2 = P - 1 - np.argmax(below[::-1], axis=0)
            cols = np.flatnonzero(count > 2)
            assert (raw[t0[cols], cols] != raw[t2[cols], cols]).any(1).sum() > 0


@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
@pytest.mark.parametrize("P", MEMBERS)
def test_host_build_is_bit_exact(x87, op, P):
    srcs = W.inputs(op, P)
    want = W.want(op, P)
    got = [np.zeros_like(srcs[0]) for _ in range(P)]
    sp = (ctypes.c_void_p * P)(*[s.ctypes.data for s in srcs])
    dp = (ctypes.c_void_p * P)(*[g.ctypes.data for g in got])
    assert x87.x87check_team(O.OPS.index(op), P, sp, dp, srcs[0].size) == 0
    for q in range(P):
        w = O.value_bytes(want[q]).reshape(-1, 10)
        g = O.value_bytes(got[q]).reshape(-1, 10)
        bad = np.nonzero((w != g).any(1))[0]
        assert bad.size == 0, f"member {q}: {bad.size} mismatches at {bad[:5]} (runs {bad[:5] // 64})"
