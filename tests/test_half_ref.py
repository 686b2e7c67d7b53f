"""half / bfloat16 reduce-to-all without a GPU: the numpy restatement
(tests/support/half_ref.py) against numpy.float16 arithmetic, the double route
and torch.bfloat16 on the CPU; hand-written edge cases of the semantics in
include/osgpu_reduce.h Part 1c; the element ops compiled for the host
(tests/support/half_check) against their independent oracle; the ABI.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import osgpu
from support import half_build
from support import half_ref as R

N = 1 << 20


def _pairs(t, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 16, size=N, dtype=np.uint32).astype(np.uint16)
    b = rng.integers(0, 1 << 16, size=N, dtype=np.uint32).astype(np.uint16)
    # half of the pairs near each other in exponent, so sums cancel and round
    b[::2] = (a[::2] & 0x7FFF) ^ rng.integers(0, 1 << 11, size=N // 2, dtype=np.uint32).astype(
        np.uint16) | (b[::2] & 0x8000)
    keep = ~(R.isnan(t, a) | R.isnan(t, b))
    return a[keep], b[keep]


def _double_route_half(op, a, b):
    """widen -> float64 operation (exact) -> numpy's one RNE step to float16."""
    x, y = R.widen("half", a).astype(np.float64), R.widen("half", b).astype(np.float64)
    with np.errstate(all="ignore"):
        return (x + y if op == "sum" else x * y).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("op", ["sum", "prod"])
def test_half_matches_numpy_float16_and_double_route(op):
    a, b = _pairs("half", 0xA1)
    assert a.size >= N // 2
    got = R.op2("half", op, a, b)
    fa, fb = a.view(np.float16), b.view(np.float16)
    with np.errstate(all="ignore"):
        want = (fa + fb if op == "sum" else fa * fb).view(np.uint16)
    nan = R.isnan("half", want)  # inf - inf, 0 * inf: the rule is checked by hand below
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all(got[nan] == 0xFE00)
    assert np.array_equal(_double_route_half(op, a, b)[~nan], got[~nan])


@pytest.mark.parametrize("op", ["sum", "prod"])
def test_bfloat16_matches_torch_cpu_and_double_route(op):
    import torch
    a, b = _pairs("bfloat16", 0xB2)
    assert a.size >= N // 2
    got = R.op2("bfloat16", op, a, b)
    ta = torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    tb = torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16)
    tr = (ta + tb) if op == "sum" else (ta * tb)
    want = tr.view(torch.int16).numpy().view(np.uint16)
    nan = R.isnan("bfloat16", want)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all(got[nan] == 0xFFC0)
    # the double route: float64 operation, then straight to bfloat16 via torch
    x = torch.from_numpy(R.widen("bfloat16", a).astype(np.float64))
    y = torch.from_numpy(R.widen("bfloat16", b).astype(np.float64))
    d = ((x + y) if op == "sum" else (x * y)).to(torch.bfloat16)
    d = d.view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(d[~nan], got[~nan])


@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("op", ["max", "min"])
def test_max_min_select_the_operands_bits(t, op):
    a, b = _pairs(t, 0xC3)
    got = R.op2(t, op, a, b)
    x, y = R.widen(t, a).astype(np.float64), R.widen(t, b).astype(np.float64)
    want = np.where((x > y) if op == "max" else (x < y), a, b)
    assert np.array_equal(got, want)


def _one(t, op, a, b):
    return int(R.op2(t, op, np.array([a], np.uint16), np.array([b], np.uint16))[0])


def test_hand_written_cases_half():
    one, ulp = 0x3C00, 0x1400  # 1.0; 2^-10 = ulp(1.0)
    # ties at the last bit, both directions: 1 + 2^-11 -> 1 (even), (1 + ulp) + 2^-11 -> 1 + 2 ulp
    assert _one("half", "sum", one, 0x1000) == 0x3C00
    assert _one("half", "sum", one + 1, 0x1000) == 0x3C02
    assert _one("half", "sum", one, ulp) == 0x3C01
    # just above / below the tie
    assert _one("half", "sum", one, 0x1001) == 0x3C01
    assert _one("half", "sum", one + 1, 0x0FFF) == 0x3C01
    # subnormal + subnormal (exact), up into the normals
    assert _one("half", "sum", 0x0001, 0x0002) == 0x0003
    assert _one("half", "sum", 0x03FF, 0x0001) == 0x0400
    assert _one("half", "prod", 0x0001, 0x3800) == 0x0000  # 2^-25: tie to even (0)
    assert _one("half", "prod", 0x0003, 0x3800) == 0x0002  # 1.5 * 2^-24: tie to even (2)
    # the largest finite + half an ulp (2^4) overflows to inf; a little less does not
    assert _one("half", "sum", 0x7BFF, 0x4C00) == 0x7C00
    assert _one("half", "sum", 0x7BFF, 0x4BFF) == 0x7BFF
    assert _one("half", "sum", 0xFBFF, 0xCC00) == 0xFC00
    # invalid operations: the negative default NaN
    assert _one("half", "sum", 0x7C00, 0xFC00) == 0xFE00
    assert _one("half", "sum", 0xFC00, 0x7C00) == 0xFE00
    assert _one("half", "prod", 0x0000, 0x7C00) == 0xFE00
    # sNaN first against qNaN second, and the reverse: the first, quieted, sign and payload kept
    assert _one("half", "sum", 0xFC01, 0x7E05) == 0xFE01
    assert _one("half", "sum", 0x7E05, 0xFC01) == 0x7E05
    assert _one("half", "prod", 0x3C00, 0x7C15) == 0x7E15
    # max / min: the second operand on equality and on any NaN
    assert _one("half", "max", 0x0000, 0x8000) == 0x8000
    assert _one("half", "max", 0x8000, 0x0000) == 0x0000
    assert _one("half", "min", 0x3C00, 0x7C01) == 0x7C01  # min(x, sNaN): the NaN, not quieted
    assert _one("half", "min", 0x7C01, 0x3C00) == 0x3C00  # min(NaN, x) = x
    assert _one("half", "max", 0x0001, 0x0002) == 0x0002  # subnormals compare as values


def test_hand_written_cases_bfloat16():
    one = 0x3F80
    assert _one("bfloat16", "sum", one, 0x3B80) == 0x3F80      # 1 + 2^-8: tie to even
    assert _one("bfloat16", "sum", one + 1, 0x3B80) == 0x3F82  # tie, odd: up
    assert _one("bfloat16", "sum", one, 0x3B81) == 0x3F81
    assert _one("bfloat16", "sum", 0x0001, 0x0002) == 0x0003   # subnormals kept
    assert _one("bfloat16", "sum", 0x007F, 0x0001) == 0x0080
    assert _one("bfloat16", "sum", 0x7F7F, 0x7B00) == 0x7F80   # largest + half an ulp (2^119) -> inf
    assert _one("bfloat16", "sum", 0x7F7F, 0x7AFF) == 0x7F7F
    assert _one("bfloat16", "sum", 0x7F80, 0xFF80) == 0xFFC0
    assert _one("bfloat16", "prod", 0x8000, 0x7F80) == 0xFFC0
    assert _one("bfloat16", "sum", 0xFF81, 0x7FC5) == 0xFFC1
    assert _one("bfloat16", "sum", 0x7FC5, 0xFF81) == 0x7FC5
    assert _one("bfloat16", "max", 0x0000, 0x8000) == 0x8000
    assert _one("bfloat16", "max", 0x8000, 0x0000) == 0x0000
    assert _one("bfloat16", "min", one, 0x7F81) == 0x7F81
    assert _one("bfloat16", "min", 0x7F81, one) == one


def test_fold_orders_differ_in_the_last_bit():
    # 1 + 2^-11 + 2^-11: (1 + t) + t = 1 (two ties to even), (t + t) + 1 = 1 + ulp
    src = [np.array([0x3C00], np.uint16), np.array([0x1000], np.uint16),
           np.array([0x1000], np.uint16)]
    res = [int(r[0]) for r in R.to_all("half", "sum", src)]
    assert res == [0x3C00] * 3  # every member's order adds 1 before the second t
    assert int(R.fold("half", "sum", [1, 2, 0], src)[0]) == 0x3C01
    assert int(R.fold("half", "sum", [0, 1, 2], src)[0]) == 0x3C00


@pytest.fixture(scope="module")
def lib():
    osgpu.build()
    return osgpu.load()


def _run_check(path):
    p = subprocess.run([path], capture_output=True, text=True, timeout=600)
    rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    assert len(rows) == 8, p.stdout + p.stderr
    assert {(r["type"], r["op"]) for r in rows} == {(t, o) for t in R.TYPES for o in R.OPS}
    for r in rows:
        assert r["pairs"] >= 65536 * 512
        assert r["elem_mismatches"] == 0 and r["fast_contract_mismatches"] == 0, r
    assert p.returncode == 0, p.stderr[-2000:]


def test_half_check_reports_zero_mismatches():
    _run_check(half_build.build())


def test_half_check_under_ubsan():
    """The same program with the host code under -fsanitize=undefined,
    stand-alone (a program with its own main; the test preloads nothing)."""
    _run_check(half_build.build(ubsan=True))


def test_header_declares_and_library_exports_the_extension(lib):
    names = set(osgpu.header_symbols())
    want = [f"osgpu_{t}_{o}_reduce" for t in osgpu.EXT_TYPES for o in osgpu.EXT_OPS]
    want += ["osgpu_reduce_ext", "osgpu_has_ext_op"]
    for n in want:
        assert n in names, n
        assert hasattr(lib, n), n
    assert not [n for n in want if n.endswith("_to_all")]
    assert osgpu.type_code("half") == 9 and osgpu.type_code("bfloat16") == 10
    assert osgpu.type_code("short") == 0 and osgpu.type_code("complexd") == 8
    assert osgpu.ext_reduce("half", "sum") is not None


def test_type_tables(lib):
    on = [(t, o) for t in range(-1, 13) for o in range(-1, 9) if lib.osgpu_has_ext_op(t, o) == 1]
    assert on == [(t, o) for t in (9, 10) for o in (0, 1, 5, 6)]
    assert len(on) == 8
    for t in (9, 10):
        assert [lib.osgpu_has_op(t, o) for o in range(7)] == [0] * 7
        assert lib.osgpu_type_size(t) == 2
    assert lib.osgpu_type_size(11) == 0


_AND_CALL = """
import ctypes, sys
sys.path[:0] = {paths!r}
import osgpu
L = osgpu.load()
buf = (ctypes.c_uint16 * 8)()
ps = (ctypes.c_long * 128)()
L.osgpu_reduce_ext(9, osgpu.OPS.index("and"), ctypes.addressof(buf), ctypes.addressof(buf), 4,
                   0, 0, 1, None, ctypes.addressof(ps))
print("returned")
"""


def test_reduce_ext_refuses_bit_ops(lib):
    """op `and` through osgpu_reduce_ext dies with a message (child process;
    no GPU needed: the check comes before anything else)."""
    paths = [os.path.dirname(os.path.dirname(osgpu.__file__))]
    env = dict(os.environ, OSGPU_NO_TORCH="1")
    p = subprocess.run([sys.executable, "-c", _AND_CALL.format(paths=paths)], capture_output=True,
                       text=True, timeout=120, env=env)
    assert p.returncode != 0
    assert "returned" not in p.stdout
    assert "osgpu_reduce_ext" in p.stderr and "not an extension reduction" in p.stderr
