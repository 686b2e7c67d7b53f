"""The HIP-free logic of the batched reduce-to-all on the CPU
(csrc/many_host.hpp through tests/support/many_host_check.cpp): which kernel
an entry takes, the packing plan (16 segments and a thread limit per launch,
an entry split at a tile boundary, every tile covered exactly once, no edges
on a continuation), the overlap check of the table (target i against source
i allowed, against another entry's target or source refused, ranges that
only touch allowed) and the host fold's loop against a plain per-entry fold
with fake getmem and fold callbacks.

Each case runs the stand-alone program as a child process, once built plain
and once with AddressSanitizer + UBSan, which must report nothing.

test_interface: the header declares the three new symbols, the library
exports them, and the route counters are refused without OSGPU_TEST_HOOKS.
"""
import os
import subprocess
import sys

import pytest

import osgpu
from support import host_check_build

CASES = ["routes", "packing", "overlap", "fold1", "fold3", "fold8", "fold_empty"]


@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("many_host", san=request.param == "san")


@pytest.mark.parametrize("case", CASES)
def test_many_host(program, case):
    p = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_unknown_case_fails(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode == 1


_HOOK = """
import ctypes, sys
import osgpu
L = osgpu.load()
c = (ctypes.c_ulonglong * 7)()
rc = L.osgpu_test_many_routes(ctypes.byref(c))
print(rc, L.osgpu_last_error().decode())
"""


def test_interface():
    names = osgpu.header_symbols()
    for sym in ("osgpu_reduce_many", "osgpu_has_reduce_many", "osgpu_combine_many"):
        assert sym in names, f"{sym} is not declared in include/osgpu_reduce.h"
    assert "osgpu_test_many_routes" not in names, "a test hook in the public header"
    L = osgpu.load()
    for sym in ("osgpu_reduce_many", "osgpu_has_reduce_many", "osgpu_combine_many",
                "osgpu_test_many_routes"):
        assert hasattr(L, sym), f"libosgpu_reduce.so does not export {sym}"
    # 1 exactly where osgpu_has_op or osgpu_has_ext_op is
    for t in range(-1, 13):
        for op in range(-1, 9):
            want = 1 if (L.osgpu_has_op(t, op) or L.osgpu_has_ext_op(t, op)) else 0
            assert L.osgpu_has_reduce_many(t, op) == want, (t, op)
    # the route counters: refused without OSGPU_TEST_HOOKS=1, served with it
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    env.pop("OSGPU_TEST_HOOKS", None)
    off = subprocess.run([sys.executable, "-c", _HOOK], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=120)
    assert off.returncode == 0 and off.stdout.split()[0] != "0" and "test hooks are off" in off.stdout, \
        off.stdout[-2000:]
    on = subprocess.run([sys.executable, "-c", _HOOK], env=dict(env, OSGPU_TEST_HOOKS="1"),
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert on.returncode == 0 and on.stdout.split()[0] == "0", on.stdout[-2000:]
