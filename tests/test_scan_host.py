"""The HIP-free arithmetic of osgpu_scan on the CPU (csrc/scan_host.hpp through
tests/support/scan_host_check.cpp): how many members' sources a member folds
for P in 1..9 and both modes, the pulled-byte bound at nreduce = INT_MAX and
16-byte elements (size_t, no overflow), GETMEM's chunk walk covering [0, n)
exactly once, and the identity bytes of all 52 (type, op) pairs.

Each case runs the stand-alone program as a child process, once built plain
and once with AddressSanitizer + UBSan, which must report nothing.
"""
import subprocess

import pytest

from support import host_check_build

CASES = ["prefix", "bytes", "chunks", "identity"]


@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("scan_host", san=request.param == "san")


@pytest.mark.parametrize("case", CASES)
def test_scan_host(program, case):
    p = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_unknown_case_fails(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode == 1
