"""The HIP-free arithmetic of osgpu_reduce_scatter's host paths on the CPU
(csrc/rscatter_host.hpp through tests/support/rscatter_host_check.cpp): block
m's bytes in size_t (P * nreduce above INT_MAX), GETMEM's chunk walk, and the
host fold's loop -- one getmem of exactly the block per peer, none at P = 1 --
over heaps, targets and peer buffers allocated to the byte.

Each case runs the stand-alone program as a child process, once built plain
and once with AddressSanitizer + UBSan, which must report nothing.
"""
import subprocess

import pytest

from support import host_check_build

CASES = ["blocks", "chunks", "fold1", "fold3", "fold8", "fold_empty"]


@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("rscatter_host", san=request.param == "san")


@pytest.mark.parametrize("case", CASES)
def test_rscatter_host(program, case):
    p = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_unknown_case_fails(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode == 1
