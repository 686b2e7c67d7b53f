"""The host arithmetic of osgpu_reduce_wsum on the CPU (csrc/wsum_host.hpp and
csrc/elem_ops.hpp WsumStep compiled for the host, through
tests/support/wsum_host_check.cpp): the pair table, the byte counts at
nreduce = INT_MAX (size_t, no overflow), the carry scratch rule, GETMEM's
chunk, the walk over more than 8 members -- and the fold itself over cases this
test writes to a file, compared with tests/support/wsum_ref.py: both types on
the order-sensitive inputs at P in {1, 2, 3, 8, 9, 17} (9 and 17: the chunked
fold with the float carry), the NaN / overflow table, every 16-bit pattern as
one member, and nreduce in {0, 1}.

Each case runs the stand-alone program as a child process, once built plain
and once with AddressSanitizer + UBSan, which must report nothing.
"""
import subprocess

import numpy as np
import pytest

import osgpu
from support import host_check_build
from support import wsum_ref as W

# the program's row of host_check_build's table: no further sources, the
# headers watched, the HIP headers for elem_ops.hpp's marks
host_check_build.CHECKS.setdefault(
    "wsum_host", ([], ["wsum_host.hpp", "scan_host.hpp", "elem_ops.hpp"],
                  host_check_build.HIP_HEADERS))


@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("wsum_host", san=request.param == "san")


def record(t, srcs):
    n = len(srcs[0])
    out = [np.array([osgpu.type_code(t), len(srcs), n], np.int32).tobytes()]
    out += [np.ascontiguousarray(x, np.uint16).tobytes() for x in srcs]
    out += [W.wsum(t, "float", srcs).astype(np.uint32).tobytes(),
            W.wsum(t, t, srcs).astype(np.uint16).tobytes()]
    return b"".join(out)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("wsum") / "cases.bin"
    recs = []
    for t in W.TYPES:
        for P in (1, 2, 3, 8, 9, 17):
            srcs = W.inputs(t, P, 211, 0xC0DE + P)
            W.assert_discriminating(t, srcs)
            recs.append(record(t, srcs))
        for P in (2, 3, 8):
            recs.append(record(t, W.nan_table(t, P)))
        recs.append(record(t, [np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)]))
        for n in (0, 1):
            recs.append(record(t, W.inputs(t, 3, n, 5)))
    path.write_bytes(b"".join(recs))
    return str(path)


def test_arith(program):
    p = subprocess.run([program, "arith"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_fold_matches_the_definition(program, cases):
    p = subprocess.run([program, "fold", cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_a_per_step_expectation_is_seen(program, tmp_path):
    """The program compares: a record that expects the per-step sum fails."""
    srcs = W.inputs("bfloat16", 4, 64, 1)
    good = record("bfloat16", srcs)
    bad = good[:-128] + W.per_step("bfloat16", srcs).astype(np.uint16).tobytes()
    assert bad != good
    f = tmp_path / "bad.bin"
    f.write_bytes(bad)
    p = subprocess.run([program, "fold", str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 1 and "element 2:" in p.stdout, p.stdout[-2000:]


def test_unknown_case_fails(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode == 1
