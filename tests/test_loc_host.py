"""The host arithmetic of osgpu_reduce_loc on the CPU (csrc/loc_host.hpp and
csrc/elem_ops.hpp LocStep compiled for the host, through
tests/support/loc_host_check.cpp): the pair table, the byte counts at
nreduce = INT_MAX (size_t, no overflow), the overlap rule, the two-stream
vector split at every head, GETMEM's chunk, the walk over more than 8 inputs
-- and the fold itself over cases this test writes to a file, compared with
the closed form of tests/support/loc_cases.py: all 16 pairs on the tie inputs
at P in {1, 2, 3, 8, 9, 17} (9 and 17: the chunked fold with the pair fed
back), the form without index sources on a strided set's PE numbers, and
nreduce in {0, 1}.

Each case runs the stand-alone program as a child process, once built plain
and once with AddressSanitizer + UBSan, which must report nothing.
"""
import subprocess

import numpy as np
import pytest

import osgpu
from support import loc_cases as C
from support import host_check_build


@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("loc_host", san=request.param == "san")


def record(t, op, vals, locs=None, member=None):
    n = len(vals[0])
    if locs is None:
        idx = C.const_indices(member, n)
    else:
        idx = locs
    v, i = C.expected(t, op, vals, idx)
    out = [np.array([osgpu.type_code(t), osgpu.OPS.index(op), len(vals), n, int(locs is not None)],
                    np.int32).tobytes()]
    out += [np.ascontiguousarray(x).tobytes() for x in vals]
    out += ([np.ascontiguousarray(x, np.int32).tobytes() for x in locs] if locs is not None
            else [np.array(member, np.int32).tobytes()])
    out += [np.ascontiguousarray(v).tobytes(), i.astype(np.int32).tobytes()]
    return b"".join(out)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("loc") / "cases.bin"
    recs = []
    for t, op in C.PAIRS:
        for P in (1, 2, 3, 8, 9, 17):
            vals, locs = C.tie_case(t, op, P, 211, 0xC0DE + P)
            recs.append(record(t, op, vals, locs))
        vals = C.tie_values(t, 3, 97, 0xBEE)
        recs.append(record(t, op, vals, member=C.member_pes(1, 1, 3)))
        vals = C.tie_values(t, 9, 97, 0xBEF)
        recs.append(record(t, op, vals, member=list(range(8, -1, -1))))
        for n in (0, 1):
            vals, locs = C.tie_values(t, 3, n, 5), C.tie_indices(3, n, 5)
            recs.append(record(t, op, vals, locs))
    path.write_bytes(b"".join(recs))
    return str(path)


def test_arith(program):
    p = subprocess.run([program, "arith"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_fold_matches_the_closed_form(program, cases):
    p = subprocess.run([program, "fold", cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_a_wrong_expectation_is_seen(program, tmp_path):
    """The program compares: a record whose expected index is off fails."""
    vals, locs = C.tie_case("float", "max", 3, 64, 1)
    good = record("float", "max", vals, locs)
    bad = bytearray(good)
    bad[-4] ^= 1
    f = tmp_path / "bad.bin"
    f.write_bytes(bytes(bad))
    p = subprocess.run([program, "fold", str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 1 and "index 63" in p.stdout, p.stdout[-2000:]


def test_unknown_case_fails(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode == 1
