"""The pair matrix without a GPU (tests/support/matrix_cases.py).

1. The matrix covers every (type, op) the library lists -- 52 pairs per door
   and raw kernel, 16 for the location door -- enumerated from osgpu.has_op.
2. The inputs discriminate: for every pair, at P in {3, 8} and the whole-tile
   lengths the GPU tests run (n_tile of every kernel, the collective's length),
   the oracle alone shows that both routes of the branch-free fold are taken,
   that NaNs come from a first member, a middle member and from arithmetic,
   that a fold starting at the wrong member differs in 16 elements or more,
   that the complex products reach libgcc's recovery with and without a NaN
   left, and the max / min, integer and long double conditions.  n_small
   (W + 1 elements, two vectors at the most) cannot hold counts of 4 and 16:
   there the layout puts an ordinary vector first and a NaN vector second, and
   that is what is asserted.
3. The premise of the fast route: tests/support/fast_fold_check.cpp, built
   plain and with ASan + UBSan and run as a program -- over all triples of an
   alphabet, a Fast fold without a NaN part is the Elem fold bit for bit and a
   NaN part survives the next step; and the kernels' route (fast fold per
   vector, exact refold when flagged) over the matrix inputs gives the oracle's
   bytes, both routes taken for every pair.
"""
import subprocess

import numpy as np
import pytest

import oracle as O
import osgpu
from support import host_check_build
from support import half_ref as R
from support import matrix_cases as X

ARITH = [(t, op) for t in X.FLOATING for op in ("sum", "prod")]


# ------------------------------------------------------------- 1. coverage
def library_pairs():
    pairs = [(t, op) for t in osgpu.TYPES for op in osgpu.OPS if osgpu.has_op(t, op)]
    pairs += [(t, op) for t in osgpu.EXT_TYPES for op in osgpu.EXT_OPS]
    return pairs


def test_the_matrix_covers_every_pair_of_every_door_and_kernel():
    lib = library_pairs()
    assert len(lib) == 52 and len(set(lib)) == 52
    for door in X.DOORS:
        got = X.door_pairs(door)
        if door == "loc":
            want = [(t, op) for t, op in lib if op in ("max", "min") and t != "longdouble"]
            assert len(want) == 16
        else:
            want = lib
        assert sorted(got) == sorted(want), door
        # the GPU test is parametrized over door_types and loops over ops_of
        looped = [(t, op) for t in X.door_types(door) for op in X.ops_of(t)
                  if door != "loc" or op in ("max", "min")]
        assert sorted(looped) == sorted(want), door
    for kernel in X.RAW_KERNELS:
        got = X.raw_pairs(kernel)
        want = [p for p in lib if not (kernel == "team_scan" and p[0] == "longdouble")]
        assert sorted(got) == sorted(want), kernel
    assert len(X.raw_pairs("team_scan")) == 48 and len(X.raw_pairs("team_uniform")) == 52
    assert set(X.P8_PAIRS) <= set(lib)


def test_lengths_are_a_head_a_whole_tile_a_partial_tile_and_a_tail():
    for t in X.TYPES:
        W = X.width(t)
        assert X.n_small(t) == W + 1
        for P in X.MEMBERS:
            assert X.n_tile("team_uniform", t, P) == 64 * P * W + W + W - 1
            assert X.n_tile("team_scan", t, P) == 64 * W + W + W - 1
            assert X.n_tile("combine_shifted", t, P) == 128 * W + W + W - 1
        for door in X.DOORS:
            if door == "loc" and t not in X.door_types(door):
                continue
            n = X.n_collective(door, t)
            assert n * X.esize(t) > 4096 and (n * X.esize(t)) % 2048, (door, t)
            assert n >= X.n_tile(X._DOOR_KERNEL[door], t, 3)


# ------------------------------------------------------ 2. input conditions
def lengths_run(t, P):
    """The whole-tile lengths some GPU test runs (t, P) at."""
    ns = {X.n_tile(k, t, P) for k in X.RAW_KERNELS}
    if P == 3:
        ns |= {X.n_collective(d, t) for d in ("scan_inc", "uniform", "many")}
        ns.add(3 * X.n_collective("rscatter", t))
    return sorted(ns)


@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("t,op", X.ALL_PAIRS, ids=lambda x: x)
def test_inputs_discriminate(t, op, P):
    W = X.width(t)
    for n in lengths_run(t, P):
        c = X.conditions(t, op, X.matrix_inputs(t, op, P, n, 0x3A7 + P))
        w = f"{t} {op} P={P} n={n}: {c}"
        if (t, op) in ARITH:
            for h in (0, 1 % W):
                nv = c[f"vectors_h{h}"]
                assert 4 * c[f"fast_vectors_h{h}"] >= nv, w
                assert 8 * c[f"nan_vectors_h{h}"] >= nv, w
                assert c[f"mixed_groups_h{h}"] >= 1, w
            assert c["nan_from_first"] >= 1 and c["nan_from_middle"] >= 1, w
            assert c["nan_from_arithmetic"] >= 1, w
            assert c["order_sensitive"] >= 16, w
            if t in O.CPLX and op == "prod":
                assert c["recovered_clean"] >= 4 and c["recovered_nan"] >= 4, w
        if op in ("max", "min"):
            assert c["fourth_elements_tied"], w
            if t not in O.INT_TYPES:
                assert min(c["nan_first"], c["nan_middle"], c["nan_last"]) >= 1, w
            if t in X.FLOATING:
                assert c["zeros_plus_first"] >= 1 and c["zeros_minus_first"] >= 1, w
                assert c["all_minus_inf"] >= 1 and c["all_plus_inf"] >= 1, w
        if t in O.INT_TYPES:
            assert c["has_min"] and c["has_max"], w
            if op == "prod":
                assert c["wraps"] >= 1 and c["small"] >= 1, w
        if t == "longdouble":
            assert c["x87_only_rows"] == 4, w


@pytest.mark.parametrize("t,op", ARITH, ids=lambda x: x)
def test_short_inputs_open_with_an_ordinary_and_a_nan_vector(t, op):
    """n_small and every other prefix: vector 0 is ordinary, vector 1 has a
    NaN, so a call of W + 1 elements takes the fast route in one vector and
    the exact one in the next."""
    W = X.width(t)
    for P in (2, 3, 8):
        src = X.matrix_inputs(t, op, P, 2 * W, 0x3A7 + P)
        nan = np.logical_or.reduce([X.has_nan(t, s) for s in src])
        assert not nan[:W].any() and nan[W:].any(), (t, op, P)
        # a prefix of a longer input is the shorter input: the GPU tests slice
        long = X.matrix_inputs(t, op, P, 40 * W + 3, 0x3A7 + P)
        for a, b in zip(src, long):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b[:2 * W]).view(np.uint8))


def test_location_inputs_discriminate():
    """The location door reuses loc_cases.tie_values / tie_indices, whose own
    condition (an index neither the first nor the last holder's, a NaN in a
    middle member) holds at the matrix's lengths."""
    from support import loc_cases as L
    for t, op in X.door_pairs("loc"):
        n = X.n_collective("loc", t)
        L.tie_case(t, op, 3, n, 0x10C + X.esize(t))


def test_door_cases_lay_out_disjoint_areas():
    for door in X.DOORS:
        for t in ("short", "complexd", "longdouble", "half"):
            if t not in X.door_types(door):
                continue
            op = "max" if door == "loc" else "sum"
            n = X.n_collective(door, t)
            lens = [X.n_small(t), 0, n] if door == "many" else None
            c = X.DoorCase(door, t, op, n, 5, lens=lens)
            assert c.bytes <= X.HEAP - 4096
            used = np.zeros(c.bytes, int)
            for off, arr in c.writes[1]:
                used[off:off + np.ascontiguousarray(arr).nbytes] += 1
            used += c.target_mask()
            assert used.max() == 1, (door, t)
            assert c.team_path() in ("team", "pull")
            assert set(c.wants) == {1, 2, 3} and 0 in c.writes


# ----------------------------------------------------- 3. the fast route
@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("fast_fold", san=request.param == "san")


def test_fast_fold_premise(program):
    p = subprocess.run([program, "premise"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-3000:]


def record(t, op, srcs, want):
    out = [np.array([osgpu.type_code(t), osgpu.OPS.index(op), len(srcs), len(want)],
                    np.int32).tobytes()]
    out += [np.ascontiguousarray(s).tobytes() for s in srcs]
    out.append(np.ascontiguousarray(want).tobytes())
    return b"".join(out)


def ascending(t, op, srcs):
    from support import uniform_cases as U
    return U.value(t, op, list(srcs))


def test_the_kernels_route_gives_the_oracles_bytes(program, tmp_path):
    """Fast fold per vector, exact refold of a flagged vector -- the body of
    team_scan_lds_kernel and team_uniform_lds_kernel on the host -- over the
    matrix inputs of every floating sum / prod at 2, 3 and 8 members; each
    record takes both routes.  (On an x86 host a plain + or * follows the SSE
    NaN rule by itself, so for real types a fast fold that skipped the refold
    would give the same bytes here: the route counts are what holds it.  The
    complex products' recovery differs in bytes on the host too.)"""
    for t, op in ARITH:
        recs = []
        for P in (2, 3, 8):
            src = X.matrix_inputs(t, op, P, X.n_tile("team_scan", t, P), 0x3A7 + P)
            recs.append(record(t, op, src, ascending(t, op, src)))
        f = tmp_path / f"{t}_{op}.bin"
        f.write_bytes(b"".join(recs))
        p = subprocess.run([program, "route", str(f)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith("ok 3 records"), (t, op, p.stdout[-2000:])
        fast, exact = (int(x.split("=")[1]) for x in p.stdout.split()[3:5])
        assert fast >= 16 and exact >= 16, (t, op, p.stdout)


def test_a_wrong_expectation_is_seen(program, tmp_path):
    """The program compares: one flipped bit of the expected bytes fails."""
    src = X.matrix_inputs("double", "prod", 3, 40, 7)
    bad = bytearray(record("double", "prod", src, ascending("double", "prod", src)))
    bad[-8] ^= 1
    f = tmp_path / "bad.bin"
    f.write_bytes(bytes(bad))
    p = subprocess.run([program, "route", str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 1 and "element 39 differs" in p.stdout, p.stdout[-2000:]
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL).returncode == 1
