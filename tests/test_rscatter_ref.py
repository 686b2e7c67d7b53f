"""osgpu_reduce_scatter without a GPU: what the library answers before any
memory is looked at, and the expected-value helper the GPU tests use.

* osgpu_has_reduce_scatter over the whole type x op grid (and beyond it): 1
  exactly where osgpu_has_op or osgpu_has_ext_op is -- 44 + 8 pairs;
* the three symbols are declared in the header, exported and bound;
* nreduce == 0 only synchronises: two barriers, pSync left at 0, on a
  contiguous and on a strided active set (logPE_stride = 1), PE_size == 1 too;
* a (type, op) pair that does not exist is fatal, with a message;
* tests/support/rscatter_cases.expected is the slice of the reduce-to-all
  oracle it says it is (a 2-PE case written out), on strided sets as well.

A host-heap call that moves data looks its arguments up with the HIP runtime
(every path of this library runs on the GPU or refuses: there is no CPU
implementation), so the host fold, GETMEM, PE_size == 1 and overlap cases
are GPU tests (tests/test_gpu_rscatter.py test_collective_host_heaps); their
byte arithmetic runs here under sanitizers (tests/test_rscatter_host.py).
"""
import os
import subprocess
import sys

import numpy as np

import oracle as O
import osgpu
from support import half_ref as R
from support import rscatter_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_has_reduce_scatter_grid():
    L = osgpu.load()
    on = {(t, o) for t in range(-2, 14) for o in range(-2, 10)
          if L.osgpu_has_reduce_scatter(t, o) == 1}
    want = {(osgpu.type_code(t), osgpu.OPS.index(o)) for t in osgpu.TYPES for o in osgpu.OPS
            if osgpu.has_op(t, o)}
    want |= {(osgpu.type_code(t), osgpu.OPS.index(o)) for t in osgpu.EXT_TYPES
             for o in osgpu.EXT_OPS}
    assert len(want) == 52 and on == want
    for t in range(-2, 14):
        for o in range(-2, 10):
            assert L.osgpu_has_reduce_scatter(t, o) == int(
                L.osgpu_has_op(t, o) == 1 or L.osgpu_has_ext_op(t, o) == 1)


def test_symbols_declared_exported_bound():
    names = osgpu.header_symbols()
    want = ["osgpu_reduce_scatter", "osgpu_has_reduce_scatter", "osgpu_combine_shifted"]
    assert not [n for n in want if n not in names]
    out = subprocess.run(["nm", "-D", "--defined-only", osgpu.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    kinds = {p[2]: p[1] for p in (line.split() for line in out.splitlines()) if len(p) == 3}
    for n in want:
        assert kinds.get(n) == "T", n
    assert "shmem_reduce_scatter" not in out      # an extension: no shmem_ / pshmem_ twins
    L = osgpu.load()
    assert L.osgpu_reduce_scatter.restype is None
    assert len(L.osgpu_reduce_scatter.argtypes) == 10
    assert len(L.osgpu_combine_shifted.argtypes) == 7
    assert callable(osgpu.reduce_scatter("half", "sum"))


def test_shift_routes_hook_is_refused_without_test_hooks(monkeypatch):
    """osgpu_test_shift_routes (which kernel osgpu_combine_shifted's chunks
    took) is not in the public header and answers only under
    OSGPU_TEST_HOOKS=1; it reports the shipped tile the GPU tests assume."""
    import ctypes
    assert "osgpu_test_shift_routes" not in open(osgpu.HEADER).read()
    L = osgpu.load()
    L.osgpu_test_shift_routes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong * 4),
                                          ctypes.POINTER(ctypes.c_int)]
    c, shape = (ctypes.c_ulonglong * 4)(), ctypes.c_int()
    monkeypatch.delenv("OSGPU_TEST_HOOKS", raising=False)
    assert L.osgpu_test_shift_routes(ctypes.byref(c), ctypes.byref(shape)) != 0
    monkeypatch.setenv("OSGPU_TEST_HOOKS", "1")
    assert L.osgpu_test_shift_routes(ctypes.byref(c), ctypes.byref(shape)) == 0
    assert shape.value * 64 == C.TILE_VECTORS


def test_zero_elements_only_synchronise():
    from support import team as T
    tm = T.Team(8, 4096, device=False)
    for t, op, start, log, size in (("double", "sum", 0, 0, 8), ("half", "max", 1, 1, 3),
                                    ("longdouble", "prod", 2, 0, 1), ("short", "xor", 0, 2, 2)):
        before = [tm.pet.pet_barrier_calls(pe) for pe in range(8)]
        members = C.run(tm, t, op, 1024, 0, 0, start, log, size)
        assert members == O.active_set(start, log, size)
        after = [tm.pet.pet_barrier_calls(pe) for pe in range(8)]
        assert [a - b for a, b in zip(after, before)] == [2 if pe in members else 0
                                                          for pe in range(8)]
        assert set(tm.last_paths.values()) == {"barrier_only"}


def test_unknown_pair_is_fatal():
    """complexf max does not exist: fatal before anything moves, in a fresh
    child process as tests/test_abi.py checks the other fatal paths."""
    code = (
        "import sys; sys.path[:0]=[%r, %r, %r]\n"
        "import osgpu\n"
        "from support import team as T\n"
        "tm = T.Team(2, 4096, device=False)\n"
        "tm.pet.pet_set_me(0)\n"
        "osgpu.reduce_scatter('complexf', 'max')(tm.ptr(0, 1024), tm.ptr(0, 0), 4, 0, 0, 2,"
        " None, tm.psync_ptr(0))\n"
        "print('RETURNED')\n"
    ) % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "test-resilient-osss-ucx_amd"),
         os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "RETURNED" not in r.stdout
    assert "osgpu_reduce_scatter: type 7 op 5 is not a reduction" in r.stderr


def test_expected_is_the_to_all_slice():
    # 2 PEs, n = 2, int sum, written out: source of PE p holds 10 p + i
    src = [np.array([0, 1, 2, 3], np.int32), np.array([10, 11, 12, 13], np.int32)]
    want = C.expected("int", "sum", src, 2)
    assert want[0].tolist() == [10, 12] and want[1].tolist() == [14, 16]
    # a strided set of 3 among 8: member index, not PE number, picks the block
    n = 5
    for t, op in (("double", "sum"), ("bfloat16", "prod")):
        srcs = C.inputs(t, op, 8, 3 * n, 99)
        want = C.expected(t, op, srcs, n, 1, 1, 3)
        assert sorted(want) == [1, 3, 5]
        full = C.to_all(t, op, srcs, 1, 1, 3)
        for m, pe in enumerate((1, 3, 5)):
            assert C.same_bits(t, want[pe], full[pe][m * n:(m + 1) * n]) is None
            # float sums depend on the order: PE pe's own source comes first
            if t == "bfloat16":
                own = R.fold(t, op, [pe] + [q for q in (1, 3, 5) if q != pe], srcs)
                assert np.array_equal(want[pe], own[m * n:(m + 1) * n])
