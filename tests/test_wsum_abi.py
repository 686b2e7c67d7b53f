"""The C interface of the float-accumulated half / bfloat16 sum without a GPU
(include/osgpu_reduce.h Part 1i): the header compiles as C with the three
declarations usable, the symbols are exported with no shmem_ / pshmem_ twins,
osgpu_has_reduce_wsum is 1 for exactly the 4 pairs, the raw launcher refuses a
bad pair / P / ndst with OSGPU_EINVAL before it touches a GPU, and -- on PE
threads over host memory, with no GPU call -- nreduce <= 0 makes two barriers
and reports BARRIER_ONLY, and a pair outside the 4 is fatal (in a child
process).
"""
import ctypes
import os
import subprocess
import sys

import pytest

import osgpu
from support import team as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["osgpu_reduce_wsum", "osgpu_has_reduce_wsum", "osgpu_team_wsum"]
PAIRS = [("half", "half"), ("half", "float"), ("bfloat16", "bfloat16"), ("bfloat16", "float")]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_wsum.c"
    src.write_text(
        '#include "osgpu_reduce.h"\n'
        'int main(void){\n'
        '  void (*a)(int,int,void*,const void*,int,int,int,int,void*,long*) = osgpu_reduce_wsum;\n'
        '  int (*b)(int,int) = osgpu_has_reduce_wsum;\n'
        '  int (*c)(int,int,int,int,void*const*,const void*const*,const float*,size_t,void*)'
        ' = osgpu_team_wsum;\n'
        '  return a == 0 || b == 0 || c == 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(src), "-I",
                    os.path.join(ROOT, "include"), "-o", str(tmp_path / "a.o")], check=True)


def test_symbols_declared_exported_bound():
    names = osgpu.header_symbols()
    assert not [n for n in SYMBOLS if n not in names]
    out = subprocess.run(["nm", "-D", "--defined-only", osgpu.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    kinds = {p[2]: p[1] for p in (line.split() for line in out.splitlines()) if len(p) == 3}
    for n in SYMBOLS:
        assert kinds.get(n) == "T", n
    assert not [s for s in kinds if "wsum" in s and s.startswith(("shmem_", "pshmem_"))]
    L = osgpu.load()
    assert L.osgpu_reduce_wsum.restype is None and len(L.osgpu_reduce_wsum.argtypes) == 10
    assert len(L.osgpu_team_wsum.argtypes) == 9
    assert callable(osgpu.reduce_wsum("half", "float")) and callable(osgpu.team_wsum)


def test_has_reduce_wsum_grid():
    L = osgpu.load()
    on = []
    for t in range(-2, 14):
        for o in range(-2, 14):
            r = L.osgpu_has_reduce_wsum(t, o)
            assert r in (0, 1)
            if r:
                on.append((t, o))
    want = sorted((osgpu.type_code(t), osgpu.type_code(o)) for t, o in PAIRS)
    assert sorted(on) == want and len(on) == 4


def test_raw_launcher_refuses_bad_arguments():
    """Refused before any GPU call: the pointers are never read."""
    buf = (ctypes.c_byte * 256)()
    p = [ctypes.addressof(buf) + 16 * k for k in range(10)]
    bad = [("half", "bfloat16", 2, 2), ("float", "float", 2, 2), ("short", "float", 2, 2),
           ("bfloat16", "double", 2, 2), ("half", "half", 9, 9), ("half", "half", 9, 1),
           ("half", "float", 3, 2), ("bfloat16", "bfloat16", 1, 0), ("half", "half", 0, 1)]
    L = osgpu.load()
    for t, o, P, D in bad:
        rc = L.osgpu_team_wsum(osgpu.type_code(t), osgpu.type_code(o), P, D,
                               (ctypes.c_void_p * 9)(*p[:9]), (ctypes.c_void_p * 9)(*p[:9]), None,
                               4, None)
        assert rc == -1, (t, o, P, D)          # OSGPU_EINVAL
        assert b"osgpu_team_wsum" in L.osgpu_last_error()
    tc = osgpu.type_code("half")
    assert L.osgpu_team_wsum(tc, tc, 2, 2, None, (ctypes.c_void_p * 2)(*p[:2]), None, 4, None) == -1
    assert L.osgpu_team_wsum(tc, tc, 2, 2, (ctypes.c_void_p * 2)(*p[:2]), None, None, 4, None) == -1


def test_zero_length_only_synchronises():
    tm = T.Team(4, 4096, device=False)
    pwrk = (ctypes.c_byte * 64)()
    for t, o in PAIRS:
        fn = osgpu.reduce_wsum(t, o)
        for n in (0, -3):
            before = [tm.pet.pet_barrier_calls(pe) for pe in range(4)]
            tm._on_members(range(4), lambda pe: fn(tm.ptr(pe, 0), tm.ptr(pe, 2048), n, 0, 0, 4,
                                                   ctypes.addressof(pwrk), tm.psync_ptr(pe)))
            after = [tm.pet.pet_barrier_calls(pe) for pe in range(4)]
            assert [a - b for a, b in zip(after, before)] == [2, 2, 2, 2]
            assert set(tm.last_paths.values()) == {"barrier_only"}, tm.last_paths


CHILD = (
    "import sys; sys.path[:0]=[%r, %r, %r]\n"
    "from support import team as T\n"
    "import osgpu, ctypes\n"
    "tm = T.Team(2, 8192, device=False)\n"
    "%%s\n"
    "print('RETURNED')\n"
) % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "test-resilient-osss-ucx_amd"),
     os.path.join(ROOT, "oracle"))


def _child(body):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([sys.executable, "-c", CHILD % body], capture_output=True, text=True,
                          timeout=300, env=env)


@pytest.mark.parametrize("t,o", [("half", "bfloat16"), ("float", "float"), ("bfloat16", "double"),
                                 ("int", "float")])
def test_bad_pair_is_fatal(t, o):
    body = ("f = osgpu.load().osgpu_reduce_wsum\n"
            "tm.pet.pet_set_me(0)\n"
            "f(%d, %d, tm.ptr(0, 0), tm.ptr(0, 2048), 8, 0, 0, 1, None, tm.psync_ptr(0))"
            % (osgpu.type_code(t), osgpu.type_code(o)))
    r = _child(body)
    assert r.returncode != 0 and "RETURNED" not in r.stdout
    assert "osgpu_reduce_wsum" in r.stderr and "osgpu_has_reduce_wsum" in r.stderr, r.stderr[-1500:]
