"""The C interface of the prefix scans without a GPU (include/osgpu_reduce.h
Part 1f): the header compiles as C with the four declarations usable, the
four symbols are exported with no shmem_ / pshmem_ twins, osgpu_has_scan
agrees with osgpu_has_op | osgpu_has_ext_op over the whole type x op grid,
and osgpu_scan_identity returns the identity table (checked against numpy in
tests/test_scan_ref.py) and refuses every other pair.
"""
import ctypes
import os
import subprocess

import numpy as np

import osgpu
from support import scan_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["osgpu_scan", "osgpu_has_scan", "osgpu_scan_identity", "osgpu_team_scan"]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_scan.c"
    src.write_text(
        '#include "osgpu_reduce.h"\n'
        'int main(void){\n'
        '  void (*a)(int,int,int,void*,const void*,int,int,int,int,void*,long*) = osgpu_scan;\n'
        '  int (*b)(int,int) = osgpu_has_scan;\n'
        '  int (*c)(int,int,void*) = osgpu_scan_identity;\n'
        '  int (*d)(int,int,int,int,void*const*,const void*const*,size_t,void*) = osgpu_team_scan;\n'
        '  return a == 0 || b == 0 || c == 0 || d == 0; }\n')
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
    assert "shmem_scan" not in out and "inscan" not in out   # an extension: no shmem_ twins
    L = osgpu.load()
    assert L.osgpu_scan.restype is None and len(L.osgpu_scan.argtypes) == 11
    assert len(L.osgpu_team_scan.argtypes) == 8
    assert callable(osgpu.scan("half", "sum", True))


def test_has_scan_grid():
    L = osgpu.load()
    on = 0
    for t in range(-2, 14):
        for o in range(-2, 10):
            want = int(L.osgpu_has_op(t, o) == 1 or L.osgpu_has_ext_op(t, o) == 1)
            assert L.osgpu_has_scan(t, o) == want, (t, o)
            on += want
    assert on == 52


def test_scan_identity_returns_the_table():
    L = osgpu.load()
    pairs = [(t, o) for t in osgpu.TYPES for o in osgpu.OPS if osgpu.has_op(t, o)]
    pairs += [(t, o) for t in osgpu.EXT_TYPES for o in osgpu.EXT_OPS]
    assert len(pairs) == 52
    for t, o in pairs:
        got = osgpu.scan_identity(t, o)
        want = np.ascontiguousarray(C.identity(t, o)).view(np.uint8)
        assert len(got) == C.esize(t) == L.osgpu_type_size(osgpu.type_code(t))
        if t == "longdouble":
            assert got[:10] == want.tobytes()[:10] and got[10:] == bytes(6), (t, o)
        else:
            assert got == want.tobytes(), (t, o)
    # every other pair, and a null output, is refused and leaves the buffer alone
    buf = ctypes.create_string_buffer(b"\x5a" * 16, 16)
    for t in range(-2, 14):
        for o in range(-2, 10):
            if L.osgpu_has_scan(t, o) != 1:
                assert L.osgpu_scan_identity(t, o, buf) == -1, (t, o)
    assert buf.raw == b"\x5a" * 16
    assert L.osgpu_scan_identity(1, 0, None) == -1
