"""The C interface of the uniform reduce-to-all without a GPU
(include/osgpu_reduce.h Part 1g): the header compiles as C with the three
declarations usable, the three symbols are exported with no shmem_ / pshmem_
twins, and osgpu_has_reduce_uniform agrees with osgpu_has_op |
osgpu_has_ext_op over the whole type x op grid (52 pairs).
"""
import os
import subprocess

import osgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["osgpu_reduce_uniform", "osgpu_has_reduce_uniform", "osgpu_team_uniform"]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_uniform.c"
    src.write_text(
        '#include "osgpu_reduce.h"\n'
        'int main(void){\n'
        '  void (*a)(int,int,void*,const void*,int,int,int,int,void*,long*) = osgpu_reduce_uniform;\n'
        '  int (*b)(int,int) = osgpu_has_reduce_uniform;\n'
        '  int (*c)(int,int,int,void*const*,const void*const*,size_t,void*) = osgpu_team_uniform;\n'
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
    # an extension: no shmem_ twins
    assert not [s for s in kinds if "uniform" in s and s.startswith(("shmem_", "pshmem_"))]
    assert "shmem_reduce_uniform" not in out
    L = osgpu.load()
    assert L.osgpu_reduce_uniform.restype is None and len(L.osgpu_reduce_uniform.argtypes) == 10
    assert len(L.osgpu_team_uniform.argtypes) == 7
    assert callable(osgpu.reduce_uniform("half", "sum"))
    assert callable(osgpu.team_uniform)


def test_has_reduce_uniform_grid():
    L = osgpu.load()
    on = 0
    for t in range(-2, 14):
        for o in range(-2, 10):
            want = int(L.osgpu_has_op(t, o) == 1 or L.osgpu_has_ext_op(t, o) == 1)
            assert L.osgpu_has_reduce_uniform(t, o) == want, (t, o)
            on += want
    assert on == 52
