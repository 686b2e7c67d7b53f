"""half_build.py -- TEST INFRASTRUCTURE: build tests/support/half_check (the
half / bfloat16 element ops of csrc/elem_ops.hpp compiled for the host, with
their own main) the way libx87check.so is built, but as an executable."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "half_check.hip")
HDR = os.path.join(HERE, "..", "..", "test-resilient-osss-ucx_amd", "csrc", "elem_ops.hpp")
PATH = os.path.join(HERE, "half_check")
UBSAN_PATH = os.path.join(HERE, "half_check_ubsan")
UBSAN_FLAGS = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host",
               "-fno-sanitize-recover=undefined"]


def build(ubsan: bool = False) -> str:
    """The program's path, compiled if missing or older than its sources."""
    out = UBSAN_PATH if ubsan else PATH
    if (not os.path.exists(out)
            or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))):
        cmd = (["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950"]
               + (UBSAN_FLAGS if ubsan else []) + [SRC, "-o", out])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stdout[-4000:]}")
    return out
