"""rscatter_host_build.py -- TEST INFRASTRUCTURE: build
tests/support/rscatter_host_check (the HIP-free block arithmetic of
osgpu_reduce_scatter, csrc/rscatter_host.hpp, and the chunk and host-fold
helpers it shares, scan_host.hpp and many_host.hpp, with its own main) with
g++, plain and with ASan + UBSan, the way heap_host_build.py builds
heap_host_check."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "test-resilient-osss-ucx_amd", "csrc")
SRCS = [os.path.join(HERE, "rscatter_host_check.cpp")]
HDRS = [os.path.join(CSRC, h) for h in ("rscatter_host.hpp", "scan_host.hpp", "many_host.hpp")]
PATH = os.path.join(HERE, "rscatter_host_check")
SAN_PATH = os.path.join(HERE, "rscatter_host_check_san")
# the runtimes linked in: a program with the shared ASan runtime refuses to
# start in an environment that preloads any other library
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
             "-static-libasan", "-static-libubsan"]


def build(san: bool = False) -> str:
    """The program's path, compiled if missing or older than its sources."""
    out = SAN_PATH if san else PATH
    if (not os.path.exists(out)
            or os.path.getmtime(out) < max(os.path.getmtime(f) for f in SRCS + HDRS)):
        cmd = (["g++", "-O1", "-std=c++17", "-Wall"] + (SAN_FLAGS if san else [])
               + SRCS + ["-o", out])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stdout[-4000:]}")
    return out
