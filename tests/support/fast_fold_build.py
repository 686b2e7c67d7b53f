"""fast_fold_build.py -- TEST INFRASTRUCTURE: build tests/support/fast_fold_check
(the branch-free folds of csrc/elem_ops.hpp, Fast<T, OP>, against the exact
Elem<T, OP> on the host, with their own main) with g++ against the HIP headers,
plain and with ASan + UBSan, the way loc_host_build.py builds loc_host_check."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "test-resilient-osss-ucx_amd", "csrc")
SRCS = [os.path.join(HERE, "fast_fold_check.cpp")]
HDRS = [os.path.join(CSRC, "elem_ops.hpp")]
PATH = os.path.join(HERE, "fast_fold_check")
SAN_PATH = os.path.join(HERE, "fast_fold_check_san")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
# the runtimes linked in: a program with the shared ASan runtime refuses to
# start in an environment that preloads any other library
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
             "-static-libasan", "-static-libubsan"]


def build(san: bool = False) -> str:
    """The program's path, compiled if missing or older than its sources."""
    out = SAN_PATH if san else PATH
    if (not os.path.exists(out)
            or os.path.getmtime(out) < max(os.path.getmtime(f) for f in SRCS + HDRS)):
        # elem_ops.hpp includes the HIP runtime header for its __host__ __device__ marks only
        cmd = (["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                "-I", os.path.join(ROCM, "include")] + (SAN_FLAGS if san else [])
               + SRCS + ["-o", out])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stdout[-4000:]}")
    return out
