"""host_check_build.py -- TEST INFRASTRUCTURE: build the host checks
tests/support/<name>_check: HIP-free code of csrc/ compiled for the host with
its own main, by g++, plain and with ASan + UBSan (<name>_check_san).

  rscatter_host  the block arithmetic of osgpu_reduce_scatter and the chunk and
                 host-fold helpers it shares
  many_host      the routes, packing plan, overlap check and host-fold loop of
                 the batched reduce-to-all
  scan_host      the prefix lengths, byte counts, chunk walk and identity table
                 of osgpu_scan
  loc_host       the arithmetic of osgpu_reduce_loc and its step (elem_ops.hpp
                 LocStep), against the HIP headers
  fast_fold      the branch-free folds Fast<T, OP> against the exact Elem<T, OP>,
                 against the HIP headers
  heap_host      the job setup: the pSync board, the descriptor channel, the
                 chunk layout and the preflight report
"""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "test-resilient-osss-ucx_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
# elem_ops.hpp includes the HIP runtime header for its __host__ __device__ marks only
HIP_HEADERS = ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include")]
# the runtimes linked in: a program with the shared ASan runtime refuses to
# start in an environment that preloads any other library
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
             "-static-libasan", "-static-libubsan"]

# name -> (further sources in csrc/, headers of csrc/ watched, extra flags)
CHECKS = {
    "rscatter_host": ([], ["rscatter_host.hpp", "scan_host.hpp", "many_host.hpp"], []),
    "many_host": ([], ["many_host.hpp"], []),
    "scan_host": ([], ["scan_host.hpp"], []),
    "loc_host": ([], ["loc_host.hpp", "scan_host.hpp", "elem_ops.hpp"], HIP_HEADERS),
    "fast_fold": ([], ["elem_ops.hpp"], HIP_HEADERS),
    "heap_host": (["fd_channel.cpp"],
                  ["coll.hpp", "psync_board.hpp", "fd_channel.hpp", "heap_host.hpp"], ["-pthread"]),
}


def build(name: str, san: bool = False) -> str:
    """The program's path, compiled if missing or older than its sources."""
    more, hdrs, flags = CHECKS[name]
    srcs = [os.path.join(HERE, name + "_check.cpp")] + [os.path.join(CSRC, f) for f in more]
    out = os.path.join(HERE, name + ("_check_san" if san else "_check"))
    watched = srcs + [os.path.join(CSRC, h) for h in hdrs]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in watched):
        cmd = (["g++", "-O1", "-std=c++17", "-Wall"] + flags + (SAN_FLAGS if san else [])
               + srcs + ["-o", out])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stdout[-4000:]}")
    return out
