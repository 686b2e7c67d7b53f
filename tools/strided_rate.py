#!/usr/bin/env python3
"""strided_rate.py -- rate of the strided copy kernel (osgpu_copy_strided,
the data movement of shmem_alltoalls32/64) against osgpu_copy of the same
useful bytes, in ONE process on the SAME allocations, and the in-process A/B
of its launch shapes: U units in flight per lane (2, 4, 8) x plain or
non-temporal accesses on the strided side (osgpu_test_strided_shape).

Cases: the three forms (gather: strided source, contiguous destination;
scatter: the mirror; both: both strided), element strides 2, 3 and 17, 4- and
8-byte elements, the useful bytes as 1 segment and split over 8.  HIP events
around each launch, median of --reps (>= 20) after 3 warm-up launches.

Two rates per case, both over the same time:
  useful    nelems * elem_bytes (the bytes alltoalls delivers; what osgpu_copy
            moves one way in the same time gives the yardstick beside it);
  touched   128-byte lines covered by the strided side(s) plus the contiguous
            side's bytes: what the memory system has to move at least.

JSON lines on stdout; --table FILE writes the markdown table (profiles/).
Not part of the product."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-resilient-osss-ucx_amd"))
os.environ["OSGPU_TEST_HOOKS"] = "1"
import torch  # noqa: E402
import osgpu  # noqa: E402

FORMS = ["gather", "scatter", "both"]
SHAPES = [(u, nt) for u in (2, 4, 8) for nt in (0, 1)]
LINE = 128


def shape_name(u, nt):
    return f"U{u}{'nt' if nt else ''}"


def touched_bytes(n, stride, esz):
    """Bytes of the 128-byte lines n elements `stride` apart cover (the base
    is line-aligned here)."""
    if stride == 1:
        return n * esz
    if stride * esz >= LINE:
        return n * LINE
    return -(-((n - 1) * stride + 1) * esz // LINE) * LINE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--useful-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--strides", type=int, nargs="+", default=[2, 3, 17])
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    assert a.reps >= 20 or a.useful_mib < 8, "at least 20 timed launches"
    assert torch.cuda.is_available(), "strided_rate.py measures on the GPU"

    L = osgpu.load()
    L.osgpu_test_strided_shape.argtypes = [ctypes.c_int] * 3
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    useful = a.useful_mib << 20
    smax = max(a.strides)
    # two buffers that hold the largest strided extent; the contiguous side
    # of a case is the head of the other one (the same allocations serve
    # osgpu_copy)
    A = torch.empty(useful * smax + 4096, dtype=torch.uint8, device="cuda")
    B = torch.empty(useful * smax + 4096, dtype=torch.uint8, device="cuda")
    A[:useful].fill_(1)
    B[:useful].fill_(2)
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(3):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.reps)]
        torch.cuda.synchronize()
        for e0, e1 in ev:
            e0.record(st)
            fn()
            e1.record(st)
        torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) * 1e-3 for e0, e1 in ev)
        return ts[len(ts) // 2]

    rows = []
    for esz in (4, 8):
        for fi, form in enumerate(FORMS):
            for stride in a.strides:
                for nseg in (1, 8):
                    n = useful // esz // nseg          # elements per segment
                    ss = stride if form != "scatter" else 1
                    ds = stride if form != "gather" else 1
                    srcs = [A.data_ptr() + i * n * ss * esz for i in range(nseg)]
                    dsts = [B.data_ptr() + i * n * ds * esz for i in range(nseg)]
                    assert n * nseg * max(ss, ds) * esz <= A.numel()

                    def strided():
                        osgpu.copy_strided(esz, dsts, [ds] * nseg, srcs, [ss] * nseg,
                                           [n] * nseg, stream=sp)

                    csrc = [A.data_ptr() + i * n * esz for i in range(nseg)]
                    cdst = [B.data_ptr() + i * n * esz for i in range(nseg)]

                    def plain():
                        osgpu.copy(cdst, csrc, [n * esz] * nseg, stream=sp)

                    row = {"form": form, "elem_bytes": esz, "stride": stride, "segments": nseg,
                           "useful_bytes": n * esz * nseg,
                           "touched_bytes": nseg * (touched_bytes(n, ss, esz)
                                                    + touched_bytes(n, ds, esz))}
                    # the yardstick first and last: its spread brackets the case
                    c0 = timed(plain)
                    for u, nt in SHAPES:
                        assert L.osgpu_test_strided_shape(fi, u, nt) == 0
                        row[shape_name(u, nt) + "_us"] = timed(strided) * 1e6
                    assert L.osgpu_test_strided_shape(fi, 0, 0) == 0
                    row["shipped_us"] = timed(strided) * 1e6
                    c1 = timed(plain)
                    row["osgpu_copy_us"] = [c0 * 1e6, c1 * 1e6]
                    t = row["shipped_us"] * 1e-6
                    row["useful_GBps"] = row["useful_bytes"] / t / 1e9
                    row["touched_GBps"] = row["touched_bytes"] / t / 1e9
                    row["osgpu_copy_GBps"] = row["useful_bytes"] / min(c0, c1) / 1e9
                    rows.append(row)
                    print(json.dumps(row), flush=True)

    # per form: the shape with the lowest geometric-mean time over its cases
    import math
    verdict = {}
    for form in FORMS:
        rs = [r for r in rows if r["form"] == form]
        gm = {shape_name(u, nt): math.exp(sum(math.log(r[shape_name(u, nt) + "_us"]) for r in rs)
                                          / len(rs)) for u, nt in SHAPES}
        best = min(gm, key=gm.get)
        verdict[form] = {"best": best, "geomean_us": gm}
    print(json.dumps({"verdict": verdict}), flush=True)

    if a.table:
        names = [shape_name(u, nt) for u, nt in SHAPES]
        with open(a.table, "w") as f:
            f.write(f"# Strided copy kernel: rates and the shape A/B\n\n"
                    f"tools/strided_rate.py, {torch.cuda.get_device_name(0)}, one process, "
                    f"{a.useful_mib} MiB useful per case, HIP events, median of {a.reps} after 3 "
                    f"warm-up launches.  Times in us per launch; `useful` and `touched` GB/s are "
                    f"the shipped shape's; `osgpu_copy` is the contiguous copy of the same "
                    f"useful bytes on the same allocations in the same run (GB/s one way; "
                    f"measured before and after the case, the faster one).\n\n")
            f.write("| form | B | stride | segs | " + " | ".join(names) +
                    " | shipped | useful GB/s | touched GB/s | osgpu_copy GB/s |\n")
            f.write("|---|---|---|---|" + "---|" * (len(names) + 4) + "\n")
            for r in rows:
                f.write(f"| {r['form']} | {r['elem_bytes']} | {r['stride']} | {r['segments']} | "
                        + " | ".join(f"{r[n + '_us']:.0f}" for n in names)
                        + f" | {r['shipped_us']:.0f} | {r['useful_GBps']:.0f} | "
                          f"{r['touched_GBps']:.0f} | {r['osgpu_copy_GBps']:.0f} |\n")
            f.write("\nGeometric-mean time per form (us), lowest first:\n\n")
            for form in FORMS:
                gm = verdict[form]["geomean_us"]
                f.write(f"- {form}: " + ", ".join(f"{k} {v:.0f}" for k, v in
                                                  sorted(gm.items(), key=lambda kv: kv[1])) + "\n")


if __name__ == "__main__":
    main()
