#!/usr/bin/env python3
"""half_rate.py -- rate of the half / bfloat16 combine and team kernels
against `short` sum at the same shapes (identical bytes, an integer fold),
in ONE process on the SAME allocations.

Cases: osgpu_combine sum with K = 2 and K = 8 inputs, osgpu_team_combine sum
with P = 2 and P = 8 members (one GPU: the members share its HBM, not xGMI),
--mi Mi elements each (default 64).  HIP events around each launch, median of
--reps (>= 20) after 3 warm-up launches.  `short` is measured before and
after the two types of every case, so its own spread is beside every ratio.

JSON lines on stdout; --table FILE writes the markdown table (profiles/).
Not part of the product."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-resilient-osss-ucx_amd"))
import torch  # noqa: E402
import osgpu  # noqa: E402

CASES = [("combine", 2), ("combine", 8), ("team", 2), ("team", 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mi", type=int, default=64, help="Mi elements per array")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    assert a.reps >= 20 or a.mi < 8, "at least 20 timed launches"
    assert torch.cuda.is_available(), "half_rate.py measures on the GPU"
    osgpu.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    n = a.mi << 20
    # 8 sources and 8 targets of n 2-byte elements: 1.0 as binary16 (a finite
    # bfloat16 and short too), so no fold leaves the streaming path
    src = [torch.full((n,), 0x3C00, dtype=torch.int16, device="cuda") for _ in range(8)]
    dst = [torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(8)]
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
    for kind, k in CASES:
        sp_ = [s.data_ptr() for s in src[:k]]
        dp_ = [d.data_ptr() for d in dst[:k]]

        def run(t):
            if kind == "combine":
                return lambda: osgpu.combine(t, "sum", dp_[0], sp_, n, sp)
            return lambda: osgpu.team_combine(t, "sum", dp_, sp_, n, sp)

        nbytes = 2 * n * (k + 1 if kind == "combine" else 2 * k)
        s0 = timed(run("short"))
        h = timed(run("half"))
        b = timed(run("bfloat16"))
        s1 = timed(run("short"))
        sm = 0.5 * (s0 + s1)
        row = {"kernel": kind, "inputs": k, "elements": n, "bytes": nbytes,
               "short_us": [s0 * 1e6, s1 * 1e6], "half_us": h * 1e6, "bfloat16_us": b * 1e6,
               "short_spread": abs(s0 - s1) / sm, "half_over_short": h / sm,
               "bfloat16_over_short": b / sm, "short_GBps": nbytes / sm / 1e9,
               "half_GBps": nbytes / h / 1e9, "bfloat16_GBps": nbytes / b / 1e9}
        rows.append(row)
        print(json.dumps(row), flush=True)

    if a.table:
        with open(a.table, "w") as f:
            f.write("# half / bfloat16 sum against short sum\n\n"
                    f"tools/half_rate.py, {torch.cuda.get_device_name(0)}, one process, {a.mi} Mi "
                    f"elements per array, HIP events, median of {a.reps} after 3 warm-up launches.  "
                    "Times in us per launch.  `short` runs on the same allocations before and "
                    "after the two types of each case: both times are given, `spread` is their "
                    "difference over their mean, and the ratios are over that mean.  The team "
                    "cases run on one GPU (shared HBM, not xGMI).\n\n")
            f.write("| kernel | inputs | short before | short after | spread | half | bfloat16 | "
                    "half / short | bfloat16 / short | short GB/s |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['kernel']} | {r['inputs']} | {r['short_us'][0]:.1f} | "
                        f"{r['short_us'][1]:.1f} | {100 * r['short_spread']:.1f} % | "
                        f"{r['half_us']:.1f} | {r['bfloat16_us']:.1f} | {r['half_over_short']:.3f} | "
                        f"{r['bfloat16_over_short']:.3f} | {r['short_GBps']:.0f} |\n")


if __name__ == "__main__":
    main()
