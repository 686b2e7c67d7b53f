#!/usr/bin/env python3
"""scan_rate.py -- the owner-computes scan kernel against the kernels that move
comparable bytes, in ONE process on the SAME allocations.  Not part of the
product.

  python tools/scan_rate.py [--table profiles/scan_rate.md] [--commit ID]   (on the GPU)

double sum and float sum at P = 2, 4, 8, --elems (64 Mi) elements per source,
timed with HIP events on one stream:

  scan     osgpu_team_scan, inclusive: P reads + P writes per element, P - 1 folds;
  team     osgpu_team_combine: the same bytes, P (P - 1) folds (on the parent commit too);
  pull     osgpu_combine over P inputs: what the LAST member of a pull
           emulation runs -- P reads + 1 write per element.

Per case 3 warm-ups, then --reps timed launches of each kernel in the order
scan, team, pull and again in the order pull, team, scan (both orders: the
second pass tells a drift of the clocks from a difference between kernels).
Best and median of all 2 x reps timings; ratios on the medians.  JSON lines on
stdout; --table FILE writes the markdown table.  One GPU: every member's
arrays are in the same HBM, so nothing here says anything about xGMI."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("test-resilient-osss-ucx_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

WARM = 3


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def measure(a, torch, osgpu):
    L = osgpu.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    rows = []
    for t, dt, s in (("double", torch.float64, 8), ("float", torch.float32, 4)):
        tc = osgpu.type_code(t)
        for P in (2, 4, 8):
            n = a.elems
            srcs = [torch.randint(-3, 4, (n,), device="cuda").to(dt) for _ in range(P)]
            dsts = [torch.empty(n, dtype=dt, device="cuda") for _ in range(P)]
            sv = (ctypes.c_void_p * P)(*[x.data_ptr() for x in srcs])
            dv = (ctypes.c_void_p * P)(*[x.data_ptr() for x in dsts])
            kernels = {
                "scan": lambda: L.osgpu_team_scan(tc, 0, 0, P, dv, sv, n, sp),
                "team": lambda: L.osgpu_team_combine(tc, 0, P, dv, sv, n, sp),
                "pull": lambda: L.osgpu_combine(tc, 0, dsts[P - 1].data_ptr(), sv, P, n, sp),
            }

            def timed(fn):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(a.reps)]
                torch.cuda.synchronize()
                for e0, e1 in ev:
                    e0.record(st)
                    assert fn() == 0, L.osgpu_last_error()
                    e1.record(st)
                    torch.cuda.synchronize()
                return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]

            for k in kernels.values():
                for _ in range(WARM):
                    assert k() == 0, L.osgpu_last_error()
            torch.cuda.synchronize()
            ts = {k: [] for k in kernels}
            for order in (("scan", "team", "pull"), ("pull", "team", "scan")):
                for k in order:
                    ts[k] += timed(kernels[k])
            # the scan's last target is the full fold: small integers, any order the same
            assert L.osgpu_team_scan(tc, 0, 0, P, dv, sv, n, sp) == 0
            torch.cuda.synchronize()
            ok = bool(torch.equal(dsts[P - 1], torch.stack(srcs).sum(0)))
            row = {"type": t, "P": P, "elems": n, "reps": 2 * a.reps, "last_is_sum": ok}
            for k in kernels:
                row[k + "_best_us"], row[k + "_median_us"] = min(ts[k]), median(ts[k])
            row["scan_GBps"] = 2 * P * n * s / row["scan_median_us"] / 1e3
            row["team_over_scan"] = row["team_median_us"] / row["scan_median_us"]
            row["pull_over_scan"] = row["pull_median_us"] / row["scan_median_us"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            del srcs, dsts
    return rows


def table(a, torch, rows):
    with open(a.table, "w") as f:
        f.write("# Prefix scan: the owner-computes kernel against the team combine and the pull\n\n"
                f"tools/scan_rate.py, {torch.cuda.get_device_name(0)}, commit {a.commit}, one process, "
                f"the same allocations, sum, {rows[0]['elems']} elements per source, {WARM} warm-ups, "
                f"then {a.reps} timed launches of each kernel in the order scan, team, pull and "
                f"{a.reps} more in the reverse order; HIP events, times in us (best / median of all "
                "timings).  scan: osgpu_team_scan, inclusive (P reads + P writes per element); team: "
                "osgpu_team_combine (the same bytes); pull: osgpu_combine over P inputs, the last "
                "member of a pull emulation (P reads + 1 write).  x: that kernel's median over the "
                "scan's (above 1: the scan is faster).  GB/s: the scan's 2 P n size bytes over its "
                "median.\n\n"
                "| type | P | scan best | scan median | GB/s | team best | team median | team x | "
                "pull best | pull median | pull x | last target is the sum |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['type']} | {r['P']} | {r['scan_best_us']:.1f} | {r['scan_median_us']:.1f} | "
                    f"{r['scan_GBps']:.0f} | {r['team_best_us']:.1f} | {r['team_median_us']:.1f} | "
                    f"{r['team_over_scan']:.3f} | {r['pull_best_us']:.1f} | {r['pull_median_us']:.1f} | "
                    f"{r['pull_over_scan']:.3f} | {'yes' if r['last_is_sum'] else 'NO'} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--elems", type=int, default=64 << 20)
    ap.add_argument("--table", default=None)
    ap.add_argument("--commit", default="(not given)")
    a = ap.parse_args()
    import torch
    import osgpu
    assert torch.cuda.is_available(), "scan_rate.py measures on the GPU"
    rows = measure(a, torch, osgpu)
    if a.table:
        table(a, torch, rows)


if __name__ == "__main__":
    main()
