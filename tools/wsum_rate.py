#!/usr/bin/env python3
"""wsum_rate.py -- the widening kernel (osgpu_team_wsum) against the uniform
reduce's kernel, in ONE process on the SAME allocations.  Not part of the
product.

  python tools/wsum_rate.py [--table profiles/wsum_rate.md] [--commit ID]   (on the GPU)

P = 2, 4, 8 members, ndst = P, --elems (64 Mi) elements per source, timed with
HIP events on one stream:

  short_a, short_b   osgpu_team_uniform for short sum, at the start and at the
                     end of every round: the spread between the two is the
                     yardstick's own;
  half_u, bf16_u     osgpu_team_uniform for half sum and for bfloat16 sum (one
                     rounding a step): the kernels this one is an alternative to;
  half_16, bf16_16   osgpu_team_wsum with a 16-bit target: 4 P bytes per element,
                     as the three above;
  half_32, bf16_32   osgpu_team_wsum with a float target: 6 P bytes per element.

Per member count 3 warm-ups of each, then --rounds (7) interleaved rounds in the
order above and back, each timing --batch (3) launches between two events.  Per
kernel the median and the minimum of its timings, bytes per second over ITS OWN
algorithmic bytes (median), and the ratio of its median to short's and to the
same type's uniform sum.  spread: |median(short_a) - median(short_b)| /
median(short).  JSON lines on stdout; --table FILE writes the markdown table.
One GPU: every member's arrays are in the same HBM, so nothing here says
anything about xGMI."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("test-resilient-osss-ucx_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

WARM = 3
HBM_PEAK = 8.0e12   # bytes / s
KERNELS = ("short_a", "half_u", "bf16_u", "half_16", "bf16_16", "half_32", "bf16_32", "short_b")
ORDER = KERNELS + KERNELS[::-1]


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def measure(a, torch, osgpu):
    L = osgpu.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    n = a.elems
    rows = []
    tc = {t: osgpu.type_code(t) for t in ("short", "half", "bfloat16", "float")}
    for P in (2, 4, 8):
        # small values: the sums stay finite in every format
        srcs = {"short": [torch.randint(-3000, 3000, (n,), device="cuda", dtype=torch.int16)
                          for _ in range(P)],
                "half": [torch.randn(n, device="cuda", dtype=torch.float16) for _ in range(P)],
                "bfloat16": [torch.randn(n, device="cuda", dtype=torch.bfloat16) for _ in range(P)]}
        dst = [torch.empty(n * 4, dtype=torch.uint8, device="cuda") for _ in range(P)]
        arr = lambda xs: (ctypes.c_void_p * P)(*[x.data_ptr() for x in xs])
        dv = arr(dst)
        sv = {t: arr(v) for t, v in srcs.items()}
        uni = lambda t: (lambda: L.osgpu_team_uniform(tc[t], 0, P, dv, sv[t], n, sp))
        ws = lambda t, o: (lambda: L.osgpu_team_wsum(tc[t], tc[o], P, P, dv, sv[t], None, n, sp))
        kernels = {"short_a": uni("short"), "short_b": uni("short"), "half_u": uni("half"),
                   "bf16_u": uni("bfloat16"), "half_16": ws("half", "half"),
                   "bf16_16": ws("bfloat16", "bfloat16"), "half_32": ws("half", "float"),
                   "bf16_32": ws("bfloat16", "float")}
        bytes_per_elem = {k: (6 * P if k.endswith("_32") else 4 * P) for k in kernels}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            for _ in range(a.batch):
                assert fn() == 0, L.osgpu_last_error()
            e1.record(st)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.batch

        torch.cuda.synchronize()   # the sources are written on torch's stream, not on st
        for k in kernels.values():
            for _ in range(WARM):
                assert k() == 0, L.osgpu_last_error()
        torch.cuda.synchronize()
        ts = {k: [] for k in kernels}
        for _ in range(a.rounds):
            for k in ORDER:
                ts[k].append(timed(kernels[k]))
        # the float target is torch's float32 running sum of the same values
        # (NaN-free data: bit for bit), the 16-bit target its one rounding
        ok = True
        for t, td in (("half", torch.float16), ("bfloat16", torch.bfloat16)):
            acc = srcs[t][0].to(torch.float32)
            for x in srcs[t][1:]:
                acc = acc + x.to(torch.float32)
            assert ws(t, "float")() == 0
            torch.cuda.synchronize()
            ok = ok and all(bool(torch.equal(d.view(torch.float32), acc)) for d in dst)
            assert ws(t, t)() == 0
            torch.cuda.synchronize()
            ok = ok and all(bool(torch.equal(d[:2 * n].view(td), acc.to(td))) for d in dst)
            del acc
        row = {"P": P, "elems": n, "timings": 2 * a.rounds, "batch": a.batch,
               "matches_float32_running_sum": ok}
        short = median(ts["short_a"] + ts["short_b"])
        row["short_spread"] = abs(median(ts["short_a"]) - median(ts["short_b"])) / short
        for k in kernels:
            row[k + "_min_us"], row[k + "_median_us"] = min(ts[k]), median(ts[k])
            row[k + "_bytes_per_s"] = bytes_per_elem[k] * n / (row[k + "_median_us"] * 1e-6)
            row[k + "_x_short"] = row[k + "_median_us"] / short
        for k, base in (("half_16", "half_u"), ("half_32", "half_u"), ("bf16_16", "bf16_u"),
                        ("bf16_32", "bf16_u")):
            row[k + "_x_uniform"] = row[k + "_median_us"] / row[base + "_median_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del srcs, dst
        torch.cuda.empty_cache()
    return rows


def table(a, torch, rows):
    with open(a.table, "w") as f:
        f.write("# Float-accumulated half / bfloat16 sum: the widening kernel against the uniform kernel\n\n"
                f"tools/wsum_rate.py, {torch.cuda.get_device_name(0)}, commit {a.commit}, one process, "
                f"the same allocations, {a.elems} elements per source, ndst = P, {WARM} warm-ups of "
                f"each kernel, then {a.rounds} interleaved rounds ({', '.join(KERNELS)} and back), "
                f"each timing {a.batch} launches between two HIP events; times in us per launch "
                f"(min / median of a kernel's {2 * a.rounds} timings).  short_a / short_b: "
                "osgpu_team_uniform for short sum, first and last of every round; half_u / bf16_u: "
                "osgpu_team_uniform for half / bfloat16 sum (one rounding a step); _16: "
                "osgpu_team_wsum with a 16-bit target (4 P bytes per element, as the uniform "
                "kernels); _32: with a float target (6 P bytes).  TB/s: the kernel's own "
                "algorithmic bytes over its median.  x short: median over the median of all of "
                "short's timings.  x uniform: median over the same type's uniform sum's.  spread: "
                "|median(short_a) - median(short_b)| / median(short) in this run.  same: both "
                "targets equal torch's float32 running sum of the sources (rounded once for the "
                "16-bit target) on every member.  One GPU: nothing here says anything about xGMI.\n\n"
                "| P | kernel | min | median | TB/s | x short | x uniform | spread | same |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            for k in KERNELS:
                xu = f"{r[k + '_x_uniform']:.3f}" if k + "_x_uniform" in r else ""
                f.write(f"| {r['P']} | {k} | {r[k + '_min_us']:.1f} | {r[k + '_median_us']:.1f} | "
                        f"{r[k + '_bytes_per_s'] / 1e12:.3f} | {r[k + '_x_short']:.3f} | {xu} | "
                        f"{r['short_spread']:.3f} | "
                        f"{'yes' if r['matches_float32_running_sum'] else 'NO'} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--elems", type=int, default=64 << 20)
    ap.add_argument("--table", default=None)
    ap.add_argument("--commit", default="(not given)")
    a = ap.parse_args()
    import torch
    import osgpu
    assert torch.cuda.is_available(), "wsum_rate.py measures on the GPU"
    rows = measure(a, torch, osgpu)
    if a.table:
        table(a, torch, rows)


if __name__ == "__main__":
    main()
