#!/usr/bin/env python3
"""uniform_rate.py -- the owner-computes uniform kernel against the team
combine, in ONE process on the SAME allocations.  Not part of the product.

  python tools/uniform_rate.py [--table profiles/uniform_rate.md] [--commit ID]   (on the GPU)

P = 2, 4, 8 for double sum, float sum, int sum, complexf prod, float max
(--elems, 64 Mi, elements per source) and longdouble sum on random
significands with random signs and exponents 2^-3..2^3 (--ld-elems, 16 Mi),
timed with HIP events on one stream:

  uniform  osgpu_team_uniform: P reads + P writes per element, P - 1 folds;
  team     osgpu_team_combine: the same 2 P s bytes per element, P (P - 1)
           folds for the ordered (floating-point) ops -- the parent commit's
           kernel.

Per case 3 warm-ups of each, then --rounds (7) interleaved rounds: team,
uniform, uniform, team, each timing --batch (3) launches between two events.
Per kernel the median and the minimum of its 2 x rounds timings.  The noise
floor of a case is the spread of the team kernel's own repeated timings in
that run, (max - min) / median: the uniform kernel counts as faster or slower
only when the ratio of the medians leaves 1 by more than that.  JSON lines on
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
HBM_PEAK = 8.0e12   # bytes / s
CASES = (("double", "sum", 8), ("float", "sum", 4), ("int", "sum", 4), ("complexf", "prod", 8),
         ("float", "max", 4), ("longdouble", "sum", 16))


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def sources(torch, t, P, n):
    """P device arrays of n elements of type t as byte tensors."""
    out = []
    for _ in range(P):
        if t in ("double", "float"):
            dt = torch.float64 if t == "double" else torch.float32
            x = torch.randn(n, device="cuda", dtype=dt)
        elif t == "int":
            x = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int32)
        elif t == "complexf":      # moduli round 1: a product of 8 stays finite
            x = torch.randn(n, 2, device="cuda", dtype=torch.float32) * 0.7
        else:                      # long double: significand (J set), sign | exponent, padding 0
            x = torch.zeros(n, 2, device="cuda", dtype=torch.int64)
            x[:, 0] = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), device="cuda") | (-2 ** 63)
            x[:, 1] = (0x3fff - 3 + torch.randint(0, 7, (n,), device="cuda")) | \
                      (torch.randint(0, 2, (n,), device="cuda") << 15)
        out.append(x.view(torch.uint8).reshape(-1))
    return out


def measure(a, torch, osgpu):
    L = osgpu.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    rows = []
    for t, op, s in CASES:
        tc, oc = osgpu.type_code(t), osgpu.OPS.index(op)
        n = a.ld_elems if t == "longdouble" else a.elems
        for P in (2, 4, 8):
            srcs = sources(torch, t, P, n)
            dsts = [torch.empty(n * s, dtype=torch.uint8, device="cuda") for _ in range(P)]
            sv = (ctypes.c_void_p * P)(*[x.data_ptr() for x in srcs])
            dv = (ctypes.c_void_p * P)(*[x.data_ptr() for x in dsts])
            kernels = {
                "uniform": lambda: L.osgpu_team_uniform(tc, oc, P, dv, sv, n, sp),
                "team": lambda: L.osgpu_team_combine(tc, oc, P, dv, sv, n, sp),
            }

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
            # the team kernel's member 0 folds ascending: the uniform value
            first = dsts[0].clone()
            ts = {k: [] for k in kernels}
            for _ in range(a.rounds):
                for k in ("team", "uniform", "uniform", "team"):
                    ts[k].append(timed(kernels[k]))
            assert kernels["uniform"]() == 0
            torch.cuda.synchronize()
            ok = all(bool(torch.equal(d, first)) for d in dsts)
            row = {"type": t, "op": op, "P": P, "elems": n, "timings": 2 * a.rounds,
                   "batch": a.batch, "all_targets_are_member_0s_fold": ok}
            if not ok:   # the elements that differ, with their inputs, as hex
                q = next(i for i, d in enumerate(dsts) if not torch.equal(d, first))
                bad = (dsts[q].view(n, s) != first.view(n, s)).any(1).nonzero().reshape(-1)
                row["differ"] = {"target": q, "count": int(bad.numel()), "elements": [
                    {"index": int(i), "team_member_0": bytes(first.view(n, s)[i].tolist()).hex(),
                     "uniform": bytes(dsts[q].view(n, s)[i].tolist()).hex(),
                     "inputs": [bytes(x.view(n, s)[i].tolist()).hex() for x in srcs]}
                    for i in bad[:4]]}
            for k in kernels:
                row[k + "_min_us"], row[k + "_median_us"] = min(ts[k]), median(ts[k])
            row["noise"] = (max(ts["team"]) - min(ts["team"])) / row["team_median_us"]
            row["team_over_uniform"] = row["team_median_us"] / row["uniform_median_us"]
            r = row["team_over_uniform"]
            row["verdict"] = ("faster" if r > 1 + row["noise"] else
                              "slower" if r < 1 - row["noise"] else "parity")
            row["uniform_of_peak"] = 2 * P * n * s / (row["uniform_median_us"] * 1e-6) / HBM_PEAK
            row["team_of_peak"] = 2 * P * n * s / (row["team_median_us"] * 1e-6) / HBM_PEAK
            print(json.dumps(row), flush=True)
            rows.append(row)
            del srcs, dsts, first
            torch.cuda.empty_cache()
    return rows


def table(a, torch, rows):
    with open(a.table, "w") as f:
        f.write("# Uniform reduce-to-all: the owner-computes kernel against the team combine\n\n"
                f"tools/uniform_rate.py, {torch.cuda.get_device_name(0)}, commit {a.commit}, one "
                f"process, the same allocations, {a.elems} elements per source (long double "
                f"{a.ld_elems}), {WARM} warm-ups of each kernel, then {a.rounds} interleaved rounds "
                f"(team, uniform, uniform, team), each timing {a.batch} launches between two HIP "
                "events; times in us per launch (min / median of a kernel's "
                f"{2 * a.rounds} timings).  uniform: osgpu_team_uniform (P reads + P writes per "
                "element, P - 1 folds); team: osgpu_team_combine (the same bytes, P (P - 1) folds "
                "for floating-point ops).  of 8 TB/s: 2 P n size bytes over the median.  noise: "
                "(max - min) / median of the team kernel's own timings in this run.  x: the team's "
                "median over the uniform's (above 1: uniform is faster); the verdict is parity "
                "unless x leaves 1 by more than the noise.  same: every target of the uniform "
                "kernel holds the bytes of the team kernel's member 0.\n\n"
                "| type op | P | uniform min | uniform median | of 8 TB/s | team min | team median "
                "| of 8 TB/s | noise | x | verdict | same |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['type']} {r['op']} | {r['P']} | {r['uniform_min_us']:.1f} | "
                    f"{r['uniform_median_us']:.1f} | {r['uniform_of_peak']:.3f} | "
                    f"{r['team_min_us']:.1f} | {r['team_median_us']:.1f} | {r['team_of_peak']:.3f} | "
                    f"{r['noise']:.3f} | {r['team_over_uniform']:.3f} | {r['verdict']} | "
                    f"{'yes' if r['all_targets_are_member_0s_fold'] else 'NO'} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--elems", type=int, default=64 << 20)
    ap.add_argument("--ld-elems", type=int, default=16 << 20)
    ap.add_argument("--table", default=None)
    ap.add_argument("--commit", default="(not given)")
    a = ap.parse_args()
    import torch
    import osgpu
    assert torch.cuda.is_available(), "uniform_rate.py measures on the GPU"
    rows = measure(a, torch, osgpu)
    if a.table:
        table(a, torch, rows)


if __name__ == "__main__":
    main()
