#!/usr/bin/env python3
"""loc_rate.py -- the value + index kernel (osgpu_team_loc) against the uniform
reduce's kernel, in ONE process on the SAME allocations.  Not part of the
product.

  python tools/loc_rate.py [--table profiles/loc_rate.md] [--commit ID]   (on the GPU)

short, float and double max at P = 2, 4, 8 members, --elems (64 Mi) elements
per source, timed with HIP events on one stream:

  uniform  osgpu_team_uniform, the yardstick: 2 P s bytes per element;
  loc      osgpu_team_loc with index sources, ndst = P: 2 P (s + 4) bytes;
  null     osgpu_team_loc without index sources (member numbers by value),
           ndst = P: P (2 s + 4) bytes;
  shards   the loc case launched as the collective launches it: P launches
           over the sub-ranges osgpu_shard_range cuts with element size
           min(s, 4), back to back on the stream.

Per case 3 warm-ups of each, then --rounds (7) interleaved rounds: uniform,
loc, null, shards, shards, null, loc, uniform, each timing --batch (3)
launches between two events.  Per kernel the median and the minimum of its
2 x rounds timings, and the fraction of 8 TB/s of ITS OWN algorithmic bytes
over the median.  The noise floor of a case is the spread of the yardstick's
own repeated timings in that run, (max - min) / median: a kernel's rate per
byte counts as above or below the yardstick's only when the ratio of the two
fractions leaves 1 by more than that.  JSON lines on stdout; --table FILE
writes the markdown table.  One GPU: every member's arrays are in the same
HBM, so nothing here says anything about xGMI."""
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
CASES = (("short", "max", 2), ("float", "max", 4), ("double", "max", 8))
ORDER = ("uniform", "loc", "null", "shards", "shards", "null", "loc", "uniform")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def measure(a, torch, osgpu):
    L = osgpu.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    rows = []
    for t, op, s in CASES:
        tc, oc = osgpu.type_code(t), osgpu.OPS.index(op)
        n = a.elems
        for P in (2, 4, 8):
            if t == "short":
                vs = [torch.randint(-30000, 30000, (n,), device="cuda", dtype=torch.int16)
                      for _ in range(P)]
            else:
                dt = torch.float64 if t == "double" else torch.float32
                vs = [torch.randn(n, device="cuda", dtype=dt) for _ in range(P)]
            ls = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), device="cuda", dtype=torch.int32)
                  for _ in range(P)]
            vd = [torch.empty(n * s, dtype=torch.uint8, device="cuda") for _ in range(P)]
            ld = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(P)]
            arr = lambda xs, off=0, w=1: (ctypes.c_void_p * P)(*[x.data_ptr() + off * w for x in xs])
            vsv, lsv, vdv, ldv = arr(vs), arr(ls), arr(vd), arr(ld)
            members = (ctypes.c_int * P)(*range(P))
            cuts = [osgpu.shard_range(n, P, g, min(s, 4)) for g in range(P)]
            assert cuts[0][0] == 0 and cuts[-1][1] == n
            shard_args = [(arr(vd, lo, s), arr(ld, lo, 4), arr(vs, lo, s), arr(ls, lo, 4), hi - lo)
                          for lo, hi in cuts if hi > lo]

            def shards():
                rc = 0
                for d, i, v, l, m in shard_args:
                    rc |= L.osgpu_team_loc(tc, oc, P, P, d, i, v, l, None, m, sp)
                return rc

            kernels = {
                "uniform": lambda: L.osgpu_team_uniform(tc, oc, P, vdv, vsv, n, sp),
                "loc": lambda: L.osgpu_team_loc(tc, oc, P, P, vdv, ldv, vsv, lsv, None, n, sp),
                "null": lambda: L.osgpu_team_loc(tc, oc, P, P, vdv, ldv, vsv, None, members, n, sp),
                "shards": shards,
            }
            bytes_per_elem = {"uniform": 2 * P * s, "loc": 2 * P * (s + 4), "null": P * (2 * s + 4),
                              "shards": 2 * P * (s + 4)}

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
            # the value targets of the loc kernel are the yardstick's bytes, whole and in shards
            assert kernels["uniform"]() == 0
            torch.cuda.synchronize()
            first = vd[0].clone()
            same = True
            for k in ("loc", "shards"):
                assert kernels[k]() == 0
                torch.cuda.synchronize()
                same = same and all(bool(torch.equal(d, first)) for d in vd)
            row = {"type": t, "op": op, "P": P, "elems": n, "timings": 2 * a.rounds,
                   "batch": a.batch, "values_are_the_uniform_kernels": same}
            row["noise"] = (max(ts["uniform"]) - min(ts["uniform"])) / median(ts["uniform"])
            for k in kernels:
                row[k + "_min_us"], row[k + "_median_us"] = min(ts[k]), median(ts[k])
                row[k + "_of_peak"] = bytes_per_elem[k] * n / (row[k + "_median_us"] * 1e-6) / HBM_PEAK
            for k in ("loc", "null", "shards"):
                r = row[k + "_of_peak"] / row["uniform_of_peak"]
                row[k + "_per_byte_x"] = r
                row[k + "_verdict"] = ("above" if r > 1 + row["noise"] else
                                       "below" if r < 1 - row["noise"] else "parity")
            print(json.dumps(row), flush=True)
            rows.append(row)
            del vs, ls, vd, ld, first
            torch.cuda.empty_cache()
    return rows


def table(a, torch, rows):
    with open(a.table, "w") as f:
        f.write("# Max / min with location: the value + index kernel against the uniform kernel\n\n"
                f"tools/loc_rate.py, {torch.cuda.get_device_name(0)}, commit {a.commit}, one process, "
                f"the same allocations, {a.elems} elements per source, {WARM} warm-ups of each "
                f"kernel, then {a.rounds} interleaved rounds ({', '.join(ORDER)}), each timing "
                f"{a.batch} launches between two HIP events; times in us per launch (min / median "
                f"of a kernel's {2 * a.rounds} timings).  uniform: osgpu_team_uniform, the yardstick "
                "(2 P s bytes per element); loc: osgpu_team_loc with index sources, ndst = P "
                "(2 P (s + 4) bytes); null: without index sources (P (2 s + 4) bytes); shards: "
                "loc as P launches over the collective's shard ranges (osgpu_shard_range with "
                "element size min(s, 4)).  of 8 TB/s: the kernel's own algorithmic bytes over its "
                "median.  noise: (max - min) / median of the yardstick's own timings in this run.  "
                "x: the kernel's fraction of 8 TB/s over the yardstick's (above 1: more bytes per "
                "second than the yardstick); parity unless x leaves 1 by more than the noise.  "
                "same: the value targets of loc and shards hold the yardstick's bytes.  One GPU: "
                "nothing here says anything about xGMI.\n\n"
                "| type op | P | kernel | min | median | of 8 TB/s | x | verdict | noise | same |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            for k in ("uniform", "loc", "null", "shards"):
                x = "" if k == "uniform" else f"{r[k + '_per_byte_x']:.3f}"
                v = "yardstick" if k == "uniform" else r[k + "_verdict"]
                f.write(f"| {r['type']} {r['op']} | {r['P']} | {k} | {r[k + '_min_us']:.1f} | "
                        f"{r[k + '_median_us']:.1f} | {r[k + '_of_peak']:.3f} | {x} | {v} | "
                        f"{r['noise']:.3f} | "
                        f"{'yes' if r['values_are_the_uniform_kernels'] else 'NO'} |\n")


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
    assert torch.cuda.is_available(), "loc_rate.py measures on the GPU"
    rows = measure(a, torch, osgpu)
    if a.table:
        table(a, torch, rows)


if __name__ == "__main__":
    main()
