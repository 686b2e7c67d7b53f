#!/usr/bin/env python3
"""many_rate.py -- what batching buys: M reduce-to-all arrays as M calls
against ONE batched call, in ONE process on the SAME allocations.  Not part of
the product.

  python tools/many_rate.py [--table profiles/many_rate.md]     (on the GPU)

(a) Raw, timed with HIP events on one stream: M osgpu_combine launches against
    one osgpu_combine_many over the same arrays (int sum of 1 Ki elements and
    double sum of 64 Ki, M in {1, 4, 16, 64}; 4 arrays of 16 Mi doubles), at
    K = 2 and K = 8 inputs.  The events bracket the whole sequence, so the
    time holds the gaps the host leaves between M launches.  Both forms are
    driven from Python through ctypes (about a microsecond a call).
(b) The collective with threads as PEs (tests/support/team.py), P = 2, device
    heaps, host wall-clock of one step on PE 0: M shmem_<T>_sum_to_all calls
    -- the loop of single calls, whose code this feature does not touch --
    against one osgpu_reduce_many, at the same M and the two small sizes.
    Every step is a collective, so the PEs stay in step by themselves.  The
    PE threads are Python threads: the M single calls also pay M ctypes
    calls each under the interpreter lock.

Median of --reps (>= 20) after 3 warm-ups; the loop is timed twice, before and
after the batch, and the spread between its two medians is reported: a batch
figure inside that spread says nothing.  JSON lines on stdout; --table FILE
writes the markdown table."""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("test-resilient-osss-ucx_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

WARM = 3
SMALL = [("int", 1 << 10), ("double", 64 << 10)]
MS = [1, 4, 16, 64]


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def raw(a, torch, osgpu):
    L = osgpu.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    rows = []
    cases = [(t, n, M) for t, n in SMALL for M in MS] + [("double", 16 << 20, 4)]
    for t, n, M in cases:
        dt, s = (torch.int32, 4) if t == "int" else (torch.float64, 8)
        tc = osgpu.type_code(t)
        for K in (2, 8):
            srcs = [[torch.randint(-3, 4, (n,), device="cuda").to(dt) for _ in range(K)]
                    for _ in range(M)]
            outs = [torch.empty(n, dtype=dt, device="cuda") for _ in range(M)]
            refs = [torch.empty(n, dtype=dt, device="cuda") for _ in range(M)]
            rowp = [(ctypes.c_void_p * K)(*[x.data_ptr() for x in r]) for r in srcs]
            tab = (ctypes.c_void_p * M)(*[ctypes.addressof(r) for r in rowp])
            nel = (ctypes.c_size_t * M)(*([n] * M))

            def loop(dst):
                for i in range(M):
                    assert L.osgpu_combine(tc, 0, dst[i].data_ptr(), rowp[i], K, n, sp) == 0

            def batch(dst):
                tg = (ctypes.c_void_p * M)(*[x.data_ptr() for x in dst])
                assert L.osgpu_combine_many(tc, 0, M, tg, tab, K, nel, sp) == 0

            def timed(fn, dst):
                for _ in range(WARM):
                    fn(dst)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(a.reps)]
                torch.cuda.synchronize()
                for e0, e1 in ev:
                    e0.record(st)
                    fn(dst)
                    e1.record(st)
                    torch.cuda.synchronize()
                return median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)

            row = {"part": "raw", "type": t, "elems": n, "M": M, "K": K}
            row["loop_us"] = timed(loop, refs)
            row["batch_us"] = timed(batch, outs)
            row["loop_us_again"] = timed(loop, refs)
            torch.cuda.synchronize()
            row["same_bits"] = all(bool(torch.equal(x, y)) for x, y in zip(outs, refs))
            finish(row)
            rows.append(row)
            del srcs, outs, refs
    return rows


def collective(a, torch, osgpu):
    from support import many_cases as MC
    from support import team as T
    rows = []
    P = 2
    for t, n in SMALL:
        for M in MS:
            lay = MC.Layout(t, [n] * M)
            tm = T.Team(P, lay.bytes, device=True)
            dt = torch.int32 if t == "int" else torch.float64
            for pe in range(P):
                for i in range(M):
                    tm.write(pe, lay.soff[i],
                             torch.randint(-3, 4, (n,)).to(dt).numpy())
            one = osgpu.to_all(t, "sum")
            many = osgpu.reduce_many(t, "sum")
            pwrk = (ctypes.c_byte * 4096)()
            paths = {}

            def step_loop(pe):
                for to, so in zip(lay.toff, lay.soff):
                    one(tm.ptr(pe, to), tm.ptr(pe, so), n, 0, 0, P, ctypes.addressof(pwrk),
                        tm.psync_ptr(pe))

            def step_batch(pe):
                many([tm.ptr(pe, o) for o in lay.toff], [tm.ptr(pe, o) for o in lay.soff],
                     lay.lens, 0, 0, P, ctypes.addressof(pwrk), tm.psync_ptr(pe))

            def timed(step, tag):
                ts = []

                def body(pe):
                    tm.pet.pet_set_me(pe)
                    for r in range(WARM + a.reps):
                        t0 = time.perf_counter()
                        step(pe)
                        if pe == 0 and r >= WARM:
                            ts.append((time.perf_counter() - t0) * 1e6)
                    paths[tag] = osgpu.last_path()
                ths = [threading.Thread(target=body, args=(pe,)) for pe in range(P)]
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()
                return median(ts)

            row = {"part": "collective", "type": t, "elems": n, "M": M, "P": P}
            row["loop_us"] = timed(step_loop, "loop")
            image = tm.read(0, 0, lay.bytes)
            row["batch_us"] = timed(step_batch, "batch")
            row["same_bits"] = bool((tm.read(0, 0, lay.bytes) == image).all())
            row["loop_us_again"] = timed(step_loop, "loop")
            row["loop_path"], row["batch_path"] = paths["loop"], paths["batch"]
            finish(row)
            rows.append(row)
    return rows


def finish(row):
    lo, hi = sorted((row["loop_us"], row["loop_us_again"]))
    row["loop_spread"] = hi / lo - 1.0
    row["speedup"] = lo / row["batch_us"]      # against the loop's better median
    print(json.dumps(row), flush=True)


def table(a, torch, rows):
    with open(a.table, "w") as f:
        f.write("# Batched reduce-to-all: M calls against one\n\n"
                f"tools/many_rate.py, {torch.cuda.get_device_name(0)}, one process, the same "
                f"allocations, sum, median of {a.reps} after {WARM} warm-ups, times in us.  loop: M "
                "single calls (the faster of two medians, before and after the batch); spread: the "
                "two medians' distance; batch: one batched call; x: loop / batch.\n\n"
                "## (a) raw launchers, HIP events: M osgpu_combine against one osgpu_combine_many\n\n"
                "| type | elements | M | K | loop | spread | batch | x | same bits |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if r["part"] == "raw":
                f.write(f"| {r['type']} | {r['elems']} | {r['M']} | {r['K']} | "
                        f"{min(r['loop_us'], r['loop_us_again']):.1f} | {100 * r['loop_spread']:.1f} % | "
                        f"{r['batch_us']:.1f} | {r['speedup']:.2f} | "
                        f"{'yes' if r['same_bits'] else 'NO'} |\n")
        f.write("\n## (b) collective, threads as PEs, P = 2, device heaps, host wall-clock per step "
                "on PE 0: M shmem_<T>_sum_to_all against one osgpu_reduce_many\n\n"
                "| type | elements | M | loop | path | spread | batch | path | x | same bits |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if r["part"] == "collective":
                f.write(f"| {r['type']} | {r['elems']} | {r['M']} | "
                        f"{min(r['loop_us'], r['loop_us_again']):.1f} | {r['loop_path']} | "
                        f"{100 * r['loop_spread']:.1f} % | {r['batch_us']:.1f} | {r['batch_path']} | "
                        f"{r['speedup']:.2f} | {'yes' if r['same_bits'] else 'NO'} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--table", default=None)
    ap.add_argument("--skip-collective", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed steps"
    import torch
    import osgpu
    assert torch.cuda.is_available(), "many_rate.py measures on the GPU"
    rows = raw(a, torch, osgpu)
    if not a.skip_collective:
        rows += collective(a, torch, osgpu)
    if a.table:
        table(a, torch, rows)


if __name__ == "__main__":
    main()
