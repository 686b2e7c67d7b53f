#!/usr/bin/env python3
"""rscatter_rate.py -- rate of the shifted combine (osgpu_combine_shifted, the
kernel under osgpu_reduce_scatter) in ONE process on the SAME allocations,
and the in-process A/B of its shapes.  Not part of the product.

  python tools/rscatter_rate.py build            (on the CPU: the variants)
  python tools/rscatter_rate.py run [--table F]  (on the GPU)

Per case -- double, float, int and short sum; K in {2, 4, 8} inputs;
--target-mib of target -- three launches are timed:
  (a) osgpu_combine on same-phase pointers: the ceiling (the LDS combine);
  (b) osgpu_combine on the shifted pointers: what a caller had before, the
      element-granular kernel (that entry point is unchanged);
  (c) osgpu_combine_shifted on the same shifted pointers.
The shifted pointers: input k starts ((k + 1) mod W) elements into its
allocation (W = 16 / element size), the target 0, so every input but each
W-th sits at a phase of its own.  (c)'s output is compared with (b)'s bit for
bit.

Variants: `build` compiles csrc/combine.hip with -DOSGPU_SHIFT_U=1|2|4 and
links each with the tree's other objects into
tools/variants/rs_U<u>/libosgpu_reduce.so (RS_VARIANTS_DIR: another
directory for them), with -Bsymbolic so that a
build's entry points reach that build's own launcher and kernels whatever
else the process holds.  `run` loads the shipped library and every variant
RTLD_LOCAL (never through osgpu.load(), whose RTLD_GLOBAL would put the
shipped launcher in front of every variant's), times each one's (c) on the
same arrays, and has each build say which shape it holds and that its own
shift kernel was launched (osgpu_test_shift_routes).
(The run recorded in profiles/rscatter_rate.md also held a second form of the
kernel's shifted LDS read, -DOSGPU_SHIFT_READ=1, as columns U<u>r1; it timed
the same and its branch is gone from combine.hip.)

HIP events around each launch, median of --reps (>= 20) after 3 warm-up
launches.  JSON lines on stdout; --table FILE writes the markdown table
(profiles/rscatter_rate.md)."""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "test-resilient-osss-ucx_amd")
CSRC = os.path.join(PKG, "csrc")
VAR = os.path.join(ROOT, "tools", "variants")
SHAPES = [1, 2, 4]
FL = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
      "-fno-fast-math"]
OTHERS = ["team.o", "fused.o", "verify.o", "longdouble.o", "copy.o", "host_fold.o", "runtime.o",
          "heap.o", "fd_channel.o", "shmem_reduce.o", "shmem_collect.o"]
TYPES = {"double": ("float64", 8), "float": ("float32", 4), "int": ("int32", 4),
         "short": ("int16", 2)}


def vname(u):
    return f"U{u}"


def vpath(u):
    return os.path.join(os.environ.get("RS_VARIANTS_DIR", VAR), "rs_" + vname(u),
                        "libosgpu_reduce.so")


def build():
    subprocess.run(["make", "-s", "-j8"], cwd=CSRC, check=True)
    procs = []
    for u in SHAPES:
        os.makedirs(os.path.dirname(vpath(u)), exist_ok=True)
        procs.append(subprocess.Popen(
            ["/opt/rocm/bin/hipcc"] + FL + [f"-DOSGPU_SHIFT_U={u}", "-c",
                                            os.path.join(CSRC, "combine.hip"), "-o",
                                            os.path.join(os.path.dirname(vpath(u)), "combine.o")]))
    assert all(p.wait() == 0 for p in procs)
    for u in SHAPES:
        d = os.path.dirname(vpath(u))
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC",
                        "-Wl,-Bsymbolic", "-o", vpath(u), os.path.join(d, "combine.o")]
                       + [os.path.join(CSRC, o) for o in OTHERS] + ["-lrccl", "-ldl", "-lpthread"],
                       check=True)
        print("built", vname(u))


def open_lib(path):
    L = ctypes.CDLL(path, mode=os.RTLD_LOCAL)
    sig = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
           ctypes.c_size_t, ctypes.c_void_p]
    L.osgpu_combine.argtypes = sig
    L.osgpu_combine_shifted.argtypes = sig
    L.osgpu_test_shift_routes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong * 4),
                                          ctypes.POINTER(ctypes.c_int)]
    return L


def routes(L):
    """(counts, U) of ONE build: osgpu_test_shift_routes."""
    c, u = (ctypes.c_ulonglong * 4)(), ctypes.c_int()
    assert L.osgpu_test_shift_routes(ctypes.byref(c), ctypes.byref(u)) == 0
    return list(c), u.value


def run(a):
    os.environ["OSGPU_TEST_HOOKS"] = "1"
    sys.path.insert(0, PKG)
    import torch
    import osgpu  # the type codes only: osgpu.load() is never called here
    assert a.reps >= 20 or a.target_mib < 8, "at least 20 timed launches"
    assert torch.cuda.is_available(), "rscatter_rate.py measures on the GPU"
    torch.cuda.init()

    L = open_lib(os.path.join(PKG, "libosgpu_reduce.so"))
    shipped_shape = routes(L)[1]
    variants = {}
    for u in ([] if a.no_variants else SHAPES):
        V = open_lib(vpath(u))
        assert routes(V)[1] == u, f"{vname(u)} holds U = {routes(V)[1]}"
        variants[vname(u)] = V
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    nbytes = a.target_mib << 20
    kmax = max(a.ks)
    bufs = [torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda") for _ in range(kmax)]
    out = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    ref = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")

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
    for t in a.types:
        dtn, s = TYPES[t]
        tc = osgpu.type_code(t)
        dt = getattr(torch, dtn)
        W = 16 // s
        n = nbytes // s
        for b in bufs:   # small values: no overflow traps, no NaNs
            v = b[:nbytes].view(dt)
            v.copy_(torch.randint(-3, 4, (n,), device="cuda").to(dt))
        torch.cuda.synchronize()
        for K in a.ks:
            same = (ctypes.c_void_p * K)(*[bufs[k].data_ptr() for k in range(K)])
            shifts = [((k + 1) % W) for k in range(K)]
            shifted = (ctypes.c_void_p * K)(*[bufs[k].data_ptr() + shifts[k] * s
                                              for k in range(K)])
            m = n - W  # every shifted input still holds m elements

            def fa():
                assert L.osgpu_combine(tc, 0, out.data_ptr(), same, K, m, sp) == 0

            def fb():
                assert L.osgpu_combine(tc, 0, ref.data_ptr(), shifted, K, m, sp) == 0

            def fc(lib=L):
                assert lib.osgpu_combine_shifted(tc, 0, out.data_ptr(), shifted, K, m, sp) == 0

            def own_kernel(lib, fn):
                """time fn; True when it was lib's OWN shift kernel that ran"""
                before = {id(x): routes(x)[0] for x in [L] + list(variants.values())}
                us = timed(fn) * 1e6
                after = {id(x): routes(x)[0] for x in [L] + list(variants.values())}
                mine = all(after[id(x)] == before[id(x)] if x is not lib else
                           after[id(x)][1] - before[id(x)][1] == a.reps + 3
                           for x in [L] + list(variants.values()))
                return us, mine

            row = {"type": t, "K": K, "elems": m, "shifts": shifts,
                   "bytes": (K + 1) * m * s}
            row["a_us"] = timed(fa) * 1e6
            row["b_us"] = timed(fb) * 1e6
            row["c_us"], row["c_own_kernel"] = own_kernel(L, fc)
            torch.cuda.synchronize()
            row["c_equals_b"] = bool(torch.equal(out[:m * s], ref[:m * s]))
            for name, V in variants.items():
                out.zero_()
                row[name + "_us"], row[name + "_own_kernel"] = own_kernel(V, lambda: fc(V))
                torch.cuda.synchronize()
                row[name + "_equals_b"] = bool(torch.equal(out[:m * s], ref[:m * s]))
            row["c_us_again"] = timed(fc) * 1e6
            row["a_us_again"] = timed(fa) * 1e6
            c, a_ = min(row["c_us"], row["c_us_again"]), min(row["a_us"], row["a_us_again"])
            row["c_over_a"] = a_ / c          # rate of (c) as a fraction of (a)'s
            row["c_over_b"] = row["b_us"] / c  # speed-up over what the caller had
            row["c_GBps"] = row["bytes"] / c / 1e3
            rows.append(row)
            print(json.dumps(row), flush=True)

    names = list(variants)
    gm = {nm: math.exp(sum(math.log(r[nm + "_us"]) for r in rows) / len(rows)) for nm in names}
    gm["shipped"] = math.exp(sum(math.log(min(r["c_us"], r["c_us_again"])) for r in rows) / len(rows))
    print(json.dumps({"geomean_us": gm, "shipped_shape": shipped_shape}), flush=True)

    if a.table:
        with open(a.table, "w") as f:
            f.write(f"# Shifted combine (reduce-scatter kernel): rates and the shape A/B\n\n"
                    f"tools/rscatter_rate.py, {torch.cuda.get_device_name(0)}, one process, "
                    f"{a.target_mib} MiB of target per case, sum, HIP events, median of {a.reps} "
                    f"after 3 warm-up launches, times in us.  (a) osgpu_combine on same-phase "
                    f"pointers (the faster of two timings, first and last of the case); (b) "
                    f"osgpu_combine on the shifted pointers (the element-granular kernel; ONE "
                    f"timing); (c) osgpu_combine_shifted on the same shifted pointers, the "
                    f"shipped build U{shipped_shape} (the faster of two "
                    f"timings, before and after the variants).  c/a: (c)'s rate as a fraction "
                    f"of (a)'s; c/b: its speed-up over (b).  GB/s: (K + 1) x elements x size "
                    f"over (c)'s time.  Variant columns: (c) of a build with U vectors per lane "
                    f"per input, each loaded RTLD_LOCAL and linked -Bsymbolic; "
                    f"'own kernel': every build reported its own shape and only its own launch "
                    f"counter moved while it was timed.\n\n")
            f.write("| type | K | (a) | (b) | (c) | c/a | c/b | (c) GB/s | same bits as (b), all "
                    "builds | own kernel, all builds | " + " | ".join(names) + " |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|" + "---|" * len(names) + "\n")
            for r in rows:
                ok = r["c_equals_b"] and all(r[nm + "_equals_b"] for nm in names)
                own = r["c_own_kernel"] and all(r[nm + "_own_kernel"] for nm in names)
                f.write(f"| {r['type']} | {r['K']} | {min(r['a_us'], r['a_us_again']):.0f} | "
                        f"{r['b_us']:.0f} | {min(r['c_us'], r['c_us_again']):.0f} | "
                        f"{r['c_over_a']:.3f} | {r['c_over_b']:.2f} | {r['c_GBps']:.0f} | "
                        f"{'yes' if ok else 'NO'} | {'yes' if own else 'NO'} | "
                        + " | ".join(f"{r[nm + '_us']:.0f}" for nm in names) + " |\n")
            f.write("\nGeometric-mean time of (c) over the cases (us), lowest first: "
                    + ", ".join(f"{k} {v:.1f}" for k, v in sorted(gm.items(), key=lambda kv: kv[1]))
                    + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["build", "run"])
    ap.add_argument("--target-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--types", nargs="+", default=list(TYPES))
    ap.add_argument("--no-variants", action="store_true", help="the shipped build alone")
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    build() if a.what == "build" else run(a)


if __name__ == "__main__":
    main()
