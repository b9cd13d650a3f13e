#!/usr/bin/env python3
"""What the horizon conflict prediction costs (lqro_predict[_device]).

Unused: `bench.py --gpus 1 --steps S --warmup W` itself with this build and
with another library of the same tree (`--parent`, e.g. the parent commit's,
built by scripts/build_rev.sh into lqr-obstacles_amd/), alternating, `--reps`
runs each.  An unused prediction adds no launch.

In use: the launches' own times from HIP events (lqro_debug_predict_times,
median of `--kernel-reps`) at C3's shape (1,024 rows x 1,024 columns x H 100,
shared gains) and at a C5 shard's (2,048 rows x 16,384 columns x H 200, X = 12,
per-agent gains), each beside its fp64 vector floor: pair-slices x the 14
operations k_conf spends on one (11 fp64 additions and multiplications, 3
compares) / 78.6 TFLOP/s.  The contexts are created with 20 sphere points: the
prediction reads the tables, not the spheres.

Every run is a process of its own (one library per process).

  python scripts/predict_bench.py [--parent liblqro_parent.so] [--reps 7] [--out FILE]
Prints one JSON line; --out also writes it to FILE.
"""
import argparse
import ctypes
import json
import os
import runpy
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lqr-obstacles_amd")
sys.path.insert(0, PKG)

FP64_VECTOR_FLOPS = 78.6e12
OPS_PER_PAIR_SLICE = 14
SHAPES = {"c3": dict(n=1024, rows=1024, h=100, x_dim=16, per_agent=False),
          "c5_shard": dict(n=16384, rows=2048, h=200, x_dim=12, per_agent=True)}
LAUNCHES = ("k_pred_paths", "k_conf", "k_conf_obs", "k_conf_total")


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_kernels(shape, reps, warmup):
    import torch
    import lqro
    s = SHAPES[shape]
    n, xd = s["n"], s["x_dim"]
    x, vg = lqro.synthetic_swarm(n, x_dim=xd)
    d_x, d_v = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    ctx = lqro.Context(lqro.config(n, s["h"], 20, x_dim=xd, flags=0, row_begin=0, row_end=s["rows"]))
    ab = lqro.synthesize_gains(x_dim=xd)
    if s["per_agent"]:
        g = lqro.synthesize_gains_batch(lqro.perturbed_models(n), x_dim=xd)
        ctx.set_gains(ab["A"], ab["B"], g["L"], g["E"], per_agent=True)
    else:
        ctx.set_gains(ab["A"], ab["B"], ab["L"], ab["E"])
    fn = lqro.lib().lqro_debug_predict_times
    fn.argtypes = [ctypes.c_void_p] * 4
    ms = np.zeros(4, np.float32)
    runs = []
    for k in range(warmup + reps):
        rc = fn(ctx._h, d_x.data_ptr(), d_v.data_ptr(), ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"lqro_debug_predict_times: {rc}")
        if k >= warmup:
            runs.append(ms.astype(float).tolist())
    last, _ = ctx.prediction()
    runs = np.array(runs)
    med = np.median(runs, axis=0)
    slices = s["rows"] * (n - 1) * s["h"]
    floor = slices * OPS_PER_PAIR_SLICE / FP64_VECTOR_FLOPS * 1e3
    out = {"shape": shape, "rows": s["rows"], "columns": n, "horizon": s["h"], "per_agent": s["per_agent"], "reps": reps,
           "ms": dict(zip(LAUNCHES, med.tolist())), "ms_min": dict(zip(LAUNCHES, runs.min(axis=0).tolist())),
           "pair_slices": slices, "fp64_floor_ms": floor, "k_conf_fraction_of_floor": floor / float(med[1]),
           "n_conf": last["n_conf"], "n_rows_conf": last["n_rows_conf"], "first_k": last["first_k"],
           "s2_min": last["s2_min"]}
    ctx.close()
    print("RESULT " + json.dumps(out))


def run(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{args}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return r.stdout


def result(out):
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(res, file=sys.stderr, flush=True)
    return res


def run_bench(libname, steps, warmup):
    out = run(["--child-bench", libname, "--steps", str(steps), "--warmup", str(warmup)])
    b = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    res = {"lib": libname, "ms_per_step": b["ms_per_step"], "value": b["value"],
           "inside": b["inside_hull_pairs_per_step"]}
    print(res, file=sys.stderr, flush=True)
    return res


def summary(rs):
    v = [r["ms_per_step"] for r in rs]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="bench.py's")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--shapes", default="c3,c5_shard")
    ap.add_argument("--parent", default=None, help="another library in lqr-obstacles_amd/ to alternate with")
    ap.add_argument("--child-bench", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-kernels", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_bench:
        return child_bench(a.child_bench, a.steps, a.warmup)
    if a.child_kernels:
        return child_kernels(a.child_kernels, a.kernel_reps, 3)
    this, parent = [], []
    for _ in range(a.reps):
        if a.parent:
            parent.append(run_bench(a.parent, a.steps, a.warmup))
        this.append(run_bench("liblqro.so", a.steps, a.warmup))
    kernels = {k: result(run(["--child-kernels", k, "--kernel-reps", str(a.kernel_reps)]))
               for k in a.shapes.split(",") if k}
    sp, st = summary(parent), summary(this)
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order",
           "unused": {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", "parent": parent,
                      "this": this, "ms_per_step_parent": sp, "ms_per_step_this": st,
                      "this_median_inside_parent_range": (sp["min"] <= st["median"] <= sp["max"]) if sp and st else None},
           "kernels": kernels,
           "rates": {"fp64_vector_flops": FP64_VECTOR_FLOPS, "ops_per_pair_slice": OPS_PER_PAIR_SLICE},
           "not_measured": ["more than one GPU", "obstacle columns (k_conf_obs) at these shapes",
                            "the given-paths calls (k_pred_tr)", "a swarm where most rows have a conflict"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
