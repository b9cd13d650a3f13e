#!/usr/bin/env python3
"""What hard planes cost the C3 step (lqro_set_hard_planes), in Qhull order.

Unused: `bench.py --gpus 1 --steps S --warmup W` itself (its headline,
ms_per_step) with this build and with another library of the same tree
(`--parent`, e.g. the parent commit's, built by scripts/build_rev.sh into
lqr-obstacles_amd/), alternating, `--reps` runs each.  bench.py is run as it
is; the child only points lqro.LIB_PATH at the library before it starts.

In use: bench.py's swarm and timed loop (scripts/fence_cost.py's) with the
6-face fence of profiles/fence_planes_bench.json (the swarm's own box with
1 m of margin, tau 2 s), at LQRO_HARD_NONE and at LQRO_HARD_FENCE,
alternating, `--fence-reps` runs each.

Every run is a process of its own (one library, one context per process).

  python scripts/hard_planes_bench.py [--parent liblqro_parent.so] [--steps 20] [--warmup 5] [--reps 6]
                                      [--fence-reps 3] [--out FILE]
Prints one JSON line; --out also writes it to FILE.
"""
import argparse
import json
import os
import runpy
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lqr-obstacles_amd")
sys.path.insert(0, PKG)

N, HORIZON, N_POINTS = 1024, 100, 100


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_fence(level, steps, warmup):
    import torch
    import lqro
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_newv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    half = 0.5 * 4.0 * N ** (1.0 / 3.0) + 1.0
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    ctx.set_fence([-half] * 3, [half] * 3, 2.0)
    ctx.set_hard_planes(level)
    sid = torch.cuda.current_stream().cuda_stream

    def step():
        ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_newv.data_ptr(), sid)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    lp_ms = []
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        lp_ms.append(ctx.timings()["lp_ms"])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    st = ctx.stats()
    ctx.close()
    print("RESULT " + json.dumps({"level": level, "ms_per_step": el / steps * 1e3, "tail_lp_ms": float(np.mean(lp_ms)),
                                  "inside": st["inside"], "newv_sum": float(d_newv.sum().item())}))


def run(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{args}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return r.stdout


def run_bench(libname, steps, warmup):
    out = run(["--child-bench", libname, "--steps", str(steps), "--warmup", str(warmup)])
    b = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    res = {"lib": libname, "ms_per_step": b["ms_per_step"], "value": b["value"],
           "inside": b["inside_hull_pairs_per_step"]}
    print(res, file=sys.stderr, flush=True)
    return res


def run_fence(level, steps, warmup):
    out = run(["--child-fence", str(level), "--steps", str(steps), "--warmup", str(warmup)])
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(res, file=sys.stderr, flush=True)
    return res


def summary(rs):
    v = [r["ms_per_step"] for r in rs]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--fence-reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="another library in lqr-obstacles_amd/ to alternate with")
    ap.add_argument("--child-bench", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-fence", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_bench:
        return child_bench(a.child_bench, a.steps, a.warmup)
    if a.child_fence is not None:
        return child_fence(a.child_fence, a.steps, a.warmup)
    this, parent, soft, hard = [], [], [], []
    for _ in range(a.reps):
        if a.parent:
            parent.append(run_bench(a.parent, a.steps, a.warmup))
        this.append(run_bench("liblqro.so", a.steps, a.warmup))
    for _ in range(a.fence_reps):
        soft.append(run_fence(0, a.steps, a.warmup))
        hard.append(run_fence(1, a.steps, a.warmup))
    sp, st = summary(parent), summary(this)
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order",
           "command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", "steps": a.steps, "warmup": a.warmup,
           "parent": parent, "this": this, "ms_per_step_parent": sp, "ms_per_step_this": st,
           "this_median_inside_parent_range": (sp["min"] <= st["median"] <= sp["max"]) if sp else None,
           "fence": {"faces": 6, "margin_m": 1.0, "tau": 2.0},
           "fence_level_0": soft, "fence_level_1": hard,
           "ms_per_step_fence_level_0": summary(soft), "ms_per_step_fence_level_1": summary(hard)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
