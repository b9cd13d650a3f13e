#!/usr/bin/env python3
"""What obstacle shape classes cost the C3 step (lqro_set_obstacles_ex), in Qhull order.

Unused: `bench.py --gpus 1 --steps S --warmup W` itself with this build and
with another library of the same tree (`--parent`, e.g. the parent commit's,
built by scripts/build_rev.sh into lqr-obstacles_amd/), alternating, `--reps`
runs each.

The existing feature in use: scripts/obstacles_bench.py's run (64 bodies at
hover trim inside the swarm's box, the agents' shape, responsibility 1.0)
with both libraries, alternating, `--reps` runs each: that path now goes
through the class lookup.

The new feature in use: the same 64 bodies in 1, 3 and 4 classes of their own
(obstacle o takes class o mod K, radii (0.3 + 0.1 c, 0.8 + 0.1 c); every
fourth responsibility 0.5), `--class-reps` runs each (by lqro_plan.hpp's
pair_layout 3 classes keep C3's 16 waves of k_pair and the 4th costs one).

Every run is a process of its own (one library per process).

  python scripts/obstacle_shapes_bench.py [--parent liblqro_parent.so] [--reps 7] [--class-reps 3] [--out FILE]
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

N, HORIZON, N_POINTS, M = 1024, 100, 100, 64


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_obstacles(libname, classes, steps, warmup):
    import torch
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_newv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    ob, _ = lqro.synthetic_swarm(M, seed=lqro.SEED + 1, box=4.0 * N ** (1.0 / 3.0))   # the swarm's own box
    states = lqro.obstacle_states(ob[:, 0:3])
    if classes == 0:
        ctx.set_obstacles(states)                # the agents' shape, 1.0: the one-shape call
    else:
        cls = np.arange(M) % classes
        ctx.set_obstacles(states, 0.3 + 0.1 * cls, 0.8 + 0.1 * cls, np.where(np.arange(M) % 4 == 3, 0.5, 1.0))
    sid = torch.cuda.current_stream().cuda_stream

    def step():
        ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_newv.data_ptr(), sid)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    st = ctx.stats()
    b = ctx.hull_builds()
    tm = ctx.timings()
    out = {"lib": libname, "classes": classes, "ms_per_step": el / steps * 1e3, "pair_ms": tm["pair_ms"],
           "pairs": st["pairs"], "inside": st["inside"], "inside_obstacle_columns": int((b["j"] >= N).sum()),
           "slowest_build_ms": float((b["t_end"] - b["t_start"]).max() * 1e-5) if len(b) else 0.0,
           "newv_sum": float(d_newv.sum().item())}
    ctx.close()
    print("RESULT " + json.dumps(out))


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


def run_obstacles(libname, classes, steps, warmup):
    out = run(["--child-obstacles", libname, "--classes", str(classes), "--steps", str(steps), "--warmup", str(warmup)])
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(res, file=sys.stderr, flush=True)
    return res


def summary(rs):
    v = [r["ms_per_step"] for r in rs]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)} if v else None


def inside(sp, st):
    return (sp["min"] <= st["median"] <= sp["max"]) if sp and st else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="bench.py's")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--obs-steps", type=int, default=10, help="the runs with obstacles (scripts/obstacles_bench.py's)")
    ap.add_argument("--obs-warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--class-reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="another library in lqr-obstacles_amd/ to alternate with")
    ap.add_argument("--child-bench", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-obstacles", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--classes", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_bench:
        return child_bench(a.child_bench, a.steps, a.warmup)
    if a.child_obstacles:
        return child_obstacles(a.child_obstacles, a.classes, a.steps, a.warmup)
    this, parent, obs_this, obs_parent = [], [], [], []
    for _ in range(a.reps):
        if a.parent:
            parent.append(run_bench(a.parent, a.steps, a.warmup))
        this.append(run_bench("liblqro.so", a.steps, a.warmup))
    for _ in range(a.reps):
        if a.parent:
            obs_parent.append(run_obstacles(a.parent, 0, a.obs_steps, a.obs_warmup))
        obs_this.append(run_obstacles("liblqro.so", 0, a.obs_steps, a.obs_warmup))
    classes = {}
    for _ in range(a.class_reps):
        for k in (1, 3, 4):
            classes.setdefault(str(k), []).append(run_obstacles("liblqro.so", k, a.obs_steps, a.obs_warmup))
    sp, st, op, ot = summary(parent), summary(this), summary(obs_parent), summary(obs_this)
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order",
           "unused": {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", "parent": parent,
                      "this": this, "ms_per_step_parent": sp, "ms_per_step_this": st,
                      "this_median_inside_parent_range": inside(sp, st)},
           "agents_shape_64": {"steps": a.obs_steps, "warmup": a.obs_warmup, "parent": obs_parent, "this": obs_this,
                               "ms_per_step_parent": op, "ms_per_step_this": ot,
                               "this_median_inside_parent_range": inside(op, ot)},
           "own_classes_64": {k: {"runs": v, "ms_per_step": summary(v)} for k, v in classes.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
