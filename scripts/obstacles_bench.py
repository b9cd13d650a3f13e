#!/usr/bin/env python3
"""What obstacle columns cost the C3 step (lqro_set_obstacles), in Qhull order.

Unused: bench.py's swarm and timed loop (warm-up steps, then `--steps`
lqro_step_device calls, wall clock over the loop ending in a synchronise)
with this build and with another library of the same tree (`--parent`, e.g.
the parent commit's, built by scripts/build_rev.sh into lqr-obstacles_amd/),
alternating, `--reps` runs each.

In use: the same loop with `--obstacles` (default 64) bodies at hover trim
inside the swarm's box (positions from synthetic_swarm's stream at seed + 1,
at rest), the agents' shape, responsibility 1.0: ms per
step, the inside-hull pairs whose column is an obstacle, and the slowest
build (lqro_get_hull_builds, 100 MHz ticks) beside the plain step's.

Every run is a process of its own (one library per process).

  python scripts/obstacles_bench.py [--parent liblqro_parent.so] [--steps 10] [--warmup 3] [--reps 3] [--out FILE]
Prints one JSON line; --out also writes it to FILE.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lqr-obstacles_amd")
sys.path.insert(0, PKG)

N, HORIZON, N_POINTS = 1024, 100, 100


def child(libname, m, steps, warmup):
    import torch
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_newv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    if m > 0:
        ob, _ = lqro.synthetic_swarm(m, seed=lqro.SEED + 1, box=4.0 * N ** (1.0 / 3.0))   # the swarm's own box
        ctx.set_obstacles(lqro.obstacle_states(ob[:, 0:3]))
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
    out = {"lib": libname, "obstacles": m, "ms_per_step": el / steps * 1e3, "last_step_ms": tm["step_ms"],
           "pair_ms": tm["pair_ms"], "pairs": st["pairs"], "inside": st["inside"],
           "inside_obstacle_columns": int((b["j"] >= N).sum()),
           "slowest_build_ms": float((b["t_end"] - b["t_start"]).max() * 1e-5) if len(b) else 0.0,
           "newv_sum": float(d_newv.sum().item())}
    ctx.close()
    print("RESULT " + json.dumps(out))


def run(libname, m, steps, warmup):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", libname, "--obstacles", str(m),
                        "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{libname} m={m}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--obstacles", type=int, default=64, help="0: the unused cost only")
    ap.add_argument("--parent", default=None, help="another library in lqr-obstacles_amd/ to alternate with")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.obstacles, a.steps, a.warmup)
    this, parent, used = [], [], []
    for _ in range(a.reps):
        if a.parent:
            parent.append(run(a.parent, 0, a.steps, a.warmup))
        this.append(run("liblqro.so", 0, a.steps, a.warmup))
        if a.obstacles > 0:
            used.append(run("liblqro.so", a.obstacles, a.steps, a.warmup))
    med = lambda rs: float(np.median([r["ms_per_step"] for r in rs])) if rs else None
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order", "steps": a.steps,
           "warmup": a.warmup, "parent": parent, "this": this, "with_obstacles": used,
           "ms_per_step_parent_median": med(parent), "ms_per_step_this_median": med(this),
           "ms_per_step_with_obstacles_median": med(used),
           "parent_spread_ms": (max(r["ms_per_step"] for r in parent) - min(r["ms_per_step"] for r in parent))
           if parent else None,
           "sweep_growth_expected": (N - 1 + a.obstacles) / (N - 1)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
