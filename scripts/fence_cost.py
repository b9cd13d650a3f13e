#!/usr/bin/env python3
"""What a 6-face fence costs the C3 step (lqro_set_fence): bench.py's swarm
and timed loop (warm-up steps, then `--steps` lqro_step_device calls with
lqro_get_timings after each, wall clock over the loop), once without a fence
and once with one, `--reps` times in turn, one context at a time.

With a fence the early LP stays on (1029 x 32 B of LDS per row), k_fence runs
at the head of the step, and the k_qhull job that closes a row leaves its LP
to the tail instead of running it in place (StepPlan::row_lp = 0).

  python scripts/fence_cost.py [--steps 10] [--warmup 3] [--reps 2] [--out FILE]
Prints one JSON line; --out also writes it to FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lqr-obstacles_amd"))

N, HORIZON, N_POINTS = 1024, 100, 100


def run(lqro, torch, gains, d_x, d_vg, d_newv, fence, steps, warmup):
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    if fence is not None:
        ctx.set_fence(*fence)
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
    return {"ms_per_step": el / steps * 1e3, "tail_lp_ms": float(np.mean(lp_ms)), "inside": st["inside"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lqro
    x, vg = lqro.synthetic_swarm(N)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_newv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    # the swarm's own box (side 4 N^(1/3) m) with 1 m of margin: every face is emitted
    half = 0.5 * 4.0 * N ** (1.0 / 3.0) + 1.0
    fence = ([-half] * 3, [half] * 3, 2.0)
    plain, fenced = [], []
    for _ in range(a.reps):
        plain.append(run(lqro, torch, gains, d_x, d_vg, d_newv, None, a.steps, a.warmup))
        fenced.append(run(lqro, torch, gains, d_x, d_vg, d_newv, fence, a.steps, a.warmup))
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order", "steps": a.steps,
           "warmup": a.warmup, "fence": {"lo": fence[0], "hi": fence[1], "tau": fence[2], "faces": 6},
           "no_fence": plain, "fence_6_faces": fenced,
           "ms_per_step_no_fence_median": float(np.median([r["ms_per_step"] for r in plain])),
           "ms_per_step_fence_median": float(np.median([r["ms_per_step"] for r in fenced]))}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
