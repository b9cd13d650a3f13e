#!/usr/bin/env python3
"""What the interaction classes cost (lqro_set_interaction).

Unused: `bench.py --gpus 1 --steps S --warmup W` itself with this build and
with another library of the same tree (`--parent`, e.g. the parent commit's,
built into lqr-obstacles_amd/), alternating, `--reps` runs each: the parent's
own run-to-run spread, and where this build's runs lie in it.  With no table
set the step launches what it launched before.

In use: the C3 step (bench.py's swarm through lqro_step) without a table, with
`uniform` (3 classes, every share 0.5: the lookup alone) and with `teams` over
4 classes (class i % 4, the diagonal 0: a row ignores its own quarter).  Per
case the median over the steady steps of the step's device time and the slowest
hull build; and the pair sweep's time, taken in a second process with
LQRO_HOT=0 (the plain schedule: every CU runs k_pair's row launch between the
step's first two events and nothing beside it, so lqro_get_timings()[0] is that
launch plus the few small kernels ahead of it), reported for `teams` against
the live-slot ratio.

Every run is a process of its own (one library per process).

  python scripts/interaction_bench.py [--parent liblqro_parent.so] [--reps 5] [--out FILE]
Prints one JSON line; --out also writes it to FILE.
"""
import argparse
import json
import os
import runpy
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lqr-obstacles_amd")
sys.path.insert(0, PKG)

N, HORIZON, N_POINTS = 1024, 100, 100
CASES = ("no_table", "uniform", "teams_c4")


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_step(case, steps, warmup):
    import lqro
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    if case == "uniform":
        ctx.set_interaction(np.arange(N) % 3, np.full((3, 3), 0.5))
    elif case == "teams_c4":
        ctx.set_interaction(np.arange(N) % 4, np.full((4, 4), 0.5) - 0.5 * np.eye(4))
    step_ms, pair_ms, build_ms = [], [], []
    for k in range(warmup + steps):
        try:
            ctx.step(x, vg)
        except lqro.QhullMergeSuspect:
            pass
        if k < warmup:
            continue
        t = ctx.timings()
        b = ctx.hull_builds()
        step_ms.append(t["step_ms"])
        pair_ms.append(t["pair_ms"])
        build_ms.append(float((b["t_end"].astype(np.int64) - b["t_start"].astype(np.int64)).max()) / 1e5 if len(b) else 0.0)
    st = ctx.stats()
    out = {"case": case, "hot": os.environ.get("LQRO_HOT", "1"),
           "step_ms": float(np.median(step_ms)), "pair_ms": float(np.median(pair_ms)),
           "slowest_build_ms": float(np.median(build_ms)), "pairs": st["pairs"], "inside": st["inside"]}
    ctx.close()
    print("RESULT " + json.dumps(out))


def run(args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
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
    res = {"lib": libname, "ms_per_step": b["ms_per_step"], "value": b["value"]}
    print(res, file=sys.stderr, flush=True)
    return res


def summary(rs):
    v = [r["ms_per_step"] for r in rs]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="bench.py's")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="another library in lqr-obstacles_amd/ to alternate with")
    ap.add_argument("--child-bench", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_bench:
        return child_bench(a.child_bench, a.steps, a.warmup)
    if a.child_step:
        return child_step(a.child_step, a.steps, a.warmup)
    this, parent = [], []
    for _ in range(a.reps):
        if a.parent:
            parent.append(run_bench(a.parent, a.steps, a.warmup))
        this.append(run_bench("liblqro.so", a.steps, a.warmup))
    in_use = {}
    for case in CASES:
        args = ["--child-step", case, "--steps", str(a.steps), "--warmup", str(a.warmup)]
        hot = result(run(args))
        plain = result(run(args, env={"LQRO_HOT": "0"}))
        in_use[case] = {"pairs": hot["pairs"], "inside": hot["inside"], "step_ms": hot["step_ms"],
                        "slowest_build_ms": hot["slowest_build_ms"], "pair_sweep_ms_plain_schedule": plain["pair_ms"],
                        "step_ms_plain_schedule": plain["step_ms"]}
    base, teams = in_use["no_table"], in_use["teams_c4"]
    sp, st = summary(parent), summary(this)
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order",
           "unused": {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", "parent": parent,
                      "this": this, "ms_per_step_parent": sp, "ms_per_step_this": st,
                      "this_median_inside_parent_range": (sp["min"] <= st["median"] <= sp["max"]) if sp else None},
           "in_use_c3_step": in_use,
           "uniform_over_no_table_step": in_use["uniform"]["step_ms"] / base["step_ms"],
           "teams_c4": {"live_slot_ratio": teams["pairs"] / base["pairs"],
                        "pair_sweep_ratio": teams["pair_sweep_ms_plain_schedule"] / base["pair_sweep_ms_plain_schedule"],
                        "step_ratio": teams["step_ms"] / base["step_ms"]},
           "not_measured": ["per-agent gains", "culling", "more than one GPU"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
