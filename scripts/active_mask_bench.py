#!/usr/bin/env python3
"""What the activity mask costs (lqro_set_active).

Unused: `bench.py --gpus 1 --steps S --warmup W` itself with this build and
with another library of the same tree (`--parent`, e.g. the parent commit's,
built by scripts/build_rev.sh into lqr-obstacles_amd/), alternating, `--reps`
runs each.  With no mask set the step launches what it launched before.

In use: the C3 step (bench.py's swarm through lqro_step) with 0 %, 25 % (i % 4
== 3) and 50 % (odd i) of the agents inactive, and, for the cost of today's
workaround, with the 25 % parked far away instead (tests/active_ref.py's
formula) and no mask.  Per case the median over the steady steps of: the
step's device time, the slowest hull build (lqro_get_hull_builds), and the
sweep's time; and the step's time of the mask against parking under the two
schedules whose side workgroups sweep rows after their hulls (given no rows
under a mask).  The sweep's time is taken in a second process with LQRO_HOT=0
(the plain schedule): every CU then runs k_pair's row launch between the
step's first two events and nothing beside it, so lqro_get_timings()[0] is
that launch plus the few small kernels ahead of it.

Every run is a process of its own (one library per process).

  python scripts/active_mask_bench.py [--parent liblqro_parent.so] [--reps 5] [--out FILE]
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
CASES = {"active_100": None, "active_75": (4, 3), "active_50": (2, 1), "parked_25": (4, 3)}


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_step(case, steps, warmup):
    import lqro
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    canonical = os.environ.get("ACTIVE_BENCH_RULE") == "canonical"
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=0 if canonical else lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    a = np.ones(N, np.uint8)
    if CASES[case]:
        mod, rem = CASES[case]
        a[np.arange(N) % mod == rem] = 0
    if case.startswith("parked"):
        for k in np.nonzero(a == 0)[0]:   # inactive agent k far away, at rest
            x[k, 0:3] = (1e6 * (k + 1), -2e6 * (k + 1), 3e6)
            x[k, 3:6] = 0.0
    elif CASES[case]:
        ctx.set_active(a)
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
    out = {"case": case, "active": int(a.sum()), "hot": os.environ.get("LQRO_HOT", "1"),
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
        in_use[case] = {"active": hot["active"], "pairs": hot["pairs"], "inside": hot["inside"],
                        "step_ms": hot["step_ms"], "slowest_build_ms": hot["slowest_build_ms"],
                        "row_launch_ms_plain_schedule": plain["pair_ms"], "step_ms_plain_schedule": plain["step_ms"]}
    # the two schedules whose side workgroups sweep rows once their hulls are done (k_side: the
    # canonical rule without the local hull; k_qside: LQRO_QSIDE=1): under a mask they are given
    # no rows, under parking they keep them
    side = {}
    for name, env in (("k_side_canonical_lds_hull", {"ACTIVE_BENCH_RULE": "canonical", "LQRO_LOCAL_HULL": "0"}),
                      ("k_qside", {"LQRO_QSIDE": "1"})):
        side[name] = {case: result(run(["--child-step", case, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                       env=env))["step_ms"] for case in ("active_100", "active_75", "parked_25")}
    sp, st = summary(parent), summary(this)
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order",
           "unused": {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", "parent": parent,
                      "this": this, "ms_per_step_parent": sp, "ms_per_step_this": st,
                      "this_median_inside_parent_range": (sp["min"] <= st["median"] <= sp["max"]) if sp else None},
           "in_use_c3_step": in_use,
           "side_row_tails_step_ms": side,
           "not_measured": ["per-agent gains", "culling", "more than one GPU"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
