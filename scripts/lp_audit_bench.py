#!/usr/bin/env python3
"""What the LP audit costs (lqro_set_lp_audit).

Unused: `bench.py --gpus 1 --steps S --warmup W` itself with this build and
with another library of the same tree (`--parent`, e.g. the parent commit's,
built by scripts/build_rev.sh into lqr-obstacles_amd/), alternating, `--reps`
runs each.  An unused audit adds no launch.

In use: the C3 step (bench.py's swarm through lqro_step_device) with the audit
on against the audit off, alternating, `--step-reps` runs each; and the two
kernels' own times from HIP events (lqro_debug_lp_audit_times, the last step's
audit once more) at C3's shape (1,024 rows x 1,023 slots) and at the C4
shard's (512 rows x 4,095 slots), beside the bytes k_lp_audit must read
(32 B a slot) and the time those take at the HBM rate of the MI355X.  The
C4-shard context is created with a short horizon (10 x 20 points): the audit
reads the slots, whatever filled them.

Every run is a process of its own (one library per process).

  python scripts/lp_audit_bench.py [--parent liblqro_parent.so] [--reps 7] [--step-reps 3] [--out FILE]
Prints one JSON line; --out also writes it to FILE.
"""
import argparse
import ctypes
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
HBM_BPS = 6.3e12                       # achievable HBM3E rate
SHAPES = {"c3": dict(n=1024, rows=1024, h=HORIZON, npts=N_POINTS),
          "c4_shard": dict(n=4096, rows=512, h=10, npts=20)}


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_step(audit, steps, warmup):
    import torch
    import lqro
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_newv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    ctx.set_lp_audit(audit, lqro.RVO_EPSILON)
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
    last, since = ctx.lp_audit()
    out = {"audit": audit, "ms_per_step": el / steps * 1e3, "n_measured": since["n_measured"],
           "n_planes": last["n_planes"], "n_rows_viol": last["n_rows_viol"], "viol_max": float(last["viol_max"]),
           "newv_sum": float(d_newv.sum().item())}
    ctx.close()
    print("RESULT " + json.dumps(out))


def traffic(rows, npr):
    """The bytes k_lp_audit must read: every slot of every own row once, 32 B
    (two 16-byte loads), and 64 B a row written."""
    b = rows * npr * 32 + rows * 64
    return {"bytes": b, "hbm_floor_ms": b / HBM_BPS * 1e3, "slots": rows * npr}


def child_kernels(shape, reps, warmup):
    import torch
    import lqro
    s = SHAPES[shape]
    n = s["n"]
    x, vg = lqro.synthetic_swarm(n)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_newv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    ctx = lqro.Context(lqro.config(n, s["h"], s["npts"], flags=lqro.LQRO_FLAG_QHULL_ORDER, row_begin=0,
                                   row_end=s["rows"]))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    ctx.set_lp_audit(1, lqro.RVO_EPSILON)
    ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_newv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fn = lqro.lib().lqro_debug_lp_audit_times
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    ms = np.zeros(2, np.float32)
    runs = []
    for k in range(warmup + reps):
        rc = fn(ctx._h, ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"lqro_debug_lp_audit_times: {rc}")
        if k >= warmup:
            runs.append(ms.astype(float).tolist())
    last, _ = ctx.lp_audit()
    runs = np.array(runs)
    med = np.median(runs, axis=0)
    out = {"shape": shape, "rows": s["rows"], "slots_per_row": n - 1, "reps": reps,
           "ms": {"k_lp_audit": float(med[0]), "k_lp_audit_total": float(med[1])},
           "ms_min": {"k_lp_audit": float(runs[:, 0].min()), "k_lp_audit_total": float(runs[:, 1].min())},
           "k_lp_audit_traffic": traffic(s["rows"], n - 1), "n_planes": last["n_planes"]}
    ctx.close()
    print("RESULT " + json.dumps(out))


def run(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=300)
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
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="another library in lqr-obstacles_amd/ to alternate with")
    ap.add_argument("--child-bench", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-step", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-kernels", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_bench:
        return child_bench(a.child_bench, a.steps, a.warmup)
    if a.child_step is not None:
        return child_step(a.child_step, a.steps, a.warmup)
    if a.child_kernels:
        return child_kernels(a.child_kernels, a.kernel_reps, 3)
    this, parent, on, off = [], [], [], []
    for _ in range(a.reps):
        if a.parent:
            parent.append(run_bench(a.parent, a.steps, a.warmup))
        this.append(run_bench("liblqro.so", a.steps, a.warmup))
    for _ in range(a.step_reps):
        off.append(result(run(["--child-step", "0", "--steps", str(a.steps), "--warmup", str(a.warmup)])))
        on.append(result(run(["--child-step", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)])))
    kernels = {k: result(run(["--child-kernels", k, "--kernel-reps", str(a.kernel_reps)])) for k in SHAPES}
    sp, st = summary(parent), summary(this)
    out = {"workload": "C3: 1024 quadrotors, horizon 100, 100 points, Qhull order",
           "unused": {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}", "parent": parent,
                      "this": this, "ms_per_step_parent": sp, "ms_per_step_this": st,
                      "this_median_inside_parent_range": (sp["min"] <= st["median"] <= sp["max"]) if sp else None},
           "in_use_c3_step": {"steps": a.steps, "warmup": a.warmup, "audit_off": off, "audit_on": on,
                              "ms_per_step_off": summary(off), "ms_per_step_on": summary(on)},
           "kernels": kernels,
           "rates": {"hbm_bytes_per_s": HBM_BPS},
           "not_measured": ["more than one GPU", "rows with thousands of user planes (up to 8,192 an agent)"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
