#!/usr/bin/env python3
"""What the clearance monitor costs (lqro_set_monitor, lqro_clearance).

Unused: `bench.py --gpus 1 --steps S --warmup W` itself with this build and
with another library of the same tree (`--parent`, e.g. the parent commit's,
built by scripts/build_rev.sh into lqr-obstacles_amd/), alternating, `--reps`
runs each.  An unused monitor adds no launch.

In use: the C3 step (bench.py's swarm through lqro_step_device) with the
monitor on against the monitor off, alternating, `--step-reps` runs each; and
the three kernels' own times from HIP events (lqro_debug_clearance_times) at
C3's shape (1024 rows x 1024 columns) and at a C5 shard's (2,048 rows x 16,384
columns), beside the bytes k_clear must move and the time those take at the
HBM and L2 rates of the MI355X.  The C5-shard context is created with a short
horizon (10 x 20 points): the measurement reads positions only, and the
step's tables would only take memory.

Every run is a process of its own (one library per process).

  python scripts/clearance_bench.py [--parent liblqro_parent.so] [--reps 7] [--step-reps 3] [--out FILE]
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
HBM_BPS, L2_BPS = 6.3e12, 34.5e12      # achievable HBM3E and aggregate L2 rates
TR = 16                                # k_clear's own rows a workgroup
SHAPES = {"c3": dict(n=1024, rows=1024, h=HORIZON, npts=N_POINTS),
          "c5_shard": dict(n=16384, rows=2048, h=10, npts=20)}


def child_bench(libname, steps, warmup):
    import lqro
    lqro.LIB_PATH = os.path.join(PKG, libname)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child_step(monitor, steps, warmup):
    import torch
    import lqro
    x, vg = lqro.synthetic_swarm(N)   # (bench.py's swarm)
    gains = lqro.synthesize_gains()
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_newv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    ctx = lqro.Context(lqro.config(N, HORIZON, N_POINTS, flags=lqro.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    ctx.set_monitor(monitor)
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
    last, since = ctx.monitor()
    out = {"monitor": monitor, "ms_per_step": el / steps * 1e3, "n_measured": since["n_measured"],
           "n_hit": last["n_hit"], "newv_sum": float(d_newv.sum().item())}
    ctx.close()
    print("RESULT " + json.dumps(out))


def traffic(rows, cols):
    """The bytes k_clear must move: every workgroup of TR rows streams the five
    packed column arrays (40 B a column) once, from L2 after the first; HBM
    sees the pack once and the 64-byte row records."""
    l2 = -(-rows // TR) * 40 * cols
    hbm = 40 * cols + 64 * rows
    return {"l2_bytes": l2, "hbm_bytes": hbm, "l2_floor_ms": l2 / L2_BPS * 1e3, "hbm_floor_ms": hbm / HBM_BPS * 1e3,
            "pairs": rows * (cols - 1)}


def child_kernels(shape, reps, warmup):
    import torch
    import lqro
    s = SHAPES[shape]
    n = s["n"]
    x, _ = lqro.synthetic_swarm(n)
    d_x = torch.from_numpy(x.copy()).cuda()
    ctx = lqro.Context(lqro.config(n, s["h"], s["npts"], flags=0, row_begin=0, row_end=s["rows"]))
    fn = lqro.lib().lqro_debug_clearance_times
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    ms = np.zeros(3, np.float32)
    runs = []
    for k in range(warmup + reps):
        rc = fn(ctx._h, d_x.data_ptr(), ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"lqro_debug_clearance_times: {rc}")
        if k >= warmup:
            runs.append(ms.astype(float).tolist())
    last, _ = ctx.monitor()
    med = np.median(np.array(runs), axis=0)
    out = {"shape": shape, "rows": s["rows"], "columns": n, "reps": reps,
           "ms": {"k_clear_pack": float(med[0]), "k_clear": float(med[1]), "k_clear_total": float(med[2])},
           "ms_min": {"k_clear_pack": float(np.min(np.array(runs)[:, 0])), "k_clear": float(np.min(np.array(runs)[:, 1])),
                      "k_clear_total": float(np.min(np.array(runs)[:, 2]))},
           "k_clear_traffic": traffic(s["rows"], n), "n_hit": last["n_hit"], "s2_min": last["s2_min"]}
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
           "in_use_c3_step": {"steps": a.steps, "warmup": a.warmup, "monitor_off": off, "monitor_on": on,
                              "ms_per_step_off": summary(off), "ms_per_step_on": summary(on)},
           "kernels": kernels,
           "rates": {"hbm_bytes_per_s": HBM_BPS, "l2_bytes_per_s": L2_BPS},
           "not_measured": ["more than one GPU", "the crowded swarm (scripts/crowded.py)"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
