"""bench.py's plain run: it stops at the headline (nothing of --full in the
result line), --steps is the number of timed steps, and --dump-outputs writes
the last timed step's new velocities — bit for bit what a context returns
after the same warm-up + timed steps on the same seeded swarm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("cpu_baseline", "gpu_over_cpu", "configs", "host_cpp")


def test_plain_run_dumps_last_step(lqro_mod, tmp_path):
    steps, warmup = 2, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["metric"] == "agent-pair LQR-obstacle evals/sec" and line["unit"] == "agent-pair evals/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value is pairs per second of the timed steps
    assert line["value"] == pytest.approx(1024 * 1023 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in FULL_ONLY:
        assert k not in line, k
    assert line["closed_loop"] is None and line["hull_rule_canonical"] is None and line["critical"] is None
    assert line["hull_failures"] == 0 and line["inside_hull_pairs_per_step"] > 100
    assert sorted(os.listdir(out)) == ["newv.npy"]
    newv = np.load(out / "newv.npy")
    assert newv.dtype == np.float64 and newv.shape == (1024, 3)
    # the same steps in this process (the bench's default rule and swarm)
    x, vg = lqro_mod.synthetic_swarm(1024)
    g = lqro_mod.synthesize_gains()
    ctx = lqro_mod.Context(lqro_mod.config(1024, 100, 100, flags=lqro_mod.LQRO_FLAG_QHULL_ORDER))
    ctx.set_gains(g["A"], g["B"], g["L"], g["E"])
    try:
        for _ in range(warmup + steps):
            v = ctx.step(x, vg)
    finally:
        ctx.close()
    assert np.array_equal(newv.view(np.uint64), v.view(np.uint64))
