"""Fence and user planes (lqro_set_fence, lqro_set_user_planes[_device]) on
the CPU: what the step's planner does with a row's extra planes, the C++
host's two new calls, and Simulator.step's re-raise.  The kernels' results
are pinned on the GPU (tests/test_gpu_user_planes.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lqr-obstacles_amd", "csrc")
PKG = os.path.join(ROOT, "lqr-obstacles_amd")


def test_plan_with_extra_planes(tmp_path):
    """C3's steady step (tests/cpp/lqro_plan_extra_main.cpp): without extras
    the early LP runs and k_qhull's jobs close their rows' LP; with a 6-face
    fence the early LP stays (1029 x 32 B fits) and the closing job leaves the
    row to the tail; with 4100 extras 5123 x 32 B = 163,936 B exceeds
    lp_lds_max = 163,840 B: no early LP."""
    exe = str(tmp_path / "plan_extra")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "lqro_plan_extra_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "0", "6", "4100", "4097", "4096"], capture_output=True, text=True, check=True)
    assert r.stdout.splitlines() == ["extra=0 early=1 row_lp=1", "extra=6 early=1 row_lp=0", "extra=4100 early=0",
                                     "extra=4097 early=1 row_lp=0",     # 5120 x 32 B: the last that fits
                                     "extra=4096 early=1 row_lp=0"]


def build_fence_main(out_dir) -> str:
    exe = os.path.join(str(out_dir), "lqro_fence_main")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lqro_fence_main.cpp"), "-o", exe,
                    "-L" + PKG, "-llqro", "-Wl,-rpath," + PKG], check=True)
    return exe


def write_fence_input(path, x, vg, H, NP, steps, lo, hi, tau, plane_lists):
    N = x.shape[0]
    offs = np.zeros(N + 1, np.int64)
    for i, p in enumerate(plane_lists):
        offs[i + 1] = offs[i] + len(p)
    with open(path, "wb") as f:
        np.array([N, H, NP, steps], np.int32).tofile(f)
        np.ascontiguousarray(x, np.float64).tofile(f)
        np.ascontiguousarray(vg, np.float64).tofile(f)
        np.array(list(lo) + list(hi) + [tau], np.float64).tofile(f)
        offs.tofile(f)
        for p in plane_lists:
            np.ascontiguousarray(p, np.float32).tofile(f)


def test_cpp_fence_consumer_links_and_fails_loudly_without_gpu(lqro_mod, tmp_path):
    """Simulator::setFence / setUserPlanes compile with plain g++ against
    liblqro.so; without a device the program fails with LQRO_E_NODEVICE."""
    import torch
    exe = build_fence_main(tmp_path)
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    write_fence_input(tmp_path / "in.bin", np.zeros((4, 16)), np.zeros((4, 3)), 10, 20, 1, [-5] * 3, [5] * 3, 2.0,
                      [np.zeros((k % 2, 6), np.float32) for k in range(4)])
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


@pytest.mark.parametrize("exc", ["QhullMergeSuspect", "HullFailure"])
def test_simulator_step_stores_newv_before_reraising(lqro_mod, exc):
    """LQRO_E_QHMERGE and LQRO_E_HULL steps complete and write newV:
    Simulator.step stores it in qlist, then raises (as lqro::Simulator::step
    does).  The context is a stand-in here; the GPU suite drives a real
    raising step."""
    nv = np.arange(12, dtype=np.float64).reshape(4, 3) + 0.5

    class Ctx:
        def step(self, x, vg):
            assert x.shape == (4, 16) and vg.shape == (4, 3)
            raise getattr(lqro_mod, exc)("raised", np.zeros((1, 2), np.int64), nv)

    sim = lqro_mod.Simulator.__new__(lqro_mod.Simulator)
    sim.qlist = [lqro_mod.Quadrotor(np.zeros(16)) for _ in range(4)]
    sim.ctx = Ctx()
    with pytest.raises(getattr(lqro_mod, exc)):
        sim.step()
    assert np.array_equal(np.stack([q.newV for q in sim.qlist]), nv)


def test_version_bumped(lqro_mod):
    assert lqro_mod.lib().lqro_version() >= 2
