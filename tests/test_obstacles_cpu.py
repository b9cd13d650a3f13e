"""Obstacles (lqro_set_obstacles[_device]) on the CPU: the exported symbols,
the C++ host's call, lqro.obstacle_states' layout, and what the step's
planner does with columns that are no rows.  The kernels' results are pinned
on the GPU (tests/test_gpu_obstacles.py)."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "lqr-obstacles_amd", "csrc")
PKG = os.path.join(ROOT, "lqr-obstacles_amd")


def test_symbols_exported(lqro_mod):
    assert "lqro_set_obstacles" in lqro_mod.EXPORTS and "lqro_set_obstacles_device" in lqro_mod.EXPORTS
    L = ctypes.CDLL(lqro_mod.LIB_PATH)
    for sym in ("lqro_set_obstacles", "lqro_set_obstacles_device"):
        assert getattr(L, sym) is not None
    hdr = open(os.path.join(ROOT, "include", "lqro.h")).read()
    for sym in ("int lqro_set_obstacles(", "int lqro_set_obstacles_device("):
        assert sym in hdr
    # a null context is refused before any device call
    lib = lqro_mod.lib()
    assert lib.lqro_set_obstacles(None, None, 0, 0.0, 0.0, 1.0) == -1
    assert lib.lqro_set_obstacles_device(None, None, 0, 0.0, 0.0, 1.0) == -1
    assert lib.lqro_version() >= 3


def build_obstacles_main(out_dir) -> str:
    exe = os.path.join(str(out_dir), "lqro_obstacles_main")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lqro_obstacles_main.cpp"), "-o", exe,
                    "-L" + PKG, "-llqro", "-Wl,-rpath," + PKG], check=True)
    return exe


def write_obstacles_input(path, x, vg, H, NP, steps, obs, radii, resp):
    with open(path, "wb") as f:
        np.array([x.shape[0], H, NP, steps, obs.shape[0]], np.int32).tofile(f)
        np.ascontiguousarray(x, np.float64).tofile(f)
        np.ascontiguousarray(vg, np.float64).tofile(f)
        np.ascontiguousarray(obs, np.float64).tofile(f)
        np.array([radii[0], radii[1], resp], np.float64).tofile(f)


def test_cpp_obstacles_consumer_links_and_fails_loudly_without_gpu(lqro_mod, tmp_path):
    """Simulator::setObstacles compiles with plain g++ against liblqro.so;
    without a device the program fails with LQRO_E_NODEVICE."""
    import torch
    exe = build_obstacles_main(tmp_path)
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    write_obstacles_input(tmp_path / "in.bin", np.zeros((4, 16)), np.zeros((4, 3)), 10, 20, 1,
                          lqro_mod.obstacle_states(np.ones((2, 3))), (0.26, 0.75), 1.0)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


def test_obstacle_states_layout(lqro_mod):
    pos = np.array([[1.0, 2.0, 3.0], [-4.0, 5.5, 0.25]])
    vel = np.array([[0.5, -0.25, 0.125], [0.0, 0.0, -1.0]])
    nominal = 9.80665 * 0.500 / 4
    s = lqro_mod.obstacle_states(pos, vel)
    assert s.shape == (2, 16) and s.dtype == np.float64 and s.flags.c_contiguous
    assert np.array_equal(s[:, 0:3], pos) and np.array_equal(s[:, 3:6], vel)
    assert not s[:, 6:12].any() and np.array_equal(s[:, 12:16], np.full((2, 4), nominal))
    # what synthetic_swarm gives an agent, apart from the draws
    x, _ = lqro_mod.synthetic_swarm(2)
    assert np.array_equal(lqro_mod.obstacle_states(x[:, 0:3], x[:, 3:6]), x)
    s = lqro_mod.obstacle_states(pos)                    # static
    assert not s[:, 3:12].any() and np.array_equal(s[:, 12:16], np.full((2, 4), nominal))
    s = lqro_mod.obstacle_states(pos, vel, x_dim=12)     # the reduced model has no rotor-force states
    assert s.shape == (2, 12) and np.array_equal(s[:, 0:3], pos) and np.array_equal(s[:, 3:6], vel)
    assert not s[:, 6:].any()
    x12, _ = lqro_mod.synthetic_swarm(2, x_dim=12)
    assert np.array_equal(lqro_mod.obstacle_states(x12[:, 0:3], x12[:, 3:6], x_dim=12), x12)
    assert lqro_mod.obstacle_states([1.0, 2.0, 3.0]).shape == (1, 16)


def test_plan_with_obstacle_columns(tmp_path):
    """tests/cpp/lqro_plan_obs_main.cpp: 1024 rows in C3's steady state whose
    rows have npr agent columns and m obstacle columns.  The slots follow
    npr + m, and the early LP's decisions move at the same byte borders as for
    extra planes: (npr + m + extra) x 32 B against lp_lds_max = 163,840 B
    (5120 planes), and row_lp at LQRO_EARLY_LP_MAX_NPR = 1024 slots."""
    exe = str(tmp_path / "plan_obs")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "lqro_plan_obs_main.cpp"), "-o", exe], check=True)
    args = ["1023:0:0", "1023:1:0", "1023:2:0", "1023:1:6", "1023:4097:0", "1023:4098:0", "1023:4091:6",
            "1023:4092:6", "959:64:0", "1023:64:0"]
    r = subprocess.run([exe] + args, capture_output=True, text=True, check=True)

    def line(npr, m, extra, early, row_lp):
        return (f"npr={npr} m={m} extra={extra} slots_per_row={npr + m} slots={1024 * (npr + m)} "
                f"early={early} row_lp={row_lp}")

    assert r.stdout.splitlines() == [
        line(1023, 0, 0, 1, 1),          # C3 as it is
        line(1023, 1, 0, 1, 1),          # 1024 slots: the last row length the closing job's LP holds
        line(1023, 2, 0, 1, 0),          # 1025: left to the tail
        line(1023, 1, 6, 1, 0),          # extras: the tail, as without obstacles
        line(1023, 4097, 0, 1, 0),       # 5120 x 32 B: the last that fits
        line(1023, 4098, 0, 0, 0),       # 5121 x 32 B = 163,872 B: no early LP
        line(1023, 4091, 6, 1, 0),       # (5114 + 6) x 32 B fits
        line(1023, 4092, 6, 0, 0),       # (5115 + 6) x 32 B does not
        line(959, 64, 0, 1, 1),          # 1023 slots, 64 of them obstacles: the plan of 1023 agent columns
        line(1023, 64, 0, 1, 0),
    ]
