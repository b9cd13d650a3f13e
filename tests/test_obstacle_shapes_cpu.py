"""Obstacles with a shape and a responsibility each (lqro_set_obstacles_ex
[_device]) on the CPU: k_pair's LDS layout as a host function
(lqro_plan.hpp pair_layout, tests/cpp/lqro_plan_shapes_main.cpp), the exported
symbols and the version, and the Python wrapper's argument handling.  The
kernels' results are pinned on the GPU (tests/test_gpu_obstacle_shapes.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lqr-obstacles_amd", "csrc")
BUDGET = 160 * 1024 // 8          # k_pair's LDS, in doubles
C1, C3, BIG = (50, 100, 16), (100, 100, 16), (256, 100, 16)   # (H, NP, X)


def build_plan_shapes(out_dir, sanitize=False) -> str:
    exe = os.path.join(str(out_dir), "plan_shapes" + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "lqro_plan_shapes_main.cpp"), "-o", exe], check=True)
    return exe


def pair_layouts(exe, cases):
    """[{field: int}] of the layout program's lines for (H, NP, X, K) cases."""
    r = subprocess.run([exe] + [":".join(str(v) for v in c) for c in cases], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    out = [{k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)} for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def max_classes(exe, H, NP, X):
    """The largest K for which a wave keeps its LDS region (-1: none, not even K = 0)."""
    ok = [L["ok"] for L in pair_layouts(exe, [(H, NP, X, k) for k in range(0, 40)])]
    assert ok == sorted(ok, reverse=True)
    return sum(ok) - 1


def parent_layout(H, NP, X, own_shape):
    """The layout arithmetic as it stood before the shape classes (one
    optional S_o, Ro_o behind the slice hashes), restated."""
    XP, PW = X + 1, (NP + 63) // 64
    off = {}
    o = 0
    for name, size in (("T", 9 * H), ("N", 3 * H * XP), ("S", 3 * NP), ("R", H), ("TF", H), ("Hh", H)):
        off[name] = o
        o += size
    off["So"] = o
    if own_shape:
        o += 3 * NP + H
    off["wave"] = o
    wd = 4 * H + H * PW + H + (H + (H & 1)) // 2 + 18 + 5
    waves = min(16, (BUDGET - o) // wd)
    return off, wd, waves, (o + waves * wd) * 8


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return build_plan_shapes(tmp_path_factory.mktemp("plan_shapes"))


@pytest.mark.parametrize("shape,waves", [(C1, 16), (C3, 16), (BIG, 2)])
def test_no_class_is_the_layout_a_context_is_created_with(plan_exe, shape, waves):
    H, NP, X = shape
    L = pair_layouts(plan_exe, [(H, NP, X, 0)])[0]
    off, wd, w, nbytes = parent_layout(H, NP, X, False)
    assert w == waves
    assert L["ok"] == 1 and L["waves"] == waves and L["wave_doubles"] == wd and L["bytes"] == nbytes
    assert [L[k] for k in ("T", "N", "S", "R", "TF", "Hh", "wave")] == [off[k] for k in ("T", "N", "S", "R", "TF", "Hh", "wave")]
    assert L["cls"] == L["wave"]          # no class block
    if shape == C3:
        assert (L["wave"], wd, nbytes) == (6600, 773, 151744)
    if shape == BIG:
        assert (L["wave"], wd) == (16428, 1943)


def test_one_class_is_the_own_shape_layout(plan_exe):
    """S_c and Ro_c where S_o and Ro_o were; the four scalars behind them
    move the wave regions by 4 doubles and leave C3's 16 waves."""
    H, NP, X = C3
    L = pair_layouts(plan_exe, [(H, NP, X, 1)])[0]
    off, wd, w, nbytes = parent_layout(H, NP, X, True)
    assert w == 16 and L["waves"] == 16 and L["ok"] == 1
    assert L["cls"] == off["So"] and L["cls_doubles"] == 3 * NP + H + 4
    assert L["wave"] == off["wave"] + 4 and L["bytes"] == nbytes + 32


def test_class_blocks_and_waves_at_c3(plan_exe):
    """3 classes keep C3's 16 waves, the 4th costs one, LQRO_OBS_SHAPES_MAX leaves 13."""
    H, NP, X = C3
    Ls = pair_layouts(plan_exe, [(H, NP, X, k) for k in range(0, 9)])
    assert [L["waves"] for L in Ls] == [16, 16, 16, 16, 15, 15, 14, 14, 13]
    for k, L in enumerate(Ls):
        assert L["wave"] == 6600 + 404 * k and L["ok"] == 1
        assert L["bytes"] == (L["wave"] + L["waves"] * 773) * 8 <= BUDGET * 8


def test_border_where_no_wave_is_left(plan_exe):
    """H = 256: 16,428 doubles of block tables and 1,943 a wave in 20,480: 3
    classes of 560 doubles leave one wave, the 4th none."""
    H, NP, X = BIG
    assert max_classes(plan_exe, H, NP, X) == 3
    Ls = pair_layouts(plan_exe, [(H, NP, X, k) for k in (2, 3, 4, 8, 39)])
    assert [(L["ok"], L["waves"]) for L in Ls[:3]] == [(1, 1), (1, 1), (0, 0)]
    assert Ls[3]["ok"] == 0 and Ls[4]["ok"] == 0 and Ls[4]["waves"] == 0   # (past the budget: no negative count)
    assert Ls[1]["wave"] == 16428 + 3 * 560
    # a horizon whose tables alone leave no wave
    assert max_classes(plan_exe, 300, 100, 16) == -1


def test_layout_program_under_sanitizers(tmp_path):
    """The same program as a host binary under ASan and UBSan: same lines, no report."""
    exe = build_plan_shapes(tmp_path)
    san = build_plan_shapes(tmp_path, sanitize=True)
    cases = [(50, 100, 16, 0), (100, 100, 16, 3), (100, 100, 12, 8), (256, 100, 16, 4), (4096, 256, 16, 8), (1, 1, 12, 0)]
    args = [":".join(str(v) for v in c) for c in cases]
    a = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    b = subprocess.run([san] + args, capture_output=True, text=True, timeout=60)
    assert a.returncode == 0 and b.returncode == 0, b.stderr
    assert a.stdout == b.stdout and b.stderr == ""


def test_exports_version_and_header(lqro_mod):
    names = ("lqro_set_obstacles_ex", "lqro_set_obstacles_ex_device")
    L = ctypes.CDLL(lqro_mod.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "lqro.h")).read()
    for sym in names:
        assert sym in lqro_mod.EXPORTS and getattr(L, sym) is not None
        m = re.search(r"int " + sym + r"\((.*?)\);", hdr, re.S)
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert [" ".join(a.split()) for a in args] == [
            "lqro_ctx* ctx", "const double* d_states" if sym.endswith("_device") else "const double* states",
            "int32_t n_obstacles", "const double* xy_radius", "const double* z_radius",
            "const double* responsibility"], sym
    assert "#define LQRO_OBS_SHAPES_MAX 8" in hdr and lqro_mod.LQRO_OBS_SHAPES_MAX == 8
    lib = lqro_mod.lib()
    assert lib.lqro_version() == 5
    # a null context is refused before any device call
    assert lib.lqro_set_obstacles_ex(None, None, 0, None, None, None) == -1
    assert lib.lqro_set_obstacles_ex_device(None, None, 0, None, None, None) == -1


SHAPES_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_shapes_main")


def shapes_main() -> str:
    """tests/cpp/lqro_shapes_main (hipcc and RCCL: __graft_entry__.build makes it)."""
    if not os.path.exists(SHAPES_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_shapes()
    return SHAPES_MAIN


def write_shapes_input(path, x, vg, pg, H, NP, steps, seed, obs, radii, resp):
    with open(path, "wb") as f:
        np.array([x.shape[0], H, NP, steps, obs.shape[0]], np.int32).tofile(f)
        np.array([seed], np.uint32).tofile(f)
        for a in (x, vg, pg, obs, [r[0] for r in radii], [r[1] for r in radii], resp):
            np.ascontiguousarray(a, np.float64).tofile(f)


def test_cpp_hosts_link_and_fail_loudly_without_gpu(lqro_mod, tmp_path):
    """The std::vector overloads of Simulator::setObstacles and
    ShardedSimulator::setObstacles compile against liblqro.so and RCCL;
    without a device the program fails with LQRO_E_NODEVICE before RCCL is
    touched."""
    import torch
    exe = shapes_main()
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    write_shapes_input(tmp_path / "in.bin", np.zeros((4, 16)), np.zeros((4, 3)), np.zeros((4, 3)), 10, 20, 1, 1,
                       lqro_mod.obstacle_states(np.ones((2, 3))), [(0.26, 0.75), (1.0, 1.0)], [1.0, 0.5])
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


def test_wrapper_arguments(lqro_mod):
    f = lqro_mod.obstacle_arrays
    # scalars and None: the one-shape call, defaults the agents' radii and 1.0
    assert f(3, None, None, 1.0, 0.26, 0.75) == (False, 0.26, 0.75, 1.0)
    assert f(3, 0.5, 0.25, 0.5, 0.26, 0.75) == (False, 0.5, 0.25, 0.5)
    assert f(3, np.float64(0.5), 1, None, 0.26, 0.75) == (False, 0.5, 1.0, 1.0)
    # any sequence: three float64 arrays of M, the scalars broadcast
    per, oxy, oz, resp = f(3, [0.0, 0.5, 1.0], None, 0.5, 0.26, 0.75)
    assert per is True
    for a, want in ((oxy, [0.0, 0.5, 1.0]), (oz, [0.75] * 3), (resp, [0.5] * 3)):
        assert a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (3,) and a.tolist() == want
    per, oxy, oz, resp = f(2, 0.5, (0.25, 1.0), np.array([1.0, 0.25], np.float32), 0.26, 0.75)
    assert per and oxy.tolist() == [0.5, 0.5] and oz.tolist() == [0.25, 1.0] and resp.tolist() == [1.0, 0.25]
    # a length that is not M, or not a vector
    for bad in (dict(xy_radius=[0.5, 0.5]), dict(z_radius=[0.5] * 4), dict(responsibility=[1.0]),
                dict(responsibility=[[1.0, 1.0, 1.0]]), dict(xy_radius=[])):
        kw = dict(xy_radius=None, z_radius=None, responsibility=1.0)
        kw.update(bad)
        with pytest.raises(lqro_mod.LqroError):
            f(3, kw["xy_radius"], kw["z_radius"], kw["responsibility"], 0.26, 0.75)
