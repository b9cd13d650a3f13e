"""Hard planes (lqro_set_hard_planes, lqro_calculate_new_v_hard) on the CPU:
the numpy restatement of the LP that the GPU tests take their expected values
from (tests/lp_hard_ref.py) against the oracle, the rule's properties on that
restatement, the exported symbols, the C++ host's call and the step planner.
The kernels' results are pinned on the GPU (tests/test_gpu_hard_planes.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lp_cases
import lp_hard_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "lqr-obstacles_amd", "csrc")
PKG = os.path.join(ROOT, "lqr-obstacles_amd")


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def anchor_rows():
    """random_cases seeds 1 and 2 (at most 60 and 200 planes) and every row of
    lp_cases.fixture_rows(), the subnormal family included: 340 rows."""
    rows = []
    for seed, mx in ((1, 60), (2, 200)):
        c, g = lp_cases.random_cases(60, seed, mx)
        rows += list(zip(c, g))
    c, g, _ = lp_cases.fixture_rows()
    return rows + list(zip(c, g))


# ---------------------------------------------------------------------------
# the anchor: with n_hard = 0 the restatement is the oracle's LP, bit for bit
# ---------------------------------------------------------------------------
def test_checker_equals_oracle_without_hard_planes(oracle):
    rows = anchor_rows()
    assert len(rows) == 340
    ran_lp4 = 0
    for k, (c, g) in enumerate(rows):
        info = {}
        got = ref.new_v(c, g, info=info)
        ran_lp4 += info["fail"] < info["m"]
        assert np.array_equal(bits(got), bits(oracle.newv(c, g))), (k, len(c))
    assert ran_lp4 >= 30   # linearProgram4 is part of what was compared


@pytest.mark.parametrize("m", lp_cases.LONG_SIZES)
def test_checker_equals_oracle_on_long_rows(oracle, m):
    c, g = lp_cases.long_row(m, 77)
    soft = ref.new_v(c, g)
    assert np.array_equal(bits(soft), bits(oracle.newv(c, g)))
    # what tests/test_gpu_hard_planes.py relies on for these rows: a hard
    # prefix that reaches into the infeasible family changes the result, one
    # of far feasible planes alone does not
    assert not np.array_equal(bits(ref.new_v(c, g, n_hard=m - 100)), bits(soft))
    assert not np.array_equal(bits(ref.new_v(c, g, n_hard=m)), bits(soft))
    assert np.array_equal(bits(ref.new_v(c, g, n_hard=65)), bits(soft))


# ---------------------------------------------------------------------------
# the rule's properties, on the restatement
# ---------------------------------------------------------------------------
def small_rows():
    """The anchor rows of at most 129 planes (random and edge rows)."""
    return [(c, g) for c, g in anchor_rows() if len(c) <= 129]


def test_rows_without_lp4_ignore_n_hard_and_the_others_do_not():
    changed_half = changed_one = with_lp4 = 0
    for c, g in small_rows():
        m = len(c)
        info = {}
        soft = ref.new_v(c, g, info=info)
        half = ref.new_v(c, g, n_hard=m // 2)
        if info["fail"] == m:   # linearProgram3 did not fail: linearProgram4 never runs
            for nh in (1, m // 2, m, m + 5):
                assert np.array_equal(bits(ref.new_v(c, g, n_hard=nh)), bits(soft))
            continue
        with_lp4 += 1
        changed_half += not np.array_equal(bits(half), bits(soft))
        changed_one += not np.array_equal(bits(ref.new_v(c, g, n_hard=1)), bits(soft))
    # the rule is live on these rows: hard prefixes change results where linearProgram4 runs
    assert with_lp4 >= 30 and changed_half >= with_lp4 // 2 and changed_one >= 1


def test_all_hard_projects_nothing():
    """n_hard >= m: every violated plane's projected list is the raw list
    (all m planes, plane i included, as RVO2 copies its obstacle lines)."""
    seen = 0
    for c, g in small_rows()[::3]:
        for nh in (len(c), len(c) + 5):
            trace = []
            ref.new_v(c, g, n_hard=nh, trace=trace)
            for i, proj in trace:
                assert np.array_equal(proj.T.view(np.uint32), np.asarray(c, np.float32).view(np.uint32)), i
                seen += 1
    assert seen >= 10


def test_prefix_is_copied_and_the_rest_projected():
    """0 < n_hard < i: the list starts with planes [0, n_hard) as they are,
    and what follows is the tail of the soft list's projections (the
    projections of planes n_hard .. i-1 do not depend on n_hard)."""
    seen = 0
    for c, g in small_rows()[::3]:
        m = len(c)
        if m < 4:
            continue
        nh = m // 2
        trace = []
        ref.new_v(c, g, n_hard=nh, trace=trace)
        cc = np.ascontiguousarray(np.asarray(c, np.float32).T)
        for i, proj in trace:
            assert np.array_equal(proj[:, :nh].view(np.uint32), cc[:, :nh].view(np.uint32))
            with np.errstate(all="ignore"):
                tail = ref.projected(cc, 0, i)
            ntail = proj.shape[1] - nh
            assert 0 <= ntail <= max(i - nh, 0)
            if ntail:
                assert np.array_equal(proj[:, nh:].view(np.uint32), tail[:, tail.shape[1] - ntail:].view(np.uint32))
                seen += 1
    assert seen >= 10


# The floor and the boxes.  A face's violation by v is normal.(point - v): how
# far outside the face v lies (<= 0: inside).
FLOOR = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0]], np.float32)   # v_z >= 0
BOX_SEED = 20261020
# The worst violation of a hard face over the floor rows and the 40 boxes
# below, measured from tests/lp_hard_ref.py on these very inputs, is
# HARD_WORST_MEASURED; the quantity is the rounding of a point placed on a
# plane (coordinates of order 1 to 100 in float32), so 8 x that is allowed.
HARD_WORST_MEASURED = 5.960464477539062e-07
HARD_BOUND = 8 * HARD_WORST_MEASURED


def crowd_down(rng, k):
    """k planes of a crowd above pushing down: normals within ~0.1 rad of -z,
    each asking for v_z <~ -d with d in [1.8, 2.3]."""
    n = np.concatenate([rng.normal(size=(k, 2)) * 0.05, -np.ones((k, 1))], 1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.uniform(1.8, 2.3, size=(k, 1))
    return np.concatenate([d * n, n], 1).astype(np.float32)


def box_case(rng):
    """A six-face box around the origin (faces at 0.5 .. 2 from it, in the
    fence's order: axis x, y, z, lower face then upper) and 5 to 40 crowd
    planes that each ask for a velocity 3 to 6 out along directions spread
    around one random direction (a crowd pushing from one side): box and
    crowd are infeasible together."""
    lo, hi = -rng.uniform(0.5, 2.0, 3), rng.uniform(0.5, 2.0, 3)
    faces = np.zeros((6, 6), np.float32)
    for a in range(3):
        faces[2 * a, a], faces[2 * a, 3 + a] = lo[a], 1.0
        faces[2 * a + 1, a], faces[2 * a + 1, 3 + a] = hi[a], -1.0
    k = int(rng.integers(5, 41))
    u = rng.normal(size=3)
    n = u / np.linalg.norm(u) + 0.35 * rng.normal(size=(k, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    crowd = np.concatenate([rng.uniform(3.0, 6.0, size=(k, 1)) * n, n], 1).astype(np.float32)
    return np.concatenate([faces, crowd]), rng.normal(size=3) * 2.0


def violation(faces, v):
    f = np.asarray(faces, np.float64)
    return float(np.max(((f[:, :3] - v) * f[:, 3:]).sum(1)))


def test_floor_holds_under_a_crowd():
    rng = np.random.default_rng(BOX_SEED)
    for k in (8, 16, 24, 40):
        c = np.concatenate([FLOOR, crowd_down(rng, k)])
        g = np.array([0.3, -0.2, 0.1])
        soft, hard = ref.new_v(c, g), ref.new_v(c, g, n_hard=1)
        print(f"floor, {k} crowd planes: soft v_z = {soft[2]!r}, hard v_z = {hard[2]!r}")
        # the soft LP splits the difference between the floor and the crowd's -d (d >= 1.8)
        assert soft[2] < -0.5
        assert hard[2] == 0.0


def test_boxes_hold_under_a_crowd():
    rng = np.random.default_rng(BOX_SEED + 1)
    soft_out, worst = 0, 0.0
    for _ in range(40):
        c, g = box_case(rng)
        soft, hard = ref.new_v(c, g), ref.new_v(c, g, n_hard=6)
        soft_out += violation(c[:6], soft) > 1e-3
        worst = max(worst, violation(c[:6], hard))
    print(f"boxes: soft LP left the box by > 1e-3 in {soft_out} of 40; hard LP's worst violation {worst!r}")
    assert soft_out >= 20
    assert worst <= HARD_BOUND


# ---------------------------------------------------------------------------
# ABI, hosts, planner
# ---------------------------------------------------------------------------
def test_symbols_exported(lqro_mod):
    for sym in ("lqro_set_hard_planes", "lqro_calculate_new_v_hard"):
        assert sym in lqro_mod.EXPORTS
    L = ctypes.CDLL(lqro_mod.LIB_PATH)
    for sym in ("lqro_set_hard_planes", "lqro_calculate_new_v_hard"):
        assert getattr(L, sym) is not None
    hdr = open(os.path.join(ROOT, "include", "lqro.h")).read()
    for text in ("int lqro_set_hard_planes(", "int lqro_calculate_new_v_hard(", "#define LQRO_HARD_NONE      0",
                 "#define LQRO_HARD_FENCE     1", "#define LQRO_HARD_HEAD      2", "#define LQRO_HARD_OBSTACLES 3"):
        assert text in hdr
    assert (lqro_mod.LQRO_HARD_NONE, lqro_mod.LQRO_HARD_FENCE, lqro_mod.LQRO_HARD_HEAD,
            lqro_mod.LQRO_HARD_OBSTACLES) == (0, 1, 2, 3)
    lib = lqro_mod.lib()
    assert lib.lqro_version() >= 4
    # refused before any device call: a null context, and a negative n_hard
    assert lib.lqro_set_hard_planes(None, 1) == -1
    planes = np.zeros((2, 6), np.float32)
    offs = np.array([0, 1, 2], np.int64)
    nh = np.array([0, -1], np.int32)
    vg, out = np.zeros((2, 3)), np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert lib.lqro_calculate_new_v_hard(p(planes), p(offs), p(nh), 2, p(vg), 100.0, p(out), 0) == -1
    for s in (lqro_mod.Context, lqro_mod.Simulator, lqro_mod.DeviceLoop):
        assert callable(getattr(s, "set_hard_planes"))


def build_hard_main(out_dir) -> str:
    exe = os.path.join(str(out_dir), "lqro_hard_main")
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lqro_hard_main.cpp"), "-o", exe,
                    "-L" + PKG, "-llqro", "-Wl,-rpath," + PKG], check=True)
    return exe


def write_hard_input(path, x, vg, H, NP, steps, level, lo, hi, tau, obs, radii, resp, plane_lists):
    N = x.shape[0]
    offs = np.zeros(N + 1, np.int64)
    for i, p in enumerate(plane_lists):
        offs[i + 1] = offs[i] + len(p)
    with open(path, "wb") as f:
        np.array([N, H, NP, steps, obs.shape[0], level], np.int32).tofile(f)
        np.ascontiguousarray(x, np.float64).tofile(f)
        np.ascontiguousarray(vg, np.float64).tofile(f)
        np.array(list(lo) + list(hi) + [tau], np.float64).tofile(f)
        np.ascontiguousarray(obs, np.float64).tofile(f)
        np.array([radii[0], radii[1], resp], np.float64).tofile(f)
        offs.tofile(f)
        for p in plane_lists:
            np.ascontiguousarray(p, np.float32).tofile(f)


def test_cpp_hard_consumer_links_and_fails_loudly_without_gpu(lqro_mod, tmp_path):
    """Simulator::setHardPlanes compiles with plain g++ against liblqro.so;
    without a device the program fails with LQRO_E_NODEVICE."""
    import torch
    exe = build_hard_main(tmp_path)
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    write_hard_input(tmp_path / "in.bin", np.zeros((4, 16)), np.zeros((4, 3)), 10, 20, 1, 3, [-5] * 3, [5] * 3, 2.0,
                     lqro_mod.obstacle_states(np.ones((2, 3))), (0.26, 0.75), 1.0,
                     [np.zeros((k % 2, 6), np.float32) for k in range(4)])
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


SHARDED_HARD = os.path.join(ROOT, "tests", "cpp", "lqro_sharded_hard_main")


def sharded_hard_main() -> str:
    """tests/cpp/lqro_sharded_hard_main (hipcc and RCCL: __graft_entry__.build makes it)."""
    if not os.path.exists(SHARDED_HARD):
        import __graft_entry__ as ge
        ge.build_cpp_sharded_hard()
    return SHARDED_HARD


def write_sharded_hard_input(path, x, vg, pg, H, NP, steps, seed, level, lo, hi, tau, obs, radii, resp):
    with open(path, "wb") as f:
        np.array([x.shape[0], H, NP, steps, obs.shape[0], level], np.int32).tofile(f)
        np.array([seed], np.uint32).tofile(f)
        for a in (x, vg, pg):
            np.ascontiguousarray(a, np.float64).tofile(f)
        np.array(list(lo) + list(hi) + [tau], np.float64).tofile(f)
        np.ascontiguousarray(obs, np.float64).tofile(f)
        np.array([radii[0], radii[1], resp], np.float64).tofile(f)


def test_cpp_sharded_hard_consumer_links_and_fails_loudly_without_gpu(lqro_mod, tmp_path):
    """ShardedSimulator::setHardPlanes compiles against liblqro.so and RCCL;
    without a device the program fails with LQRO_E_NODEVICE before RCCL is
    touched."""
    import torch
    exe = sharded_hard_main()
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    write_sharded_hard_input(tmp_path / "in.bin", np.zeros((4, 16)), np.zeros((4, 3)), np.zeros((4, 3)), 10, 20, 1, 1,
                             3, [-5] * 3, [5] * 3, 2.0, lqro_mod.obstacle_states(np.ones((2, 3))), (0.26, 0.75), 1.0)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


def test_plan_with_hard_obstacles(tmp_path):
    """tests/cpp/lqro_plan_hard_main.cpp: C3's steady step.  At level 3 with
    obstacles the k_qhull job that closes a row leaves its LP to the tail
    (row_lp = 0: the in-job LP compacts in slot order), the early LP launch
    stays; levels 0-2, and level 3 without obstacles, plan as before."""
    exe = str(tmp_path / "plan_hard")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "lqro_plan_hard_main.cpp"), "-o", exe], check=True)
    args = ["1023:0:0:0", "1023:0:0:1", "1023:0:0:2", "1023:0:0:3", "1019:4:0:0", "1019:4:0:1", "1019:4:0:2",
            "1019:4:0:3", "1019:4:6:3", "1023:0:6:1"]
    r = subprocess.run([exe] + args, capture_output=True, text=True, check=True)

    def line(npr, m, extra, level, early, row_lp):
        return f"npr={npr} m={m} extra={extra} level={level} early={early} row_lp={row_lp}"

    assert r.stdout.splitlines() == [
        line(1023, 0, 0, 0, 1, 1), line(1023, 0, 0, 1, 1, 1), line(1023, 0, 0, 2, 1, 1),
        line(1023, 0, 0, 3, 1, 1),       # level 3 with no obstacle: nothing to reorder
        line(1019, 4, 0, 0, 1, 1), line(1019, 4, 0, 1, 1, 1), line(1019, 4, 0, 2, 1, 1),
        line(1019, 4, 0, 3, 1, 0),       # obstacle slots first: the tail's LP
        line(1019, 4, 6, 3, 1, 0),
        line(1023, 0, 6, 1, 1, 0),       # extras alone already leave the row to the tail
    ]
