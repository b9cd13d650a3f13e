"""Inputs shared by tests/test_lp_audit_cpu.py and tests/test_gpu_lp_audit.py."""
import numpy as np

import lp_cases

WAVE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 200)   # k_lp_audit streams 64 planes a pass
TOL = 0.00001                                          # RVO_EPSILON


def n_hard_options(m):
    """0, 1, m - 1, m and m + 5 (clamped by the audit), without negatives."""
    return sorted({0, 1, max(m - 1, 0), m, m + 5})


def wave_rows(seed=21):
    """One row per (size, n_hard option): planes from the lp_cases families in
    turn, a goal, an arbitrary velocity.  Returns (lists, goals, n_hard, vel)."""
    rng = np.random.default_rng(seed)
    lists, goals, nh, vel = [], [], [], []
    t = 0
    for m in WAVE_SIZES:
        for h in n_hard_options(m):
            fam = lp_cases.FAMILIES[t % len(lp_cases.FAMILIES)]
            c = lp_cases._FAMILY_FN[fam](rng, m, t).astype(np.float32).reshape(-1, 6)
            lists.append(c)
            goals.append(lp_cases._goal(rng, t, c))
            nh.append(h)
            vel.append(rng.normal(size=3) * (0.0, 1.0, 30.0, 1e-20)[t % 4])
            t += 1
    return lists, np.array(goals), np.array(nh, np.int32), np.array(vel)


def few_planes(n, seed=33):
    """n agents with 0 to 5 planes each (the total's reduction edges)."""
    rng = np.random.default_rng(seed)
    lists, _ = lp_cases.random_cases(n, seed=seed, max_planes=6)
    goals = rng.normal(size=(n, 3)) * 2.0
    vel = rng.normal(size=(n, 3))
    nh = rng.integers(0, 4, size=n).astype(np.int32)
    return lists, goals, nh, vel


V0 = np.array([0.25, -0.5, 1.0])                       # exact in fp32
HOT = np.array([2.0, 0.0, 0.0, 1.0, 0.0, 0.0], np.float32) + np.concatenate([V0, np.zeros(3)]).astype(np.float32)
# (normal (1, 0, 0) through V0 + (2, 0, 0): viol = 2 exactly at v = V0)


def _satisfied(m, seed):
    """m planes the velocity V0 satisfies with a margin of 50: viol = -50 or so."""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(m, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([V0 - 50.0 * nrm, nrm], 1).astype(np.float32)


def tie_rows():
    """{name: (planes, n_hard)} at the velocity V0; what each must give is in
    tests/test_lp_audit_cpu.py::test_tie_rules."""
    out = {}
    c = _satisfied(200, 1)
    c[[3, 67, 131]] = HOT                              # different passes, the same lane
    out["same_lane"] = (c, 0)
    c = _satisfied(40, 2)
    c[[5, 6]] = HOT                                    # neighbouring lanes
    out["neighbours"] = (c, 0)
    c = _satisfied(40, 3)
    c[[4, 5, 6]] = HOT                                 # the hard prefix ends between equal planes
    out["prefix_between"] = (c, 6)
    c = _satisfied(20, 4)
    v = V0.astype(np.float32)
    c[2] = np.concatenate([v, np.float32([-1.0, -1.0, -1.0])])   # through v: every term -0, viol = -0
    c[9] = np.concatenate([v, np.float32([1.0, 0.0, 0.0])])      # through v: viol = +0
    out["signed_zero"] = (c, 20)
    return out


def equal_rows():
    """Four rows at V0; rows 1 and 3 share their list, so their viol_max is
    equal and the total names row 1; row 0's is lower, row 2 is empty."""
    low = _satisfied(12, 5)
    low[7] = HOT
    low[7, 0] -= np.float32(1.0)                       # viol = 1
    c = _satisfied(70, 6)
    c[66] = HOT
    lists = [low, c, np.zeros((0, 6), np.float32), c.copy()]
    return lists, np.zeros((4, 3)), np.array([12, 0, 0, 70], np.int32), np.tile(V0, (4, 1))


def opposing():
    """Two opposing planes: v.x >= 1 and v.x <= -1."""
    return np.array([[1, 0, 0, 1, 0, 0], [-1, 0, 0, -1, 0, 0]], np.float32)
