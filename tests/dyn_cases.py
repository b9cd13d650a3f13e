"""Seeded agent states for the dynamics/estimation step tests (test data
only): positions, velocities, body rates and rotor forces around hover,
attitudes from random axis-angle rotations, covariances SPD around Pinit."""
from __future__ import annotations

import numpy as np

HOVER = 9.80665 * 0.5 / 4   # nominalInput (LQRO:188)


def rotation(axis_angle: np.ndarray) -> np.ndarray:
    th = float(np.linalg.norm(axis_angle))
    if th == 0.0:
        return np.eye(3)
    k = axis_angle / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def random_agent_cases(n: int, seed: int, rot_err: bool = True) -> dict:
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 16))
    x[:, 0:3] = rng.uniform(-3, 3, (n, 3))
    x[:, 3:6] = rng.uniform(-1, 1, (n, 3))
    if rot_err:   # nonzero only between a propagate and its reset; exercised anyway
        x[: n // 2, 6:9] = rng.uniform(-0.02, 0.02, (n // 2, 3))
    x[:, 9:12] = rng.uniform(-0.5, 0.5, (n, 3))
    x[:, 12:16] = HOVER + rng.uniform(-0.1, 0.1, (n, 4))
    rot = np.stack([rotation(rng.normal(size=3) * rng.uniform(0, 0.4)) for _ in range(n)])
    rot[0] = np.eye(3)   # the sinangle == 0 branch of both controllers
    B = rng.normal(size=(n, 16, 16))
    P = 1e-9 * np.eye(16) + 1e-10 * np.einsum("nij,nkj->nik", B, B)
    vgoal = rng.uniform(-1, 1, (n, 3))
    p_goal = rng.uniform(-3, 3, (n, 3))
    u_goal = np.full((n, 4), HOVER)
    z = np.concatenate([x[:, 9:12], x[:, 0:3]], axis=1) + 3e-5 * rng.normal(size=(n, 6))
    return dict(x=x, rot=rot, P=P, vgoal=vgoal, p_goal=p_goal, u_goal=u_goal, z=z)


def trajectory_start(n: int, seed: int) -> dict:
    """States as they stand at a step boundary (rotation error reset to 0)."""
    cs = random_agent_cases(n, seed, rot_err=False)
    return cs


def quat_cases() -> np.ndarray:
    """Rotations for quatFromRot: random ones, the identity, half turns about
    each axis and near-half turns (where 1 + trace terms reach 0 and the
    std::max(., 0) clamp and the sign tests matter)."""
    rng = np.random.default_rng(0x5154)
    rs = [rotation(rng.normal(size=3) * rng.uniform(0, 3.1)) for _ in range(40)]
    rs.append(np.eye(3))
    for ax in np.eye(3):
        rs.append(rotation(ax * np.pi))
        rs.append(rotation(ax * (np.pi - 1e-9)))
        rs.append(rotation(-ax * (np.pi - 1e-9)))
    rs.append(rotation(np.array([1.0, 1.0, 0.0]) / np.sqrt(2) * np.pi))
    return np.stack(rs)


# ---------------------------------------------------------------------------
# Hard cases for the dynamics step (tests/test_dyn_hard_cpu.py,
# tests/test_gpu_dyn_edges.py, tests/golden/make_golden_dyn.py): dense noise
# covariances, large attitudes, per-agent models.  Seeded; additions only.
# ---------------------------------------------------------------------------
MODEL_FIELDS = ("dt", "gravity", "mass", "inertia", "moment_const", "thrust_latency", "length",
                "j_step", "qv", "qp", "r", "pos_weight")


def spd(n: int, scale: float, cond: float, rng) -> np.ndarray:
    """Q diag(scale * geomspace(1, cond, n)) Q^T with a random orthogonal Q, symmetrised."""
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = Q @ np.diag(scale * np.geomspace(1.0, cond, n)) @ Q.T
    return 0.5 * (A + A.T)


# A family whose seed misses the condition test
# (tests/test_dyn_hard_cpu.py::test_condition) draws from another one: its
# name and a salt go here (none so far), never a wider bound there.
SEED_SALT = {}

COV_FAMILIES = ("dense_N", "dense_small", "dense_mid", "dense_unit", "ties", "block_M", "asym_N")


def covariances(name: str):
    """(M 16x16, N 6x6, scale of P) of a covariance family."""
    rng = np.random.default_rng([0x434F56, COV_FAMILIES.index(name), SEED_SALT.get(name, 0)])
    I16, I6 = np.eye(16), np.eye(6)
    if name == "dense_N":        # jacobi<6> alone
        return 1e-9 * I16, spd(6, 1e-10, 1e3, rng), 1e-9
    if name == "dense_small":
        return spd(16, 1e-10, 1e3, rng), spd(6, 1e-10, 1e3, rng), 1e-9
    if name == "dense_mid":
        return spd(16, 1e-6, 1e2, rng), spd(6, 1e-5, 1e2, rng), 1e-6
    if name == "dense_unit":
        return spd(16, 1e-2, 1e2, rng), spd(6, 1e-2, 1e2, rng), 1e-2
    if name == "ties":           # every off-diagonal equal: the first strict maximum in scan order
        return 1e-9 * (I16 + 0.25 * np.ones((16, 16))), 1e-9 * (I6 + 0.5 * np.ones((6, 6))), 1e-9
    if name == "block_M":        # pivots whose scan finds nothing between rotations
        M = np.diag(np.concatenate([np.zeros(6), np.geomspace(1e-9, 1e-7, 10)]))
        M[:6, :6] = spd(6, 1e-8, 1e2, rng)
        return M, spd(6, 1e-7, 1e2, rng), 1e-9
    if name == "asym_N":         # jacobi reads the upper triangle only
        N = spd(6, 1e-8, 1e2, rng)
        N[np.tril_indices(6, -1)] *= 0.5
        return 1e-9 * I16, N, 1e-9
    raise KeyError(name)


STATE_FAMILIES = ("tilt_1.4", "tilt_2.6", "exact", "rot_err", "rates", "quat", "models")
HARD_FAMILIES = COV_FAMILIES + STATE_FAMILIES + tuple(s + "@dense_mid" for s in STATE_FAMILIES)


def _axis_rot(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64)
    return rotation(a / np.linalg.norm(a) * angle)


def exact_rotations() -> np.ndarray:
    """Pure yaws, quarter turns about x and y and their product (entries
    exactly 0 or +-1), the half turns diag(1,-1,-1) and diag(-1,-1,1)."""
    Rx = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    Ry = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    rs = [_axis_rot([0, 0, 1], a) for a in (0.3, -1.2, 2.0, np.pi / 2, 3.0)]
    rs[3] = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])   # the quarter yaw, exactly
    rs += [Rx, Ry, Rx @ Ry, Ry.T, np.diag([1.0, -1, -1]), np.diag([-1.0, -1, 1])]
    return np.stack(rs)


def model_variants(base: dict) -> list:
    """The nine (dt, thrust_latency) combinations; `base`: the default model's fields."""
    out = []
    for dt in (1.0 / 240, 1.0 / 30, 1.0 / 5):
        for lat in (5.0, 40.0, 200.0):
            out.append(dict(base, dt=dt, thrust_latency=lat))
    return out


def hard_case(name: str, n: int = 16) -> dict:
    """One family of HARD_FAMILIES: random_agent_cases' fields plus x_true,
    rot_true, the noise weights M, N, `nrm` (n x 22 standard normal draws) and
    `model_ix` (None, or per agent an index into model_variants())."""
    state, _, cov = name.partition("@")
    if state in COV_FAMILIES:
        state, cov = "", state
    rng = np.random.default_rng([0x48415244, HARD_FAMILIES.index(name), SEED_SALT.get(name, 0)])
    cs = random_agent_cases(n, int(rng.integers(1 << 30)), rot_err=False)
    cs["x_true"] = cs["x"].copy()
    cs["rot_true"] = cs["rot"].copy()
    cs["model_ix"] = None
    if cov:
        M, N, ps = covariances(cov)
    else:
        M, N, ps = 1e-9 * np.eye(16), 1e-9 * np.eye(6), 1e-9
    cs["M"], cs["N"] = M, N
    cs["P"] = cs["P"] * (ps / 1e-9)
    if state.startswith("tilt_"):
        ang = float(state[5:])
        cs["rot"] = np.stack([_axis_rot(rng.normal(size=3), ang) for _ in range(n)])
        cs["rot_true"] = np.stack([_axis_rot(rng.normal(size=3), ang) for _ in range(n)])
    elif state == "exact":
        ex = exact_rotations()
        cs["rot"] = ex[np.arange(n) % len(ex)].copy()
        cs["rot_true"] = ex[(np.arange(n) * 3 + 5) % len(ex)].copy()
    elif state == "rot_err":
        cs["x"][:, 6:9] = rng.uniform(-0.5, 0.5, (n, 3))
        cs["x_true"][:, 6:9] = rng.uniform(-0.5, 0.5, (n, 3))
    elif state == "rates":
        cs["x"][:, 9:12] = rng.uniform(-15, 15, (n, 3))
        cs["x_true"][:, 9:12] = cs["x"][:, 9:12]   # (the estimate tracks the truth: no 30 rad/s residual)
    elif state == "quat":
        q = quat_cases()[40:]
        cs["rot_true"] = q[np.arange(n) % len(q)].copy()
    elif state == "models":
        cs["model_ix"] = np.arange(n) % 9
    cs["z"] = np.concatenate([cs["x_true"][:, 9:12], cs["x_true"][:, 0:3]], axis=1) \
        + 3e-5 * rng.normal(size=(n, 6))
    cs["nrm"] = rng.standard_normal((n, 22))
    return cs
