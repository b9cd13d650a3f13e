"""Plane sets for the new-velocity LP (shared by CPU and GPU tests): random
ones, and directed families for the branches random unit normals never reach."""
import hashlib

import numpy as np


def _base(rng, m, kind):
    """The three kinds of random_cases: (points, unit normals)."""
    nrm = rng.normal(size=(m, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if kind == 0:     # half-planes through points near the origin: often infeasible
        pts = rng.normal(size=(m, 3)) * rng.uniform(0.05, 2.0)
    elif kind == 1:   # LQR-obstacle-like: v_i - d n with moderate d
        pts = rng.normal(size=3) - rng.uniform(0.0, 3.0, size=(m, 1)) * nrm
    else:             # far planes: mostly feasible, exercises the speed sphere
        pts = -rng.uniform(10.0, 120.0, size=(m, 1)) * nrm
    return pts, nrm


def random_cases(n_cases: int, seed: int = 1, max_planes: int = 60):
    """Mix of feasible and infeasible sets so that linearProgram4 runs."""
    rng = np.random.default_rng(seed)
    cases, goals = [], []
    for t in range(n_cases):
        m = int(rng.integers(0, max_planes))
        pts, nrm = _base(rng, m, t % 3)
        cases.append(np.concatenate([pts, nrm], 1).astype(np.float32))
        goals.append(rng.normal(size=3) * rng.uniform(0.1, 150.0))
    return cases, np.array(goals)


# ---------------------------------------------------------------------------
# Directed families ("The LP on the hardest rows"): exactly parallel
# and nearly parallel planes, planes at the speed limit, zero normals and
# subnormal squares.  All inputs are finite.
# ---------------------------------------------------------------------------
# the LP's scans work in 64-plane chunks: rows end before, on and after a border
EDGE_SIZES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193)
FAMILIES = ("parallel", "sphere", "zero", "tiny")
EDGE_REPS = 4   # tests/golden/lp_edges.npz holds edge_cases(EDGE_REPS)
# |n_i x n_j|^2 ~ tilt^2 on both sides of RVO_EPSILON (1e-5)
_TILTS = np.sqrt(1e-5) * np.array([0.25, 0.9, 0.999, 1.001, 1.1, 4.0])
_SPHERE_D = np.array([60.0, 90.0, 99.0, 99.999, 100.0, 100.001, 101.0, 140.0])
# launch_lp's plane-layout switches: the last row length of one layout and the
# first of the next (32-B planes in LDS | 24-B planes, linearProgram4's
# projections in LDS too | projections in global memory | all in global memory)
LONG_SIZES = (2048, 2049, 3413, 3414, 6826, 6827)


def _perp(rng, n):
    a = rng.normal(size=n.shape)
    a -= (a * n).sum(1, keepdims=True) * n
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _parallel(rng, m, t):
    """First half: base planes.  Second half: partners of random earlier
    planes (point jittered), with the same normal, the negated one, a tilted
    one or a tilted and negated one.  Odd t: planes permuted, so partners
    land on both sides of the 64-plane chunk borders."""
    h = (m + 1) // 2
    k = m - h
    pts, nrm = _base(rng, h, t % 3)
    src = rng.integers(0, h, size=k) if h else np.zeros(0, int)
    mode = rng.integers(0, 4, size=k)
    n2 = nrm[src].copy()
    p2 = pts[src] + rng.normal(size=(k, 3)) * 0.3
    ang = rng.choice(_TILTS, size=k)
    if k:
        tl = np.cos(ang)[:, None] * n2 + np.sin(ang)[:, None] * _perp(rng, n2)
        n2 = np.where((mode == 0)[:, None], n2,
                      np.where((mode == 1)[:, None], -n2, np.where((mode == 2)[:, None], tl, -tl)))
    order = rng.permutation(m) if t % 2 else np.arange(m)
    return np.concatenate([np.concatenate([pts, p2]), np.concatenate([nrm, n2])], 1)[order].astype(np.float32)


def _sphere(rng, m, t):
    """Unit normals, point +-d n with d around and beyond the speed limit 100
    (+ two times in three: the plane pushes outward)."""
    _, nrm = _base(rng, m, 0)
    d = rng.choice(_SPHERE_D, size=(m, 1))
    sgn = rng.choice([1.0, 1.0, -1.0], size=(m, 1))
    return np.concatenate([sgn * d * nrm, nrm], 1).astype(np.float32)


def _zero(rng, m, t):
    """About 20 % of the normals are (0, 0, 0) (a first step's carried normal)."""
    pts, nrm = _base(rng, m, t % 3)
    nrm[rng.random(m) < 0.2] = 0.0
    return np.concatenate([pts, nrm], 1).astype(np.float32)


def _tiny(rng, m, t):
    """Points scaled by 1e-20: their squares are fp32 subnormals."""
    pts, nrm = _base(rng, m, t % 3)
    return np.concatenate([pts * 1e-20, nrm], 1).astype(np.float32)


_FAMILY_FN = {"parallel": _parallel, "sphere": _sphere, "zero": _zero, "tiny": _tiny}


def _goal(rng, t, c):
    k = t % 6
    if k == 0:
        return np.zeros(3)
    if k == 1:
        return np.array([100.0, 0.0, 0.0])
    if k == 2:
        g = rng.normal(size=3)
        return g / np.linalg.norm(g) * rng.uniform(100.0, 400.0)
    if k == 3 and len(c):
        return c[0, :3].astype(np.float64)   # exactly on the first plane
    if k == 4:
        return rng.normal(size=3) * 1e-20
    return rng.normal(size=3) * rng.uniform(0.1, 150.0)


def edge_cases(reps: int, seed: int = 12):
    """reps x EDGE_SIZES rows of each family, family-major, then repetition,
    then size: (cases, goals, family_names), one name per case.  A family's
    rows do not depend on reps, so edge_first_rep(reps) of any reps is the
    same set."""
    cases, goals, names = [], [], []
    for f, fam in enumerate(FAMILIES):
        rng = np.random.default_rng([seed, f])
        for rep in range(reps):
            for s, m in enumerate(EDGE_SIZES):
                t = rep * len(EDGE_SIZES) + s
                c = _FAMILY_FN[fam](rng, m, t)
                cases.append(c)
                goals.append(_goal(rng, t, c))
                names.append(fam)
    return cases, np.array(goals), names


def edge_first_rep(reps: int):
    """Indices into edge_cases(reps) of every family's first repetition."""
    n = len(EDGE_SIZES)
    return [(f * reps) * n + s for f in range(len(FAMILIES)) for s in range(n)]


def subnormal_cases(seed: int = 12):
    """Twelve base rows (3, 64, 65 and 129 planes) with points and goal scaled
    by 1e-38, 1e-39 and 1e-41: the coordinates themselves, and with them the
    LP's numerators, line parameters and results, are fp32 subnormals.  The
    tiny family's subnormal squares vanish beside radius^2 (a build that
    flushes subnormals to zero still passes it); here flushing changes the
    result.  Returns (cases, goals)."""
    rng = np.random.default_rng([seed, len(FAMILIES)])
    cases, goals = [], []
    for t in range(12):
        s = (1e-38, 1e-39, 1e-41)[t // 4]
        pts, nrm = _base(rng, (3, 64, 65, 129)[t % 4], t % 3)
        cases.append(np.concatenate([pts * s, nrm], 1).astype(np.float32))
        goals.append(rng.normal(size=3) * s)
    return cases, np.array(goals)


def fixture_rows():
    """The rows of tests/golden/lp_edges.npz: edge_cases(EDGE_REPS), then
    subnormal_cases() as a fifth family: (cases, goals, family_names)."""
    cases, goals, names = edge_cases(EDGE_REPS)
    sc, sg = subnormal_cases()
    return cases + sc, np.concatenate([goals, sg]), names + ["subnormal"] * len(sc)


def long_row(m: int, seed: int):
    """m - 129 far feasible planes, then a 129-plane parallel family, goal
    N(0, 1) * 5: linearProgram4 runs a few dozen iterations at plane indices
    near m, at a cost linear in m.  Returns (planes, goal)."""
    rng = np.random.default_rng(seed)
    pts, nrm = _base(rng, m - 129, 2)
    far = np.concatenate([pts, nrm], 1).astype(np.float32)
    c = np.concatenate([far, _parallel(rng, 129, 1)])
    return c, rng.normal(size=3) * 5.0


def digest(planes, goal) -> str:
    """SHA-256 of a row's bytes (float32 planes, float64 goal)."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(planes, np.float32).tobytes())
    h.update(np.ascontiguousarray(goal, np.float64).tobytes())
    return h.hexdigest()
