"""Directed cases for the pair kernel (test data only; CPU, deterministic).

A group is one step's worth of pairs that share a configuration: agent 0 is
the row, at rest at the origin, and agents 1..m are its columns, each a state
at hover attitude with nominal rotor forces whose position and velocity put
the pair (0, j) on an edge of the kernel:

  count_edge   n_reach on either side of `n > min_reach`, the smallest clouds
               GJK can see, and min_reach = H NP - 1 / H NP
  point_edge   one point on either side of findReachableObstacle's sphere,
               adjacent doubles apart (reach_exact's literal-division band)
  inside_edge  the relative velocity on either side of the inside-hull
               threshold `distance < 0.0001`
  axes         zero, tiny, huge and needle-shaped semi-axes
  tie_edge     zero semi-axes, a support query whose winner changes slice:
               the candidate pass decides among NP-fold ties
  dist_exact   one-point clouds whose GJK distance is 0.0001 exactly
  shapes       NP and H at the lane, word and slot edges of the kernel
  x12          count_edge and point_edge with the 12-state model

Everything is found with the oracle's own pair (orc_pair) by bisection along
a ray: the column stands at a fixed offset from the row and the relative
velocity v_i - v_j is s * dir; the brackets end as adjacent doubles.  The
rays come from seeded generators; the seeds below were picked when this file
was written so that every family meets the conditions
tests/test_pair_cases_cpu.py asserts (a ray whose count jumps by two points
at its boundary was replaced here, not skipped there).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import pyoracle as orc

HOVER = 9.80665 * 0.5 / 4   # nominalInput (LQRO:188)
VGOAL = np.array([0.5, -0.25, 0.125])
DEFAULTS = dict(xy_radius=0.26, z_radius=0.75, min_reach=4, vmax_reach=30.0)

# the ray of the count_edge family
COUNT_DIR = np.array([1.0, 0.3, 0.2])
COUNT_OFF = np.array([3.0, 0.5, 0.2])
COUNT_MIN_REACH = (0, 4, 37)
SMALL_CLOUDS = (1, 2, 3, 5, 6, 8)
ULPS = (-3, -2, -1, 0, 1, 2, 3)

AXES = ((0.0, 0.0), (0.26, 0.0), (0.0, 0.75), (1e-9, 1e-9), (5.0, 8.0), (0.01, 20.0))
SHAPES = ([(50, np_) for np_ in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)] +
          [(h, 50) for h in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)] +
          [(65, 65), (129, 33), (256, 256)])   # (H, NP)

# seeds of the rays (see the module docstring)
POINT_SEEDS = tuple(range(32))
POINT_SEEDS_V = {0.5: [[11, sd] for sd in (1, 5, 9, 10, 16, 24, 31)] + [[12, 0]],
                 2.0: [[11, sd] for sd in (1, 5, 9, 10, 16, 24, 31, 2)]}   # [generator tag, seed]: 11 = POINT_SEEDS' rays
INSIDE_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12)
X12_POINT_SEEDS = tuple(range(8))
AXES_SEED = 500
TIE_SEEDS = (15, 35, 45, 50, 63, 72, 75, 80, 94, 135, 149, 154)
EXACT_SEEDS = (0, 1, 2, 4, 5, 6, 7, 9)
SHAPES_SEED = 900

_cache: dict = {}


def gains(x_dim: int = 16) -> dict:
    """The default model's gains (the `gains` fixture for x_dim = 16)."""
    key = ("gains", x_dim)
    if key not in _cache:
        _cache[key] = orc.synthesize(x_dim=x_dim)
    return _cache[key]


def tabs(H: int, NP: int, x_dim: int = 16, xy_radius: float = 0.26, z_radius: float = 0.75):
    """(T, NCF, S) of the oracle for a shape and a point set."""
    key = ("T", H, x_dim)
    if key not in _cache:
        g = gains(x_dim)
        _cache[key] = orc.tables(g["A"], g["B"], g["L"], g["E"], H, X=x_dim)
    T, NCF = _cache[key]
    return T, NCF, orc.sphere(NP, xy_radius, z_radius)


def state(pos, vel, x_dim: int = 16) -> np.ndarray:
    x = np.zeros(x_dim)
    x[0:3] = pos
    x[3:6] = vel
    if x_dim == 16:
        x[12:16] = HOVER
    return x


def ulp(x: float, k: int) -> float:
    """x moved by k units in the last place (x > 0)."""
    return float((np.array([x]).view(np.int64) + k).view(np.float64)[0])


def bisect(pred, lo: float, hi: float):
    """pred(lo) and not pred(hi): adjacent doubles (a, b), a < b, with pred(a)
    and not pred(b)."""
    assert pred(lo) and not pred(hi), "no bracket"
    while True:
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            return lo, hi
        if pred(mid):
            lo = mid
        else:
            hi = mid


class Probe:
    """The oracle's pair for one configuration, the row at rest at the origin."""

    def __init__(self, H: int, NP: int, x_dim: int = 16, **cfg):
        self.H, self.NP, self.x_dim = H, NP, x_dim
        self.cfg = {**DEFAULTS, **cfg}
        self.T, self.NCF, self.S = tabs(H, NP, x_dim, self.cfg["xy_radius"], self.cfg["z_radius"])
        self.row = state(0.0, 0.0, x_dim)

    def col(self, off, dir_, s: float) -> np.ndarray:
        """The column at offset `off` with v_i - v_j = s dir."""
        return state(off, -s * np.asarray(dir_), self.x_dim)

    def rec(self, col, want_points: bool = False):
        return orc.pair(self.T, self.NCF, self.S, self.row, col, 0, 1, self.cfg["min_reach"],
                        self.cfg["vmax_reach"], want_points)

    def reach(self, col):
        """(n_reach, indices k NP + p, points) without GJK or a hull."""
        r, idx, pts = orc.pair(self.T, self.NCF, self.S, self.row, col, 0, 1, self.H * self.NP,
                               self.cfg["vmax_reach"], True)
        return int(r["n_reach"]), idx, pts

    def n(self, col) -> int:
        return self.reach(col)[0]

    def gjk_dist(self, col):
        """run_gjk's distance (LQRO:843) over the reachable points, or None
        where `n > min_reach` fails; no hull is built."""
        n, _, pts = self.reach(col)
        if not n > self.cfg["min_reach"]:
            return None
        vrel = np.ascontiguousarray(self.row[3:6] - col[3:6])
        pts = np.ascontiguousarray(pts)
        w1, w2, simplex = np.zeros(3), np.zeros(3), np.zeros(4, np.int32)
        it, sn, bk = C.c_int(0), C.c_int(0), C.c_int(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        sq = orc.lib().orc_gjk(p(vrel), n, p(pts), p(w1), p(w2), C.byref(it), C.byref(sn), p(simplex),
                               C.byref(bk))
        return float(np.sqrt(sq))

    def inside(self, col) -> bool:
        d = self.gjk_dist(col)
        return d is not None and d < 0.0001 and d > -1 * 0.0001

    def replay(self, col):
        """createObstacle's points and findReachableObstacle's sums replayed
        in numpy in the oracle's operation order: (points H x NP x 3,
        t / r^2 H x NP with t = a a + b b + c c as reach_exact's pre-test
        orders it, the literal test H x NP)."""
        X = self.x_dim
        d = self.row - col
        tr = np.zeros((self.H, 3))
        for c in range(X):
            tr = tr + self.NCF[:, :, c] * d[c]
        u = self.S[None, :, :] + tr[:, None, :]
        Tm = self.T.reshape(self.H, 1, 3, 3)
        pt = ((0.0 + Tm[..., 0] * u[..., 0:1]) + Tm[..., 1] * u[..., 1:2]) + Tm[..., 2] * u[..., 2:3]
        e = pt - (self.row[3:6] - col[3:6])
        a, b, c = e[..., 0], e[..., 1], e[..., 2]
        r2 = self.cfg["vmax_reach"] * self.cfg["vmax_reach"]
        t = a * a + b * b + c * c
        lit = (a * a) / r2 + (b * b) / r2 + (c * c) / r2 < 1.0
        return pt, t / r2, lit


def _group(name, pr: Probe, cols, **meta) -> dict:
    return dict(family=family_of(name), name=name, H=pr.H, NP=pr.NP, x_dim=pr.x_dim, cfg=dict(pr.cfg), row=pr.row.copy(),
                vgoal=VGOAL.copy(), cols=np.array(cols), meta=meta)


# ---------------------------------------------------------------- count_edge
def count_boundary(pr: Probe, m: int, off=COUNT_OFF, dir_=COUNT_DIR, lo=0.0, hi=64.0):
    """Adjacent doubles (a, b) with n_reach(a) > m >= n_reach(b) on the ray."""
    return bisect(lambda s: pr.n(pr.col(off, dir_, s)) > m, lo, hi)


def _count_groups(x_dim: int, prefix: str) -> list:
    H, NP = 50, 100
    out = []
    for m in COUNT_MIN_REACH:
        pr = Probe(H, NP, x_dim, min_reach=m)
        a, b = count_boundary(pr, m)
        cols = [pr.col(COUNT_OFF, COUNT_DIR, ulp(a, k)) for k in ULPS]
        small = []
        if m == 0:   # the smallest clouds GJK can see
            for n in SMALL_CLOUDS:
                sa, _ = count_boundary(pr, n - 1)
                cols.append(pr.col(COUNT_OFF, COUNT_DIR, sa))
                small.append(n)
        out.append(_group(f"{prefix}count_edge-m{m}", pr, cols, s=(a, b), small=small))
    if x_dim == 16:
        # every point reachable (n = H NP) or not: GJK runs exactly when
        # n = H NP (min_reach = H NP - 1), or never (min_reach = H NP).  The
        # reach is raised so that the first slices' points (|T_0| ~ 1e6) are
        # inside it; the columns stand far off, so that the relative velocity
        # is outside the hull of the whole set
        for tag, m in (("all_minus_1", H * NP - 1), ("all", H * NP)):
            pr = Probe(H, NP, x_dim, min_reach=m, vmax_reach=1e9)
            cols = [state(p, v) for p, v in (((50, 0, 0), (1, 2, 3)), ((50, 20, -10), (-2, 0, 1)),
                                             ((-40, 30, 5), (0, 0, 0)), ((30, -45, 20), (3, -3, 3)))]
            # ... and three whose first slice is partly out of reach
            cols += [state((x, 0, 0), (0, 1, 0)) for x in (1041.0, 1045.0, 1100.0)]
            out.append(_group(f"count_edge-{tag}", pr, cols))
    return out


# ---------------------------------------------------------------- point_edge
def _ray(seed, box: float):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3)
    return rng.uniform(-box, box, 3), d / np.linalg.norm(d)


def point_boundary(pr: Probe, seed, box: float, target, hi: float = 64.0):
    """A ray and adjacent doubles (a, b) across which n_reach falls through
    `target` (a count, or None: a third of the ray's largest count, 5 at the
    least so that GJK runs on both sides, searched from where that largest
    count is met)."""
    off, d = _ray(seed, box)
    lo = 0.0
    if target is None:
        ss = np.linspace(0.0, 10.0, 401)
        n = [pr.n(pr.col(off, d, s)) for s in ss]
        lo, target = float(ss[int(np.argmax(n))]), max(max(n) // 3, 5)
    a, b = bisect(lambda s: pr.n(pr.col(off, d, s)) > target, lo, hi)
    return off, d, a, b


def _point_group(name, pr: Probe, seeds, targets) -> dict:
    cols, rays = [], []
    for sd, tg in zip(seeds, targets):
        off, d, a, b = point_boundary(pr, sd, 0.8 if sd[0] == 12 else 3.0, None if tg is None else int(tg))
        cols += [pr.col(off, d, a), pr.col(off, d, b)]
        rays.append((off, d, a, b))
    return _group(name, pr, cols, rays=rays)


def _point_groups() -> list:
    H, NP = 50, 100
    out = [_point_group("point_edge-v30", Probe(H, NP), [[11, sd] for sd in POINT_SEEDS],
                        np.geomspace(20, 3000, len(POINT_SEEDS)))]
    # 8 of those rays again at a reach of 0.5 and of 2, where most live
    # slices are MIXED.  With offsets of +-3 only 7 of the 32 rays bring any
    # point within 0.5 of the relative velocity: the eighth ray at that reach
    # is one of its own (offsets of +-0.8)
    for v, seeds in POINT_SEEDS_V.items():
        out.append(_point_group(f"point_edge-v{v:g}", Probe(H, NP, vmax_reach=v), seeds, [None] * len(seeds)))
    return out


# --------------------------------------------------------------- inside_edge
def inside_boundary(pr: Probe, seed):
    """A ray from inside the reachable hull and adjacent doubles (a, b): the
    pair at a is inside, the pair at b has a plane and is outside."""
    off, d = _ray([13, seed], 0.3)
    hi = 1.0
    while pr.inside(pr.col(off, d, hi)):
        hi *= 2.0
    a, b = bisect(lambda s: pr.inside(pr.col(off, d, s)), 0.0, hi)
    return off, d, a, b


def _inside_groups() -> list:
    pr = Probe(50, 100)
    cols, rays = [], []
    for sd in INSIDE_SEEDS:
        off, d, a, b = inside_boundary(pr, sd)
        cols += [pr.col(off, d, ulp(a, k)) for k in ULPS]
        rays.append((off, d, a, b))
    return [_group("inside_edge", pr, cols, rays=rays)]


# ---------------------------------------------------------------------- axes
def _axes_groups() -> list:
    out = []
    for n, (rxy, rz) in enumerate(AXES):
        pr = Probe(50, 100, xy_radius=rxy, z_radius=rz)
        rng = np.random.default_rng([AXES_SEED, n])
        # a set with a zero semi-axis is flat or a curve: its hull has the
        # coplanar facets Qhull merges, which the step in Qhull's order
        # reports instead of deciding (the hull kernels' own suites); these
        # sets keep to columns whose pair is outside the hull
        flat = rxy == 0.0 or rz == 0.0
        cols = []
        while len(cols) < 40:
            c = state(rng.uniform(-3, 3, 3), rng.uniform(-8, 8, 3))
            if not (flat and pr.inside(c)):
                cols.append(c)
        for speed in np.linspace(20.0, 29.0, 8):   # slices straddle the reach sphere
            d = rng.normal(size=3)
            cols.append(state(rng.uniform(-3, 3, 3), speed * d / np.linalg.norm(d)))
        out.append(_group(f"axes-{rxy:g}-{rz:g}", pr, cols))
    return out


# ------------------------------------------------------------------ tie_edge
def simplex_ids(pr: Probe, col):
    """(reach_hash, the final simplex as point ids k NP + p, in GJK's order)
    of an outside pair with a plane, else None."""
    r, idx, _ = pr.rec(col, want_points=True)
    if (int(r["flags"]) & 3) != 1:
        return None
    return int(r["reach_hash"]), tuple(int(idx[k]) for k in r["simplex"][:r["simplex_n"]])


def tie_boundary(pr: Probe, seed):
    """A ray and adjacent doubles (a, b) with the same reachable set and a
    final simplex of the same size on both sides, whose vertices differ or
    come in another order: a support query's winner changes slice between
    them, so the two slices' values in that query agree to the last places."""
    off, d = _ray([15, seed], 0.6)
    ss = np.linspace(0.0, 8.0, 321)
    sig = [simplex_ids(pr, pr.col(off, d, s)) for s in ss]
    for i in range(len(ss) - 1):
        x, y = sig[i], sig[i + 1]
        if x is None or y is None or len(x[1]) != len(y[1]) or x[1] == y[1]:
            continue
        same = lambda s: (simplex_ids(pr, pr.col(off, d, s)) or (0, None))[1] == x[1]   # noqa: E731
        a, b = bisect(same, ss[i], ss[i + 1])
        sa, sb = simplex_ids(pr, pr.col(off, d, a)), simplex_ids(pr, pr.col(off, d, b))
        if sb is not None and sa[0] == sb[0] and len(sa[1]) == len(sb[1]):
            return off, d, a, b
    raise AssertionError(f"tie_edge: no change of winner on ray {seed}")


def _tie_groups() -> list:
    # zero semi-axes: the NP points of a slice coincide.  Next to the change
    # the two slices' bounds tie in the fp32 maximum that picks the slice
    # evaluated first (the lower one), so where the higher slice wins it wins
    # in the candidate pass, in which a lane meets p and p + 64 of the same
    # coincident slice: better()'s lowest-index rule decides
    pr = Probe(50, 100, xy_radius=0.0, z_radius=0.0)
    cols, rays = [], []
    for sd in TIE_SEEDS:
        off, d, a, b = tie_boundary(pr, sd)
        cols += [pr.col(off, d, ulp(a, k)) for k in (-1, 0, 1, 2)]
        rays.append((off, d, a, b))
    return [_group("tie_edge", pr, cols, rays=rays)]


# ---------------------------------------------------------------- dist_exact
def exact_boundary(pr: Probe, seed):
    """A one-point cloud (H = NP = 1, zero semi-axes, min_reach = 0: the
    point is T_0 Translate_0, and GJK's distance is |vrel - point|) with the
    column at the row's position: a direction and the first double s at which
    the pair is outside.  With s ~ 1e-9 a step of s moves the distance by
    about one unit in its last place, so the seeds kept are those where that
    distance is 0.0001 exactly."""
    d = np.random.default_rng([16, seed]).normal(size=3)
    d = d / np.linalg.norm(d)
    _, b = bisect(lambda s: pr.inside(pr.col(np.zeros(3), d, s)), 1e-12, 1e-3)
    return d, b


def _exact_groups() -> list:
    pr = Probe(1, 1, xy_radius=0.0, z_radius=0.0, min_reach=0)
    cols, rays = [], []
    for sd in EXACT_SEEDS:
        d, b = exact_boundary(pr, sd)
        # outside members only: a hull of one point cannot be built
        cols += [pr.col(np.zeros(3), d, ulp(b, k)) for k in (0, 1, 2)]
        rays.append((d, b))
    return [_group("dist_exact", pr, cols, rays=rays)]


# -------------------------------------------------------------------- shapes
def shape_config(H: int) -> dict:
    """With one or two slices (|T_0| ~ 1e6, |T_1| ~ 4e4: the points lie
    1e4..1e6 apart) no column reaches `n > 4` within the default reach of 30,
    and the step would compare nothing but n_reach <= 1: those two shapes
    take a reach that holds the whole set."""
    return dict(vmax_reach=1e7) if H <= 2 else {}


def _shape_group(H: int, NP: int, n: int) -> dict:
    pr = Probe(H, NP, **shape_config(H))
    rng = np.random.default_rng([SHAPES_SEED, n])
    want_inside = NP >= 4 and H <= 65
    cols, inside = [], None
    while len(cols) < 12 - want_inside:   # columns whose pair is not inside the hull
        c = state(rng.uniform(-3, 3, 3), rng.uniform(-4, 4, 3))
        if not pr.inside(c):
            cols.append(c)
    for _ in range(4000 if want_inside else 0):
        c = state(rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.5, 0.5, 3))
        if pr.inside(c):
            inside = c
            break
    if want_inside:
        assert inside is not None, (H, NP)
        cols.append(inside)
    return _group(f"shapes-H{H}-NP{NP}", pr, cols, want_inside=want_inside)


# ----------------------------------------------------------------------- x12
def _x12_groups() -> list:
    out = _count_groups(12, "x12-")
    out.append(_point_group("x12-point_edge", Probe(50, 100, 12), [[14, sd] for sd in X12_POINT_SEEDS],
                            np.geomspace(20, 3000, len(X12_POINT_SEEDS))))
    return out


# ------------------------------------------------------------------ the index
_BUILDERS = {
    "count_edge": lambda: _count_groups(16, ""),
    "point_edge": _point_groups,
    "inside_edge": _inside_groups,
    "axes": _axes_groups,
    "tie_edge": _tie_groups,
    "dist_exact": _exact_groups,
    "x12": _x12_groups,
}
FAMILIES = ("count_edge", "point_edge", "inside_edge", "axes", "tie_edge", "dist_exact", "shapes", "x12")
GROUPS = ([f"count_edge-m{m}" for m in COUNT_MIN_REACH] + ["count_edge-all_minus_1", "count_edge-all"] +
          ["point_edge-v30"] + [f"point_edge-v{v:g}" for v in POINT_SEEDS_V] + ["inside_edge"] +
          [f"axes-{a:g}-{b:g}" for a, b in AXES] + ["tie_edge", "dist_exact"] + [f"shapes-H{h}-NP{n}" for h, n in SHAPES] +
          [f"x12-count_edge-m{m}" for m in COUNT_MIN_REACH] + ["x12-point_edge"])


def family_of(name: str) -> str:
    return name.split("-")[0]


def group(name: str) -> dict:
    """The group `name` of GROUPS (built once per process, family by family;
    the shapes one by one)."""
    key = ("group", name)
    if key not in _cache:
        fam = family_of(name)
        if fam == "shapes":
            n = GROUPS.index(name) - GROUPS.index(f"shapes-H{SHAPES[0][0]}-NP{SHAPES[0][1]}")
            _cache[key] = _shape_group(*SHAPES[n], n)
        else:
            for g in _BUILDERS[fam]():
                _cache[("group", g["name"])] = g
    return _cache[key]


def groups_of(family: str) -> list:
    return [group(n) for n in GROUPS if family_of(n) == family]


def swarm(g: dict):
    """(x, vgoal) of the group's step: the row, then its columns."""
    x = np.vstack([g["row"][None, :], g["cols"]])
    vg = np.zeros((x.shape[0], 3))
    vg[0] = g["vgoal"]
    return x, vg


def oracle_step(g: dict, qhull_order: bool = False):
    """(newV, records) of row 0 from the oracle, under the canonical rule or in
    Qhull's order with the carried normal 0."""
    pr = Probe(g["H"], g["NP"], g["x_dim"], **g["cfg"])
    x, vg = swarm(g)
    if qhull_order:
        orc.set_hull_rule(1, round16=True)
        orc.carry_normal(np.zeros(3))
    try:
        return orc.step(pr.T, pr.NCF, pr.S, x, vg, min_reach=g["cfg"]["min_reach"],
                        vmax_reach=g["cfg"]["vmax_reach"], rows=(0, 1), threads=8)
    finally:
        if qhull_order:
            orc.set_hull_rule(0)
