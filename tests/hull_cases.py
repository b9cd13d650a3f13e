"""Directed point clouds for the canonical rule's hull kernels (test data
only; CPU, deterministic): k_lhull, k_hull and k_hull_big through the hook
lqro_debug_hull_points_ex (lqro.Context.debug_hull).

A cloud is a set of %g-rounded points (the oracle's round6, as qconvex reads
them) with a list of relative velocities; expect() is what the oracle
(orc_hull_branch, the sequential reference) says at each of them.  For points
in general position the facet set does not depend on the insertion order, so
the kernels must reproduce it and the selection bit for bit.

  tiny        the smallest hulls: the unit tetrahedron, the tetrahedron with
              interior points, n = 5, 6, 8 all-vertex
  ties        velocities with bit-equal rule values on two or three facets
              (hull_select's lexicographic tie rule against the oracle's)
  all_vertex  ellipsoid clouds, every point a vertex: n on either side of
              k_hull's 2,048 and k_hull_big's 8,192 vertices
  filled      all_vertex with interior points, and with every point repeated
  near_facet  velocities within GJK's inside tolerance of a facet, on either
              side of it
  lhull_caps  spheres whose centre needs more local vertices than k_lhull has
  fans        high-degree vertices: flat cones and bipyramids over a ring
  scaled      all_vertex 512 at 1e-3 and 30 times its size, and on the 1e-4
              lattice round6 leaves at |coord| ~ 25
  coplanar    a grid on each face of a cube: the distance is defined, the
              facet is not
  degenerate  coplanar, collinear and coincident points: no hull

The seeds below were picked when this file was written so that every family
meets the conditions tests/test_hull_cases_cpu.py asserts (a seed that does
not is replaced here, not skipped there).

`ties`: besides the tetrahedron, mirror-symmetric clouds (mirror_cloud:
pairs of points with x negated, velocities on the plane x = 0) do give
bit-equal ties, at every velocity tried: a facet's mirror image has the same
canonical first vertex and the opposite orientation, and (b - a) x (c - a)
with the operands exchanged and x negated is the mirrored normal exactly.
Two mirror pairs alone are four coplanar points, so a belt of points on the
plane keeps every facet off it and the clouds in general position.

Near-degenerate clouds (NEAR_DEGENERATE): a `scaled` cloud that does not pass
the general-position condition would be checked as `coplanar` is: by
distance, within the oracle's own dependence on the insertion order
(perm_spread: 8 seeded permutations).  With the seeds below all three pass
(the first two seeds of all_vertex 512 left 1e-3 times the cloud 6e-10 from a
plane, under the 1e-9 bound), so the list is empty and the cube is the only
cloud checked that way; its spread is 0, its arithmetic being exact.  For
the record, the permutations move the distance of the scaled clouds (whose
facet set is unique: a permutation changes the vertex a facet is measured
from) by at most 5.4e-20 (x 1e-3), 3.6e-15 (x 30) and 5.6e-17 (lattice)."""
from __future__ import annotations

import numpy as np

import pyoracle as orc

AXES = (1.0, 0.8, 0.6)
ALL_VERTEX_N = (16, 64, 65, 128, 512, 1024, 2047, 2048, 2049, 4096, 8192, 8193)
FRACTIONS = (0.5, 0.9, 0.99)
NEAR_T = (-1e-3, -1e-5, -1e-9, 0.0, 1e-9, 1e-5, 9e-5)
LHULL_OFF = (0.01, 0.02, -0.01)
FAN_M = (96, 400)

# seeds (see the module docstring)
ALL_VERTEX_SEED = {n: 1000 + n for n in ALL_VERTEX_N}
ALL_VERTEX_SEED[512] = 1514              # (1512, 1513: 1e-3 times the cloud is not in general position)
TINY_SEED = {5: 5, 6: 6, 8: 8}
TINY_FILL_SEED = 60
FILL_SEED = {512: 7512, 2048: 9048}
DUP_SEED = 200
SPHERE_SEED = {2048: 32048, 4096: 34096}
FAN_SEED = {96: 96, 400: 400}
MIRROR_SEED = (3, 4)
MIRROR_AIM = (2, 12, 21, 40)            # the points a mirror cloud's velocities aim at (x set to 0)
NEAR_FACETS = (0, 301, 655, 1019)        # of all_vertex 512's 1,020 facets (orc_hull's order)
VEL_SEED = 77                            # which points the fractional velocities aim at
PERM_SEED = 2024

# scaled clouds that are not in general position (checked as `coplanar` is)
NEAR_DEGENERATE = ()
# max - min of the oracle's distance over 8 seeded permutations of the points,
# per velocity, of the clouds checked by distance (tests/test_hull_cases_cpu.py
# measures them again; the cube's must be 0: its arithmetic is exact)
SPREADS = {"coplanar_cube": (0.0, 0.0)}

_cache: dict = {}


def round6(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a, np.float64)
    return np.array([orc.round6(v) for v in a.reshape(-1)]).reshape(a.shape)


class Cloud:
    """name, family, pts (n x 3, rounded), vels [(label, v)], general: in
    general position (the facet set is unique)."""

    def __init__(self, name, family, pts, vels, general=True):
        self.name, self.family, self.general = name, family, general
        self.pts = np.ascontiguousarray(pts, np.float64)
        self.vels = [(lab, np.ascontiguousarray(v, np.float64)) for lab, v in vels]
        self.n = self.pts.shape[0]

    def __repr__(self):
        return f"<{self.name} n={self.n}>"


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def ellipsoid(n: int, seed: int, axes=AXES) -> np.ndarray:
    """n unit-normal directions scaled by the axes, rounded."""
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return round6(d * np.asarray(axes))


def frac_vels(pts: np.ndarray, nk: int = 3, fracs=FRACTIONS, seed: int = VEL_SEED):
    """The centroid, and centroid + f (P[k] - centroid) for nk points."""
    cen = pts.mean(0)
    ks = np.random.default_rng(seed + pts.shape[0]).choice(pts.shape[0], nk, replace=False)
    out = [("centroid", cen)]
    for k in ks:
        for f in fracs:
            out.append((f"{f}->P[{int(k)}]", cen + f * (pts[k] - cen)))
    return out


def oriented(pts: np.ndarray, tri) -> tuple:
    """(centroid, outward unit normal) of a facet."""
    a, b, c = pts[tri[0]], pts[tri[1]], pts[tri[2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    if n @ (pts.mean(0) - a) > 0:
        n = -n
    return (a + b + c) / 3.0, n


def _all_vertex(n: int) -> Cloud:
    pts = ellipsoid(n, ALL_VERTEX_SEED[n])
    vels = frac_vels(pts) if n < 4096 else frac_vels(pts, 1, (0.9,))
    return Cloud(f"all_vertex_{n}", "all_vertex", pts, vels)


def _tetra() -> np.ndarray:
    return np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])


def _tiny():
    t = _tetra()
    out = [Cloud("tiny_tetra", "tiny", t, [("centroid", t.mean(0)), ("near z=0", (0.3, 0.3, 0.01))])]
    w = np.random.default_rng(TINY_FILL_SEED).dirichlet(np.ones(4), size=60) * 0.8 + 0.05   # every weight >= 0.05
    full = round6(np.concatenate([t, w @ t]))
    out.append(Cloud("tiny_tetra_filled", "tiny", full, [("centroid", full.mean(0)), ("near z=0", (0.3, 0.3, 0.01))]))
    for n, sd in TINY_SEED.items():
        pts = ellipsoid(n, sd)
        cen, nrm = oriented(pts, orc.hull(pts)[0])
        out.append(Cloud(f"tiny_{n}", "tiny", pts, [("centroid", pts.mean(0)), ("near facet 0", cen - 0.01 * nrm)]))
    return out


MIRROR_BELT = 12


def mirror_cloud(seed: int, m: int = 32) -> np.ndarray:
    """MIRROR_BELT points on the plane x = 0, then 2m points off it, point
    MIRROR_BELT + 2k + 1 the mirror image (x negated) of point MIRROR_BELT +
    2k.  The belt lies outside the others' shadow on the plane (1.2 times the
    ellipse, a 12-gon: 1.2 cos 15 deg > 1), so no hull facet crosses the
    plane: two mirror pairs would make it a coplanar quadrilateral."""
    h = ellipsoid(m, 5000 + seed)
    h[:, 0] = np.abs(h[:, 0]) + 0.05
    ph = 2 * np.pi * (np.arange(MIRROR_BELT) + np.random.default_rng(seed).uniform(-0.2, 0.2, MIRROR_BELT)) / MIRROR_BELT
    pts = np.zeros((MIRROR_BELT + 2 * m, 3))
    pts[:MIRROR_BELT, 1] = 1.2 * AXES[1] * np.cos(ph)
    pts[:MIRROR_BELT, 2] = 1.2 * AXES[2] * np.sin(ph)
    pts[MIRROR_BELT::2] = h
    pts[MIRROR_BELT + 1::2] = h * np.array([-1.0, 1.0, 1.0])
    return round6(pts)


def canon_facets(pts: np.ndarray) -> np.ndarray:
    """orc_hull's facets, each rotated so that its lowest point id leads
    (orientation kept): the triples the rule measures from."""
    f = orc.hull(pts)
    k = np.argmin(f, axis=1)
    return np.stack([np.take_along_axis(f, ((k + e) % 3)[:, None], 1)[:, 0] for e in range(3)], axis=1)


def rule_values(pts: np.ndarray, v, fac: np.ndarray) -> np.ndarray:
    """|n_f . (v - P[t0(f)])| per canonical facet, in orc_hull_branch's
    arithmetic operation by operation (P = P_rounded here)."""
    a, b, c = pts[fac[:, 0]], pts[fac[:, 1]], pts[fac[:, 2]]
    e1, e2 = b - a, c - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    ln = np.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
    n0, n1, n2 = n0 / ln, n1 / ln, n2 / ln
    v = np.asarray(v, np.float64)
    return np.abs(n0 * (v[0] - a[:, 0]) + n1 * (v[1] - a[:, 1]) + n2 * (v[2] - a[:, 2]))


def tie_count(pts: np.ndarray, v) -> int:
    """How many of the oracle's facets share the smallest rule value, bit for bit."""
    r = rule_values(pts, v, canon_facets(pts))
    return int((r == r.min()).sum())


def _ties():
    t = _tetra()
    out = [Cloud("ties_tetra", "ties", t, [("three faces at 0.2", (0.2, 0.2, 0.2)), ("two faces at 0.1", (0.1, 0.1, 0.3))])]
    for sd in MIRROR_SEED:
        pts = mirror_cloud(sd)
        cen = pts.mean(0)
        vels = []
        # velocities on the mirror plane: the nearest facet and its image tie
        for k in MIRROR_AIM:
            for f in (0.9, 0.7):
                v = cen + f * (pts[k] - cen)
                v[0] = 0.0
                vels.append((f"x=0, {f}->P[{k}]", v))
        out.append(Cloud(f"ties_mirror_{sd}", "ties", pts, vels))
    return out


def _filled():
    out = []
    for n, sd in FILL_SEED.items():
        surf = ellipsoid(n, ALL_VERTEX_SEED[n])
        rng = np.random.default_rng(sd)
        inner = surf[rng.integers(0, n, 4000)] * rng.uniform(0.2, 0.98, 4000)[:, None]
        pts = round6(np.concatenate([surf, inner]))[rng.permutation(n + 4000)]
        out.append(Cloud(f"filled_{n}", "filled", pts, frac_vels(pts)))
    surf = ellipsoid(200, DUP_SEED)
    for rep in (2, 3):
        pts = np.concatenate([surf] * rep)
        out.append(Cloud(f"filled_dup{rep}", "filled", pts, frac_vels(surf)))
    return out


def _near_facet():
    pts = ellipsoid(512, ALL_VERTEX_SEED[512])
    fac = orc.hull(pts)
    vels = []
    for f in NEAR_FACETS:
        cen, nrm = oriented(pts, fac[f])
        for t in NEAR_T:
            vels.append((f"facet {f} t={t:g}", cen + t * nrm))
    return [Cloud("near_facet_512", "near_facet", pts, vels)]


def near_t(label: str) -> float:
    return float(label.split("t=")[1])


def _lhull_caps():
    out = []
    for n, sd in SPHERE_SEED.items():
        pts = ellipsoid(n, sd, (1.0, 1.0, 1.0))
        out.append(Cloud(f"lhull_caps_{n}", "lhull_caps", pts,
                         [("centre", np.zeros(3)), ("off centre", np.array(LHULL_OFF))]))
    return out


def _ring(m: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * (np.arange(m) + rng.uniform(-0.3, 0.3, m)) / m
    # on the unit cylinder: every ring point is extreme in the projection on
    # the plane z = 0, so it is a vertex whatever stands above and below
    # (the heights: well below the 0.1 (2 pi / m)^2 by which a cone from 0.1
    # above passes over the next ring point, so the apex meets every ring point)
    zj = 0.01 * (2 * np.pi / m) ** 2
    return np.stack([np.cos(ph), np.sin(ph), rng.uniform(-zj, zj, m)], axis=1)


def _fans():
    out = []
    for m in FAN_M:
        ring = _ring(m, FAN_SEED[m])
        rng = np.random.default_rng(FAN_SEED[m] + 1)
        # a flat cone (slope 0.1): the apex sees every ring point; points 1e-3
        # from it on nearly horizontal rays (slope 0.01 to 0.02 down: under
        # the apex, over the cone) see the fan's faces within some 80 degrees
        u = rng.normal(size=(6, 3))
        u[:, 2] = -0.02 * rng.uniform(0.5, 1.0, 6)
        u /= np.linalg.norm(u, axis=1)[:, None]
        apex = np.array([0.0, 0.0, 0.1])
        cone = round6(np.concatenate([ring, [apex], [[0.0, 0.0, -5.0]], apex + 1e-3 * u]))
        vels = [("centroid", cone.mean(0)), ("under the apex", (0.01, -0.02, 0.05)), ("low", (0.2, 0.1, -2.0))]
        out.append(Cloud(f"fans_cone_{m}", "fans", cone, vels))
        bip = round6(np.concatenate([ring, [[0.0, 0.0, 0.1]], [[0.0, 0.0, -0.1]]]))
        vels = [("centroid", bip.mean(0)), ("under the apex", (0.01, -0.02, 0.05)), ("off centre", (0.4, 0.3, -0.01))]
        out.append(Cloud(f"fans_bipyramid_{m}", "fans", bip, vels))
    return out


def _scaled():
    d = np.random.default_rng(ALL_VERTEX_SEED[512]).normal(size=(512, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    base = d * np.asarray(AXES)
    out = []
    for name, s in (("scaled_small", 1e-3), ("scaled_large", 30.0)):
        pts = round6(base * s)
        out.append(Cloud(name, "scaled", pts, frac_vels(pts)))
    pts = round6(0.5 * d + np.array([25.0, -25.0, 20.0]))
    out.append(Cloud("scaled_lattice", "scaled", pts, frac_vels(pts, 2)))
    for c in out:
        c.general = c.name not in NEAR_DEGENERATE
    return out


def _coplanar():
    g = np.linspace(-1.0, 1.0, 9)
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g))
    pts = []
    for ax in range(3):
        for s in (-1.0, 1.0):
            p = np.empty((81, 3))
            p[:, ax] = s
            p[:, (ax + 1) % 3] = a
            p[:, (ax + 2) % 3] = b
            pts.append(p)
    # (edge and corner points appear on two or three faces: once each)
    pts = np.unique(np.concatenate(pts), axis=0)
    pts = pts[np.random.default_rng(9).permutation(pts.shape[0])]
    return [Cloud("coplanar_cube", "coplanar", round6(pts), [("0.7 from z=1", (0.1, 0.2, 0.3)), ("0.001 from z=1", (0.1, 0.2, 0.999))],
                  general=False)]


def _degenerate():
    rng = np.random.default_rng(50)
    flat = np.concatenate([rng.uniform(-1, 1, (50, 2)), np.full((50, 1), 0.25)], axis=1)
    line = np.outer(rng.uniform(-1, 1, 50), (1.0, 2.0, -1.0))
    one = np.tile([0.5, -0.25, 0.125], (50, 1))
    return [Cloud(f"degenerate_{k}", "degenerate", round6(p), [("centroid", round6(p).mean(0))], general=False)
            for k, p in (("coplanar", flat), ("collinear", line), ("coincident", one))]


FAMILIES = {
    "tiny": _tiny,
    "ties": _ties,
    "all_vertex": lambda: [_all_vertex(n) for n in ALL_VERTEX_N],
    "filled": _filled,
    "near_facet": _near_facet,
    "lhull_caps": _lhull_caps,
    "fans": _fans,
    "scaled": _scaled,
    "coplanar": _coplanar,
    "degenerate": _degenerate,
}


def clouds(family: str) -> list:
    if ("clouds", family) not in _cache:
        _cache[("clouds", family)] = FAMILIES[family]()
    return _cache[("clouds", family)]


def cloud(name: str) -> Cloud:
    if name.startswith("all_vertex_"):   # (one size without building the twelve)
        if ("cloud", name) not in _cache:
            _cache[("cloud", name)] = _all_vertex(int(name.rsplit("_", 1)[1]))
        return _cache[("cloud", name)]
    for fam in FAMILIES:
        if name.startswith(fam):
            return next(c for c in clouds(fam) if c.name == name)
    raise KeyError(name)


# ---------------------------------------------------------------------------
# one pair through the step
# ---------------------------------------------------------------------------
# Agent 0 at rest at the origin, agent 1 STEP_POS away and closing at 1 m/s:
# the pair is inside, and its reachable sets, strung out along the approach,
# give a hull of some 3,000 vertices: past k_hull's 2,048.  Row 0 alone is
# computed (row_end = 1): one pair, one hull.  env: the knobs a context reads
# when it is created.
STEP_POS, STEP_VEL = (2.0, 0.2, 0.1), (-1.0, 0.02, 0.01)
STEP_VGOAL = ((0.5, -0.25, 0.125), (-0.5, 0.1, 0.0))
STEP_CASES = {
    "retry": dict(H=200, NP=100, env={"LQRO_LOCAL_HULL": "0"}),
    "retry_local": dict(H=200, NP=100, env={"LQRO_LOCAL_HULL": "1"}),
    "lds_145": dict(H=145, NP=150, env={"LQRO_LOCAL_HULL": "0"}),        # H NP = 21,750 <= kHullLdsMaxHNP = 21,845
    "big_146": dict(H=146, NP=150, env={"LQRO_LOCAL_HULL": "0"}),        # 21,900: k_hull_big takes the main queue
    "big_knob": dict(H=145, NP=150, env={"LQRO_LOCAL_HULL": "0", "LQRO_HULL_BIG": "1"}),
}
HOVER = 9.80665 * 0.5 / 4   # nominalInput (LQRO:188)


def step_states(case: dict):
    """(x, vgoal) of the two agents (16 states, hover attitude)."""
    x = np.zeros((2, 16))
    x[1, 0:3] = STEP_POS
    x[1, 3:6] = STEP_VEL
    x[:, 12:16] = HOVER
    return x, np.array(STEP_VGOAL)


def step_hull_vertices(case: dict) -> int:
    """Row 0's pair by the oracle: the vertices of its hull (0: not inside)."""
    if ("stepv", case["H"], case["NP"]) not in _cache:
        g = orc.synthesize()
        T, NCF = orc.tables(g["A"], g["B"], g["L"], g["E"], case["H"])
        S = orc.sphere(case["NP"])
        x, _ = step_states(case)
        rec, _, P = orc.pair(T, NCF, S, x[0], x[1], 0, 1, want_points=True)
        _cache[("stepv", case["H"], case["NP"])] = \
            len(set(orc.hull(round6(P)).reshape(-1).tolist())) if rec["flags"] & 2 else 0
    return _cache[("stepv", case["H"], case["NP"])]


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def facet_set(c: Cloud) -> list:
    """orc_hull's facets as sorted triples, sorted."""
    if ("facets", c.name) not in _cache:
        _cache[("facets", c.name)] = sorted(tuple(sorted(t)) for t in orc.hull(c.pts).tolist())
    return _cache[("facets", c.name)]


def expect(c: Cloud) -> list:
    """Per velocity what orc_hull_branch says: dict(nf, facet (sorted triple),
    dist, normal), nf <= 0: it cannot build a hull."""
    if ("expect", c.name) not in _cache:
        out = []
        for _, v in c.vels:
            k, d, nrm, fac = orc.hull_branch(c.pts, v)
            out.append(dict(nf=int(k), facet=tuple(sorted(fac.tolist())), dist=d, normal=nrm.copy()))
        _cache[("expect", c.name)] = out
    return _cache[("expect", c.name)]


def perm_branch(c: Cloud, v, nperm: int = 8, seed: int = PERM_SEED) -> list:
    """orc_hull_branch on nperm seeded permutations of the points, the facet
    mapped back to the cloud's ids: [(dist, normal, sorted facet)]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nperm):
        p = rng.permutation(c.n)
        k, d, nrm, fac = orc.hull_branch(c.pts[p], v)
        assert k > 0
        out.append((d, nrm.copy(), tuple(sorted(int(p[t]) for t in fac))))
    return out


def perm_spread(c: Cloud) -> tuple:
    """max - min of the oracle's distance over the permutations, per velocity."""
    if ("spread", c.name) not in _cache:
        _cache[("spread", c.name)] = tuple(
            max(r[0] for r in res) - min(r[0] for r in res)
            for res in (perm_branch(c, v) for _, v in c.vels))
    return _cache[("spread", c.name)]


def plane_gap(pts: np.ndarray, fac: np.ndarray, chunk: int = 256) -> float:
    """The smallest distance of a point from the plane of a facet it is not
    a vertex of (coincident copies of a facet's vertices excepted: they are
    the vertex), over all facets."""
    best = np.inf
    fac = np.asarray(fac)
    # every point's first copy (its own id where no two points coincide)
    _, first, inv = np.unique(pts, axis=0, return_index=True, return_inverse=True)
    rep = first[inv.reshape(-1)]
    dups = len(first) < pts.shape[0]
    for f0 in range(0, fac.shape[0], chunk):
        t = fac[f0:f0 + chunk]
        a, b, c = pts[t[:, 0]], pts[t[:, 1]], pts[t[:, 2]]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n, axis=1)[:, None]
        d = np.abs(pts @ n.T - np.einsum("ij,ij->i", a, n)[None, :])   # (its rounding, 1e-15 |coord|, is far below the bound)
        cols = np.arange(t.shape[0])
        for e in range(3):
            if dups:
                d[rep[:, None] == rep[t[:, e]][None, :]] = np.inf
            else:
                d[t[:, e], cols] = np.inf
        best = min(best, float(d.min()))
    return best
