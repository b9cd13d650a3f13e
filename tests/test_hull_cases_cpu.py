"""The directed hull clouds (tests/hull_cases.py) meet the conditions the GPU
tests (tests/test_gpu_hull_cases.py) rely on, checked with the oracle and the
CPU model of the local hull (scripts/epa_spike.py) alone:

- general position: no point within 1e-9 (max|coord| + 1) of the plane of a
  facet it is not a vertex of (1e4 times the kernels' eps), so the facet set
  does not depend on the insertion order;
- the all-vertex clouds have n vertices and 2n - 4 facets;
- the velocities are strictly inside the hull (near_facet: on the side t says);
- the `ties` velocities have at least two bit-equal smallest rule values;
- the local-hull model decides all_vertex (n <= 4096) and filled with at most
  128 vertices, half of k_lhull's LH_VMAX, needs more than 256 at the centre
  of the lhull_caps spheres and fewer off the centre of the 2,048-point one;
- the cube's distance and normal do not depend on the insertion order, bit
  for bit; the degenerate sets have no hull.

A seed that does not meet a condition is replaced in hull_cases.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scripts"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "lqr-obstacles_amd")]

import hull_cases as hc   # noqa: E402

GENERAL = ("tiny", "ties", "all_vertex", "filled", "near_facet", "lhull_caps", "fans", "scaled")
LH_VMAX = 256


def _signed(c, v):
    """The largest signed distance of v from a facet's plane (< 0: strictly inside)."""
    import pyoracle
    f = pyoracle.hull(c.pts)
    a, b, cc = c.pts[f[:, 0]], c.pts[f[:, 1]], c.pts[f[:, 2]]
    n = np.cross(b - a, cc - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    assert np.all(((c.pts.mean(0)[None, :] - a) * n).sum(1) < 0), "orc_hull's facets are outward"
    return float(((np.asarray(v)[None, :] - a) * n).sum(1).max())


def test_clouds_fit_the_hook_context():
    names = set()
    for fam in hc.FAMILIES:
        for c in hc.clouds(fam):
            assert 4 <= c.n <= 100 * 100, c
            assert c.family == fam and c.name not in names and len(c.vels) >= 1
            names.add(c.name)
            assert np.array_equal(c.pts, hc.round6(c.pts)), f"{c}: not rounded"
            assert hc.cloud(c.name).n == c.n


@pytest.mark.parametrize("fam", GENERAL)
def test_general_position(fam):
    for c in hc.clouds(fam):
        if not c.general:
            assert fam == "scaled" and c.name in hc.NEAR_DEGENERATE
            continue
        gap = hc.plane_gap(c.pts, np.array(hc.facet_set(c)))
        lim = 1e-9 * (np.abs(c.pts).max() + 1.0)
        print(f"{c.name}: a point {gap:.3g} from a facet's plane at the least (bound {lim:.3g})")
        assert gap > lim, (c, gap, lim)
    assert all(not c.general for c in hc.clouds("coplanar") + hc.clouds("degenerate"))


def test_all_vertex_sizes():
    assert tuple(c.n for c in hc.clouds("all_vertex")) == hc.ALL_VERTEX_N
    for c in hc.clouds("all_vertex") + hc.clouds("lhull_caps") + hc.clouds("scaled"):
        fs = hc.facet_set(c)
        assert len(fs) == 2 * c.n - 4 and len({u for t in fs for u in t}) == c.n, c
        assert all(e["nf"] == 2 * c.n - 4 for e in hc.expect(c))
    for c in hc.clouds("all_vertex"):
        assert len(c.vels) == (10 if c.n < 4096 else 2)
    # filled: the surface points alone are vertices, every copy's first one
    for c, nv in zip(hc.clouds("filled"), (512, 2048, 200, 200)):
        fs = hc.facet_set(c)
        assert len(fs) == 2 * nv - 4 and len({u for t in fs for u in t}) == nv, c
    for c in hc.clouds("filled")[2:]:
        assert max(u for t in hc.facet_set(c) for u in t) < 200, "a later copy is a vertex"
    # fans: the apex (and the deep point, the other apex) meets every ring point
    for c, m in zip(hc.clouds("fans"), (96, 96, 400, 400)):
        deg = np.bincount(np.array(hc.facet_set(c)).reshape(-1), minlength=c.n)
        assert deg[m] == m or c.name.startswith("fans_cone"), (c, deg[m])
        assert deg[m + 1] == m, (c, deg[m + 1])


def test_velocities_inside():
    for fam in ("tiny", "ties", "all_vertex", "filled", "lhull_caps", "fans", "scaled", "coplanar"):
        for c in hc.clouds(fam):
            lim = 1e-9 * (np.abs(c.pts).max() + 1.0)
            for lab, v in c.vels:
                assert _signed(c, v) < -lim, (c, lab)
    (c,) = hc.clouds("near_facet")
    assert len(c.vels) == len(hc.NEAR_FACETS) * len(hc.NEAR_T)
    for (lab, v), e in zip(c.vels, hc.expect(c)):
        t = hc.near_t(lab)
        s = _signed(c, v)
        assert abs(s - t) < 1e-14, (lab, s)      # (the facet's own plane is the nearest; 1e-14: the rounding of coordinates ~ 1)
        # (outside the hull another facet's plane can pass nearer: the rule takes |.|)
        assert abs(e["dist"] - abs(t)) < 1e-14 if t <= 0 else e["dist"] <= t + 1e-14, (lab, e["dist"])


def test_ties_are_bit_equal():
    counts = {}
    for c in hc.clouds("ties"):
        fac = hc.canon_facets(c.pts)
        for (lab, v), e in zip(c.vels, hc.expect(c)):
            r = hc.rule_values(c.pts, v, fac)
            assert r.min() == e["dist"], "rule_values restates orc_hull_branch's arithmetic"
            w = np.nonzero(r == r.min())[0]
            assert len(w) >= 2, (c, lab)
            # the oracle takes the lowest triple (first vertex, then the other two ascending)
            assert e["facet"] == min(tuple(sorted(fac[k].tolist())) for k in w), (c, lab)
            counts[(c.name, lab)] = len(w)
    print("bit-equal smallest rule values:", counts)
    assert counts[("ties_tetra", "three faces at 0.2")] == 3
    assert sum(1 for k in counts if k[0].startswith("ties_mirror")) >= 8, "no mirror cloud gives a tie"


def test_local_hull_model():
    import epa_spike
    most = 0
    for c in [c for c in hc.clouds("all_vertex") if c.n <= 4096] + hc.clouds("filled"):
        for (lab, v), e in zip(c.vels, hc.expect(c)):
            res = epa_spike.local(c.pts, c.pts, v, vmax=LH_VMAX // 2)
            assert res is not None and res[0] is not None, (c, lab, res)
            assert res[2] <= LH_VMAX // 2
            assert res[0] == e["dist"] and tuple(sorted(res[1])) == e["facet"], (c, lab)
            most = max(most, res[2])
    print(f"all_vertex (n <= 4096) and filled: {most} local vertices at the most")
    for c in hc.clouds("lhull_caps"):
        assert c.vels[0][0] == "centre"
        res = epa_spike.local(c.pts, c.pts, c.vels[0][1], vmax=LH_VMAX)
        assert res is not None and res[0] is None and res[2] > LH_VMAX, (c, res)
    c = hc.cloud("lhull_caps_2048")
    res = epa_spike.local(c.pts, c.pts, c.vels[1][1], vmax=LH_VMAX)
    e = hc.expect(c)[1]
    assert res is not None and res[0] == e["dist"] and tuple(sorted(res[1])) == e["facet"] and res[2] < LH_VMAX
    print(f"lhull_caps_2048 off centre: {res[2]} local vertices")


def test_near_degenerate_by_permutation():
    (cube,) = hc.clouds("coplanar")
    assert np.all(cube.pts * 4 == np.round(cube.pts * 4)), "multiples of 0.25: exact arithmetic"
    for (lab, v), e, want in zip(cube.vels, hc.expect(cube), (0.7, 0.001)):
        res = hc.perm_branch(cube, v)
        assert all(d == e["dist"] and np.array_equal(n, e["normal"]) for d, n, _ in res), lab
        assert abs(e["dist"] - want) < 1e-15 and np.array_equal(e["normal"], [0.0, 0.0, 1.0])
        # the facet is not defined: every permutation's lies in the plane z = 1
        assert all(np.all(cube.pts[list(t), 2] == 1.0) for _, _, t in res)
        print(f"coplanar_cube {lab}: {len({t for _, _, t in res})} different facets over 8 permutations")
    assert hc.perm_spread(cube) == hc.SPREADS["coplanar_cube"] == (0.0, 0.0)
    for c in hc.clouds("scaled"):
        sp = hc.perm_spread(c)
        print(f"{c.name}: permutation spread of the distance {max(sp):.3g}" + ("" if c.general else " (near-degenerate)"))
        if not c.general:
            assert sp == hc.SPREADS[c.name], (c, sp)


def test_degenerate_sets_have_no_hull():
    cs = hc.clouds("degenerate")
    assert [c.name for c in cs] == ["degenerate_coplanar", "degenerate_collinear", "degenerate_coincident"]
    for c in cs:
        assert c.n == 50 and all(e["nf"] < 0 for e in hc.expect(c)), c


def test_step_cases_pass_k_hulls_vertex_cap():
    """The pair sent through the step is inside, with more hull vertices than
    k_hull holds, at every shape used."""
    for name, sc in hc.STEP_CASES.items():
        nv = hc.step_hull_vertices(sc)
        print(f"{name}: H {sc['H']} NP {sc['NP']}: {nv} hull vertices")
        assert nv > 2048, (name, nv)
    assert hc.STEP_CASES["lds_145"]["H"] * hc.STEP_CASES["lds_145"]["NP"] <= 21845 < \
        hc.STEP_CASES["big_146"]["H"] * hc.STEP_CASES["big_146"]["NP"]
