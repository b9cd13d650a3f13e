"""The canonical rule's hull kernels (k_lhull, k_hull, k_hull_big: cleared
LQRO_FLAG_QHULL_ORDER) against the oracle on the directed clouds of
tests/hull_cases.py, through lqro.Context.debug_hull (the hook
lqro_debug_hull_points_ex), and through the step on one pair whose hull
passes k_hull's 2,048 vertices.  tests/test_hull_cases_cpu.py holds the
clouds to the conditions relied on here.

"Exact" means: REC_HULL is set, and the selected facet (as a sorted triple),
the distance and the normal are bit-equal to orc_hull_branch's.

Not asserted (the hook cannot see them, and the kernels carry no counters for
them): whether an insertion took hull_insert_wide, whether a wave's face ring
spilled, whether the overflow bag was used.  Furthest-first insertion keeps
visible regions small on smooth clouds; the `fans` family is aimed at those
paths and is checked for exactness only.

What the MI355X gave when this file was written (the tests print it; DESIGN.md
§6.4 and §6.4b keep it): all_vertex 2047 and 2048 both finish in k_hull;
filled_2048 (2,048 vertices, 4,000 interior points) hands over with fail 1,
the cap counting insertions; 8,193 vertices end in k_hull_big as REC_HULLFAIL
by fail 1; k_lhull hands over near_facet t >= 0 with code 23 (16), the
lhull_caps centres and the 400-point fans with 24, the cube with 27, the
degenerate sets with 20, and decides everything else.  The file runs in 8 s,
its slowest test (test_through_the_step[retry]) in 1.1 s."""
import numpy as np
import pytest

import hull_cases as hc

pytestmark = pytest.mark.gpu

K_HULL_VERTS, K_HULL_BIG_VERTS = 2048, 8192
CAPACITY_CODES = (24, 26, 28)   # k_lhull: LH_VMAX vertices, LH_EMAX edge entries, LH_FMAX faces


@pytest.fixture
def ctx(lqro_mod, gains):
    c = lqro_mod.Context(lqro_mod.config(2, 100, 100))
    c.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    yield c
    c.close()


def _is_exact(lqro_mod, rec, e):
    return bool(rec["flags"] & lqro_mod.REC_HULL) and tuple(sorted(rec["facet"].tolist())) == e["facet"] and \
        np.array_equal(np.array([rec["dist"]]).view(np.uint64), np.array([e["dist"]]).view(np.uint64)) and \
        np.array_equal(np.ascontiguousarray(rec["normal"]).view(np.uint64), e["normal"].view(np.uint64))


def _assert_exact(lqro_mod, rec, e, where):
    assert rec["flags"] & lqro_mod.REC_HULL and not rec["flags"] & lqro_mod.REC_HULLFAIL, (where, int(rec["flags"]))
    assert tuple(sorted(rec["facet"].tolist())) == e["facet"], (where, rec["facet"], e["facet"], rec["dist"], e["dist"])
    assert rec["dist"] == e["dist"], (where, rec["dist"], e["dist"])
    assert _is_exact(lqro_mod, rec, e), (where, rec["normal"], e["normal"])
    assert rec["n_facets"] == e["nf"], (where, rec["n_facets"], e["nf"])


def _untouched(lqro_mod, rec):
    """The record as the hook made it: no kernel wrote a plane or a failure."""
    return rec["flags"] == lqro_mod.REC_INSIDE and rec["n_facets"] == 0 and rec["dist"] == 0.0 and \
        not np.any(rec["plane_normal"])


def _facets(fl):
    return sorted(tuple(sorted(t)) for t in fl.tolist())


def _vels(c, k=None):
    """(label, velocity, the oracle's answer), the first k."""
    return [(lab, v, e) for (lab, v), e in zip(c.vels, hc.expect(c))][:k]


# ---------------------------------------------------------------------------
# k_hull
# ---------------------------------------------------------------------------
def _k_hull_clouds(fam):
    cs = hc.clouds(fam)
    if fam == "all_vertex":
        cs = [c for c in cs if c.n <= 1024]
    return [c for c in cs if c.general]


@pytest.mark.parametrize("fam", ["tiny", "ties", "all_vertex", "filled", "near_facet", "fans", "scaled"])
def test_k_hull_exact(lqro_mod, ctx, fam):
    """Mode 0: k_hull's facet set is the oracle's and its selection is exact
    at every velocity.  Caps may not be blamed below half of them: up to
    1,024 vertices a hand-over is a failure (filled_2048 stands at the vertex
    cap: there k_hull may run out of face slots, and the retry, mode 4, must
    be exact)."""
    cs = _k_hull_clouds(fam)
    assert cs
    for c in cs:
        want = hc.facet_set(c)
        nverts = len({u for t in want for u in t})
        for lab, v, e in _vels(c):
            rec, fl, st = ctx.debug_hull(c.pts, v, 0)
            if st == -2 and nverts > K_HULL_VERTS // 2:
                print(f"{c.name} {lab}: k_hull handed {nverts} vertices over, fail code {ctx.debug_hull_fails}")
                assert _untouched(lqro_mod, rec), (c.name, lab)
                rec, fl, st = ctx.debug_hull(c.pts, v, 4)
                assert st == -2
            else:
                assert st == len(want), f"{c.name} {lab}: k_hull's status {st}, {len(want)} facets, {nverts} vertices"
                assert _facets(fl) == want, (c.name, lab)
            _assert_exact(lqro_mod, rec, e, (c.name, lab))


def test_k_hull_concurrent_insertions_repeat(lqro_mod, ctx):
    """Eight waves insert under face locks: 16 runs of the same cloud give
    the same record, bit for bit, and each is exact."""
    for n in (16, 64, 128):
        c = hc.cloud(f"all_vertex_{n}")
        lab, v, e = _vels(c)[2]
        want = hc.facet_set(c)
        runs = []
        for _ in range(16):
            rec, fl, st = ctx.debug_hull(c.pts, v, 0)
            assert st == len(want) and _facets(fl) == want, (c.name, st)
            _assert_exact(lqro_mod, rec, e, (c.name, lab))
            runs.append(rec.tobytes())
        assert len(set(runs)) == 1, f"{c.name}: {len(set(runs))} different records over 16 runs"


@pytest.mark.parametrize("n", [2047, 2048])
def test_vertex_cap_below(lqro_mod, ctx, n):
    """Mode 4 at k_hull's vertex cap and one below: k_hull finishes with the
    oracle's facets, or hands over (its free face slots sit in per-wave
    lists, so a face-slot hand-over is legitimate) and the retry is exact."""
    c = hc.cloud(f"all_vertex_{n}")
    want = hc.facet_set(c)
    seen = []
    for lab, v, e in _vels(c, 4):
        rec, fl, st = ctx.debug_hull(c.pts, v, 4)
        assert st == -2 or (st == len(want) and _facets(fl) == want), (c.name, lab, st)
        _assert_exact(lqro_mod, rec, e, (c.name, lab))
        seen.append(f"k_hull_big (retry, fail {ctx.debug_hull_fails})" if st == -2 else "k_hull")
    print(f"{c.name}: decided by {seen}")


@pytest.mark.parametrize("n", [2049, 4096])
def test_vertex_cap_above(lqro_mod, ctx, n):
    """Past 2,048 vertices k_hull hands over and writes nothing (mode 0);
    with its retry queue served (mode 4) the answer is exact."""
    c = hc.cloud(f"all_vertex_{n}")
    for lab, v, e in _vels(c, 2):
        rec, fl, st = ctx.debug_hull(c.pts, v, 0)
        assert st == -2 and fl is None, (c.name, lab, st)
        assert ctx.debug_hull_fails == (1,), f"{c.name}: handed over by {ctx.debug_hull_fails}, not the vertex cap"
        assert _untouched(lqro_mod, rec), (c.name, lab, rec)
        rec, fl, st = ctx.debug_hull(c.pts, v, 4)
        assert st == -2 and ctx.debug_hull_fails == (1,), (c.name, lab, st, ctx.debug_hull_fails)
        _assert_exact(lqro_mod, rec, e, (c.name, lab))
        assert rec["n_facets"] == 2 * n - 4


# ---------------------------------------------------------------------------
# k_hull_big
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_vertex_64", "all_vertex_2049", "all_vertex_4096", "all_vertex_8192",
                                  "filled_512", "filled_2048", "filled_dup2", "filled_dup3"])
def test_k_hull_big_exact(lqro_mod, ctx, name):
    """Mode 3: k_hull_big alone; it writes no facet list, so the facet count
    in the record and the selections stand for the hull."""
    c = hc.cloud(name)
    for lab, v, e in _vels(c, 10 if c.n < 2049 else 2):
        rec, _, st = ctx.debug_hull(c.pts, v, 3)
        _assert_exact(lqro_mod, rec, e, (c.name, lab))
        assert st == rec["n_facets"] == len(hc.facet_set(c))


def test_k_hull_big_vertex_cap(lqro_mod, ctx):
    """8,193 vertices: one more than k_hull_big holds (`nvtx >= kVerts`
    before the vertex is taken; 8,192 build: test_k_hull_big_exact):
    reported as REC_HULLFAIL with n_facets = -1, never a plane.  The cap is
    where the code says: a build of 8,193 would write past vx and vpid."""
    c = hc.cloud("all_vertex_8193")
    assert c.n == K_HULL_BIG_VERTS + 1
    for lab, v, e in _vels(c, 1):
        rec, _, st = ctx.debug_hull(c.pts, v, 3)
        assert rec["flags"] & lqro_mod.REC_HULLFAIL and not rec["flags"] & lqro_mod.REC_HULL, (lab, int(rec["flags"]))
        assert st == rec["n_facets"] == -1, (st, rec)
        assert rec["dist"] == 0.0 and not np.any(rec["plane_normal"]) and not np.any(rec["plane_point"])
        # by the vertex cap itself (fail 1), not by the face slots the 8,193rd cone would need (fail 4)
        assert ctx.debug_hull_fails == (1,), ctx.debug_hull_fails


# ---------------------------------------------------------------------------
# k_lhull
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(hc.FAMILIES))
def test_k_lhull_decides_exactly_or_hands_over(lqro_mod, ctx, fam):
    """Mode 1 on every family: a decision is exact; anything else is a
    hand-over with its reason.  It must decide what the CPU model decides
    with half of LH_VMAX (all_vertex up to 4,096 points, filled), and must
    hand over where the argument's premises fail."""
    reasons = {}
    for c in hc.clouds(fam):
        for lab, v, e in _vels(c):
            rec, _, st = ctx.debug_hull(c.pts, v, 1)
            where = (c.name, lab)
            if st == 0:
                reasons[0] = reasons.get(0, 0) + 1
                assert e["nf"] > 0, where
                _assert_exact_local(lqro_mod, rec, e, where)
            else:
                assert 20 <= st <= 35, (where, st)
                assert _untouched(lqro_mod, rec), (where, rec)
                reasons[st] = reasons.get(st, 0) + 1
            if (fam == "all_vertex" and c.n <= 4096) or fam == "filled":
                assert st == 0, f"{where}: handed over (code {st}) what the model decides with <= 128 vertices"
            if fam == "near_facet" and hc.near_t(lab) >= 0:
                assert st == 23, (where, st)
            if fam == "lhull_caps" and lab == "centre":
                assert st in CAPACITY_CODES, (where, st)
            if fam in ("coplanar", "degenerate"):
                assert st != 0, where
    print(f"k_lhull on {fam}: decided {reasons.pop(0, 0)}, handed over by code {dict(sorted(reasons.items()))}")


def _assert_exact_local(lqro_mod, rec, e, where):
    """Exact, but for the facet count: k_lhull counts the certified facets of
    its local hull, not the full hull's."""
    assert rec["flags"] & lqro_mod.REC_LOCAL, where
    assert tuple(sorted(rec["facet"].tolist())) == e["facet"], (where, rec["facet"], e["facet"], rec["dist"], e["dist"])
    assert _is_exact(lqro_mod, rec, e), (where, rec["dist"], e["dist"], rec["normal"], e["normal"])
    assert 0 < rec["n_facets"] <= e["nf"], (where, rec["n_facets"])


# ---------------------------------------------------------------------------
# near-degenerate and degenerate input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 4])
def test_coplanar_and_near_degenerate(lqro_mod, ctx, mode):
    """The facet is not defined; the distance is.  The cube's arithmetic is
    exact: distance and normal bit-equal.  A near-degenerate scaled cloud:
    the distance within 10 x the oracle's own spread over 8 insertion orders
    (floor 1e-15; the GPU's order is one more sample of that)."""
    (cube,) = hc.clouds("coplanar")
    for lab, v, e in _vels(cube):
        rec, fl, st = ctx.debug_hull(cube.pts, v, mode)
        assert rec["flags"] & lqro_mod.REC_HULL and st > 0, (lab, st)
        assert rec["dist"] == e["dist"] and np.array_equal(rec["normal"], e["normal"]), (lab, rec["dist"], rec["normal"])
        # the selected facet lies in the oracle's winning plane, z = 1
        assert np.all(cube.pts[rec["facet"], 2] == 1.0), (lab, rec["facet"])
        # a triangulation of the same surface: F = 2 V - 4 over the vertices used
        assert fl is not None and st == 2 * len(set(fl.reshape(-1).tolist())) - 4
    for c in hc.clouds("scaled"):
        if c.general:
            continue
        for (lab, v, e), sp in zip(_vels(c), hc.SPREADS[c.name]):
            rec, fl, st = ctx.debug_hull(c.pts, v, mode)
            assert rec["flags"] & lqro_mod.REC_HULL, (c.name, lab)
            assert abs(rec["dist"] - e["dist"]) <= max(10 * sp, 1e-15), (c.name, lab, rec["dist"], e["dist"])
            # the selected facet lies in the oracle's winning plane
            assert all(abs((c.pts[k] - c.pts[e["facet"][0]]) @ e["normal"]) <= 1e-9 * (np.abs(c.pts).max() + 1)
                       for k in rec["facet"])


@pytest.mark.parametrize("case", ["retry", "retry_local", "lds_145", "big_146", "big_knob"])
def test_through_the_step(lqro_mod, oracle, gains, monkeypatch, case):
    """One pair (N = 2, row 0) whose hull has more than 2,048 vertices, through
    lqro_step in the canonical rule: records and new velocities bit-equal to
    the oracle's step.  retry: k_hull hands the pair to k_hull_big's retry
    queue (LQRO_LOCAL_HULL=0); retry_local: the same with the local hull on;
    lds_145 / big_146: H NP on either side of kHullLdsMaxHNP = 21,845, the
    second running k_hull_big on the main queue; big_knob: LQRO_HULL_BIG=1."""
    sc = hc.STEP_CASES[case]
    for k, val in sc["env"].items():
        monkeypatch.setenv(k, val)
    H, NP = sc["H"], sc["NP"]
    x, vg = hc.step_states(sc)
    T, NCF = oracle.tables(gains["A"], gains["B"], gains["L"], gains["E"], H)
    S = oracle.sphere(NP)
    rv, rrecs = oracle.step(T, NCF, S, x, vg, rows=(0, 1))
    nv = hc.step_hull_vertices(sc)
    assert len(rrecs) == 1 and nv > K_HULL_VERTS, (case, nv)
    assert rrecs["flags"][0] & lqro_mod.REC_INSIDE and rrecs["flags"][0] & lqro_mod.REC_HULL
    assert rrecs["n_facets"][0] == 2 * nv - 4
    ctx = lqro_mod.Context(lqro_mod.config(2, H, NP, flags=lqro_mod.LQRO_FLAG_RECORDS, row_begin=0, row_end=1))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    try:
        newv = ctx.step(x, vg)
        recs = ctx.records()
        st = ctx.stats()
    finally:
        ctx.close()
    assert st["hull_fail"] == 0 and st["hull_ok"] == 1 and st["inside"] == 1, st
    assert np.array_equal(recs["flags"] & ~lqro_mod.REC_LOCAL, rrecs["flags"]), (case, recs["flags"], rrecs["flags"])
    assert not np.any(recs["flags"] & lqro_mod.REC_LOCAL) or case == "retry_local"
    for f in ("i", "j", "n_reach", "reach_hash", "facet", "n_facets"):
        if f == "n_facets" and recs["flags"][0] & lqro_mod.REC_LOCAL:
            continue   # (k_lhull counts its certified facets, not the hull's)
        assert np.array_equal(recs[f], rrecs[f]), (case, f, recs[f], rrecs[f])
    for f in ("dist", "normal", "plane_point", "plane_normal"):
        assert np.array_equal(recs[f].view(np.uint8), rrecs[f].view(np.uint8)), (case, f, recs[f], rrecs[f])
    assert np.array_equal(newv[0:1].view(np.uint64), rv[0:1].view(np.uint64)), (case, newv, rv)


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_degenerate_sets_are_reported(lqro_mod, ctx, mode):
    """Coplanar, collinear and coincident points (fail 8): REC_HULLFAIL,
    n_facets = -1, no plane; never a hand-over to a kernel that would also
    fail, never a plane.  (Kept last in the file.)"""
    for c in hc.clouds("degenerate"):
        for lab, v, e in _vels(c):
            assert e["nf"] < 0
            rec, fl, st = ctx.debug_hull(c.pts, v, mode)
            assert rec["flags"] & lqro_mod.REC_HULLFAIL and not rec["flags"] & lqro_mod.REC_HULL, (c.name, int(rec["flags"]))
            assert rec["n_facets"] == -1 and fl is None, (c.name, rec["n_facets"])
            assert st == (-1 if mode == 3 else 0) and ctx.debug_hull_fails == (8,), (c.name, st, ctx.debug_hull_fails)
            assert rec["dist"] == 0.0 and not np.any(rec["plane_normal"]) and not np.any(rec["plane_point"]), c.name
