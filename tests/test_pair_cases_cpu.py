"""The pair kernel's directed cases (tests/pair_cases.py) on the CPU: every
family sits where it claims to sit, on the oracle, and, where the reference's
own functions are built, the oracle equals them bit for bit on those cases.

The reference's sphere radii are globals of its source, so the `axes`, `tie_edge` and
`dist_exact` families (other radii) are pinned by the oracle alone; every other X = 16 group is
compared with ref_pair, each with its own min_reach and vmax_reach (both are
arguments of the reference's functions).  The X = 12 groups have no reference
build and are the oracle's too.

Each test prints its family's branch counts (run with -s to see them).
"""
import ctypes as C

import numpy as np
import pytest

import pair_cases as pc


def _steps(name):
    g = pc.group(name)
    key = ("cpu_step", name)
    if key not in pc._cache:
        pc._cache[key] = pc.oracle_step(g)
    return g, pc._cache[key][1]


def branch_counts(names) -> dict:
    """What the family's columns exercise, from the oracle's records and a
    numpy replay of the points: columns (and points) inside reach_exact's
    literal-division band |t / r^2 - 1| < 1e-12; columns whose last support
    direction w_vrel - w_hull has two or more exact maximisers among the
    reachable points; slices by content (every point reachable / none / some:
    the last are MIXED in any sound classification); GJK's iteration maximum
    and the simplex sizes seen."""
    out = dict(groups=len(names), cases=0, band_cases=0, band_points=0, tied_queries=0, slices_in=0, slices_out=0,
               slices_mixed=0, planes=0, inside=0, backups=0, gjk_iters_max=0, simplex_sizes={})
    for name in names:
        g, recs = _steps(name)
        pr = pc.Probe(g["H"], g["NP"], g["x_dim"], **g["cfg"])
        for col, r in zip(g["cols"], recs):
            pt, tq, lit = pr.replay(col)
            assert int(lit.sum()) == r["n_reach"], name
            band = np.abs(tq - 1.0) < 1e-12
            out["cases"] += 1
            out["band_cases"] += bool(band.any())
            out["band_points"] += int(band.sum())
            cnt = lit.sum(axis=1)
            out["slices_in"] += int((cnt == g["NP"]).sum())
            out["slices_out"] += int((cnt == 0).sum())
            out["slices_mixed"] += int(((cnt > 0) & (cnt < g["NP"])).sum())
            if r["flags"] & 1:
                out["planes"] += 1
                out["inside"] += bool(r["flags"] & 2)
                out["backups"] += bool(r["flags"] & 4)
                out["gjk_iters_max"] = max(out["gjk_iters_max"], int(r["gjk_iters"]))
                k = int(r["simplex_n"])
                out["simplex_sizes"][k] = out["simplex_sizes"].get(k, 0) + 1
                v = pt[lit] @ (r["wpt_vrel"] - r["wpt_hull"])
                out["tied_queries"] += bool((v == v.max()).sum() > 1)
    out["simplex_sizes"] = dict(sorted(out["simplex_sizes"].items()))
    return out


def _report(family):
    names = [n for n in pc.GROUPS if pc.family_of(n) == family]
    c = branch_counts(names)
    print(f"\n{family}: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    return c


def test_index():
    assert len(set(pc.GROUPS)) == len(pc.GROUPS)
    assert {pc.family_of(n) for n in pc.GROUPS} == set(pc.FAMILIES)
    for n in pc.GROUPS:
        g = pc.group(n)
        assert g["name"] == n and g["cols"].shape[1] == g["x_dim"] and g["row"].shape == (g["x_dim"],)
        assert not g["row"][:12].any() and not g["cols"][:, 6:12].any()   # at rest, hover attitude
        if g["x_dim"] == 16:
            assert np.all(g["cols"][:, 12:] == pc.HOVER) and np.all(g["row"][12:] == pc.HOVER)
    # the builders are deterministic
    again = pc._count_groups(16, "")[1]
    assert np.array_equal(again["cols"], pc.group("count_edge-m4")["cols"])


@pytest.mark.parametrize("prefix,x_dim", [("", 16), ("x12-", 12)])
def test_count_edge(prefix, x_dim):
    for m in pc.COUNT_MIN_REACH:
        g, recs = _steps(f"{prefix}count_edge-m{m}")
        assert g["cfg"]["min_reach"] == m and g["x_dim"] == x_dim
        a, b = g["meta"]["s"]
        assert np.nextafter(a, np.inf) == b
        n = recs["n_reach"]
        # s at -3..+3 ulps of the last double with n_reach = min_reach + 1
        assert list(n[:7]) == [m + 1] * 4 + [m] * 3, (m, n[:7])
        assert list(recs["flags"][:7] & 1) == [1] * 4 + [0] * 3
        if m == 0:   # the smallest clouds GJK can see
            assert list(n[7:]) == list(pc.SMALL_CLOUDS) and np.all(recs["flags"][7:] & 1)
            assert np.all(recs["simplex_n"][7:] >= 1) and np.all(recs["simplex_n"][7:] <= recs["n_reach"][7:])
    if x_dim == 16:
        g4 = pc.group("count_edge-m4")["meta"]["s"]
        assert g4[0] == 22.87655712361635   # the boundary 5 -> 4 of the ray
        for tag, runs in (("all_minus_1", True), ("all", False)):
            g, recs = _steps(f"count_edge-{tag}")
            full = g["H"] * g["NP"]
            assert g["cfg"]["min_reach"] == (full - 1 if runs else full)
            n = recs["n_reach"]
            assert (n == full).sum() >= 4 and ((n > 0) & (n < full)).sum() >= 3
            # GJK runs exactly when every point is reachable, or never
            assert np.array_equal((recs["flags"] & 1) != 0, (n == full) & runs)
            assert not (recs["flags"] & 2).any()
    _report(prefix + "count_edge" if not prefix else "x12")


def _check_point_group(name):
    g, recs = _steps(name)
    pr = pc.Probe(g["H"], g["NP"], g["x_dim"], **g["cfg"])
    counts = []
    for r, (off, d, a, b) in enumerate(g["meta"]["rays"]):
        assert np.nextafter(a, np.inf) == b
        ca, cb = g["cols"][2 * r], g["cols"][2 * r + 1]
        assert np.array_equal(ca, pr.col(off, d, a)) and np.array_equal(cb, pr.col(off, d, b))
        na, ia, _ = pr.reach(ca)
        nb, ib, _ = pr.reach(cb)
        assert (na, nb) == (recs["n_reach"][2 * r], recs["n_reach"][2 * r + 1])
        # n_reach changes by exactly one point across the two doubles ...
        diff = np.setxor1d(ia, ib)
        assert na - nb == 1 and diff.size == 1, (name, r, na, nb)
        k, p = divmod(int(diff[0]), g["NP"])
        # ... and that point is inside reach_exact's literal-division band on
        # both sides (t summed as exact_point and the pre-test order it)
        for col, n in ((ca, na), (cb, nb)):
            _, tq, lit = pr.replay(col)
            assert int(lit.sum()) == n
            assert abs(tq[k, p] - 1.0) < 1e-12, (name, r, tq[k, p])
        counts.append(na)
    return counts


def test_point_edge():
    counts = _check_point_group("point_edge-v30")
    assert len(counts) == 32 and min(counts) < 100 and max(counts) > 1000   # tens to thousands
    for v in pc.POINT_SEEDS_V:
        g, recs = _steps(f"point_edge-v{v:g}")
        assert g["cfg"]["vmax_reach"] == v and len(_check_point_group(g["name"])) == 8
    c = _report("point_edge")
    assert c["band_cases"] == c["cases"]
    # at a reach of 0.5 and 2 most live slices are MIXED
    cv = branch_counts([f"point_edge-v{v:g}" for v in pc.POINT_SEEDS_V])
    assert cv["slices_mixed"] > cv["slices_in"]


def test_inside_edge():
    g, recs = _steps("inside_edge")
    assert len(g["meta"]["rays"]) == 12 and len(recs) == 84
    pr = pc.Probe(g["H"], g["NP"])
    for r, (off, d, a, b) in enumerate(g["meta"]["rays"]):
        assert np.nextafter(a, np.inf) == b
        assert pr.inside(pr.col(off, d, 0.0))   # the ray starts inside the hull
        rr = recs[7 * r:7 * r + 7]
        assert np.all(rr["flags"] & 1)
        assert rr["flags"][3] & 2 and not rr["flags"][4] & 2   # the flag flips between a and b
        out = (rr["flags"] & 2) == 0
        # the outside members sit at the threshold
        assert np.all(np.abs(rr["dist"][out] - 1e-4) < 1e-6), (r, rr["dist"])
        assert np.all(rr["flags"][~out] & 8), "the oracle's hull failed"
    _report("inside_edge")


def test_axes():
    for rxy, rz in pc.AXES:
        g, recs = _steps(f"axes-{rxy:g}-{rz:g}")
        assert (g["cfg"]["xy_radius"], g["cfg"]["z_radius"]) == (rxy, rz) and len(g["cols"]) == 48
        speed = np.linalg.norm(g["cols"][40:, 3:6], axis=1)
        assert np.allclose(speed, np.linspace(20, 29, 8))
        assert (recs["flags"] & 1).sum() >= 40
        inside = (recs["flags"] & 2) != 0
        assert np.all(recs["flags"][inside] & 8), "the oracle's hull failed"
        if rxy == 0.0 or rz == 0.0:   # flat sets and curves: no hull is asked for
            assert not inside.any()
        pr = pc.Probe(g["H"], g["NP"], **g["cfg"])
        if (rxy, rz) == (0.0, 0.0):
            # the NP points of a slice coincide: every support query ties
            # NP-fold and the lowest index wins, so every simplex rank is a
            # multiple of NP
            ranks = recs["simplex"][recs["simplex"] >= 0]
            assert ranks.size > 40 and np.all(ranks % g["NP"] == 0) and ranks.max() > 0
            assert np.all(recs["n_reach"] % g["NP"] == 0)
        if (rxy, rz) in ((0.26, 0.0), (0.0, 0.75)):
            # flat and needle sets: slices whose points are partly reachable
            # (the slices a zero slice bound would misclass)
            part = 0
            for col in g["cols"]:
                _, idx, _ = pr.reach(col)
                cnt = np.bincount(idx // g["NP"], minlength=g["H"])
                part += bool(((cnt > 0) & (cnt < g["NP"])).any())
            assert 4 * part >= len(g["cols"]), (rxy, rz, part)
    c = _report("axes")
    assert c["tied_queries"] >= 40


def test_tie_edge():
    g, recs = _steps("tie_edge")
    pr = pc.Probe(g["H"], g["NP"], **g["cfg"])
    assert (g["cfg"]["xy_radius"], g["cfg"]["z_radius"]) == (0.0, 0.0) and len(g["meta"]["rays"]) == len(pc.TIE_SEEDS)
    for r, (off, d, a, b) in enumerate(g["meta"]["rays"]):
        assert np.nextafter(a, np.inf) == b
        sa, sb = pc.simplex_ids(pr, pr.col(off, d, a)), pc.simplex_ids(pr, pr.col(off, d, b))
        # the same reachable set and simplex size across adjacent doubles ...
        assert sa[0] == sb[0] and len(sa[1]) == len(sb[1]) >= 2, (r, sa, sb)
        # ... and a support query answered from another slice: the first
        # vertex in which the two simplices differ lies in two slices
        ka, kb = next((x // g["NP"], y // g["NP"]) for x, y in zip(sa[1], sb[1]) if x != y)
        assert ka != kb, (r, sa, sb)
        rr = recs[4 * r:4 * r + 4]
        assert np.all((rr["flags"] & 3) == 1)
        ranks = rr["simplex"][rr["simplex"] >= 0]
        assert np.all(ranks % g["NP"] == 0)   # NP-fold ties: the lowest index wins
    _report("tie_edge")


def test_dist_exact():
    g, recs = _steps("dist_exact")
    assert (g["H"], g["NP"], g["cfg"]["min_reach"]) == (1, 1, 0) and len(recs) == 3 * len(pc.EXACT_SEEDS)
    assert np.all(recs["n_reach"] == 1) and np.all(recs["simplex_n"] == 1)
    assert np.all((recs["flags"] & 3) == 1)   # a plane, outside: `distance < 0.0001` fails
    d = recs["dist"].reshape(-1, 3)
    assert np.all(d[:, 0] == 0.0001)          # ... at equality in each ray's first member
    assert np.all(d[:, 1:] >= 0.0001) and np.all(d[:, 1:] < 0.0001 + 1e-18)
    _report("dist_exact")


def test_shapes():
    assert len(pc.SHAPES) == 23
    for H, NP in pc.SHAPES:
        g, recs = _steps(f"shapes-H{H}-NP{NP}")
        assert (g["H"], g["NP"], g["x_dim"]) == (H, NP, 16) and len(g["cols"]) == 12
        # 63 H + 3 NP and one wave's region in 20480 doubles (X = 16, no class)
        pw = (NP + 63) // 64
        wave = 4 * H + H * pw + H + (H + (H & 1)) // 2 + 18 + 5
        waves = (20480 - 63 * H - 3 * NP) // wave
        assert waves >= 1, (H, NP)
        assert (waves == 1) == ((H, NP) == (256, 256))   # the one-wave launch
        inside = (recs["flags"] & 2) != 0
        if H * NP > 20000:
            assert not inside.any()
        assert inside.sum() == (1 if NP >= 4 and H <= 65 else 0)
        assert np.all(recs["flags"][inside] & 8), "the oracle's hull failed"
        assert np.all(recs["flags"] & 1)   # every column runs GJK
    _report("shapes")


def test_x12_point_edge():
    g, recs = _steps("x12-point_edge")
    assert g["x_dim"] == 12 and len(_check_point_group("x12-point_edge")) == 8


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.atleast_1d(np.asarray(a)).view(np.uint8)


@pytest.mark.parametrize("name", [n for n in pc.GROUPS if pc.family_of(n) not in ("axes", "tie_edge", "dist_exact", "x12")])
def test_oracle_equals_reference(oracle, name):
    """As test_oracle_vs_ref.test_pairs_random_swarms compares them."""
    ref = oracle.reflib()
    if ref is None:
        pytest.skip("oracle/_ref/libref.so not available (no reference tree)")
    ref.ref_pair.restype = C.c_int
    g = pc.group(name)
    gn = pc.gains(16)
    H, NP = g["H"], g["NP"]
    pr = pc.Probe(H, NP, **g["cfg"])
    idx = np.zeros(H * NP, np.int32)
    pts = np.zeros((H * NP, 3))
    xi = np.ascontiguousarray(g["row"])
    for j, col in enumerate(g["cols"]):
        n = C.c_int(0)
        dist = np.zeros(1)
        nrm, wv, wh = np.zeros(3), np.zeros(3), np.zeros(3)
        pl = np.zeros(6, np.float32)
        xj = np.ascontiguousarray(col)
        st = ref.ref_pair(NP, H, g["cfg"]["min_reach"], C.c_double(g["cfg"]["vmax_reach"]), _p(gn["A"]),
                          _p(gn["B"]), _p(gn["L"]), _p(gn["E"]), _p(xi), _p(xj), C.byref(n), _p(idx), _p(pts),
                          _p(dist), _p(nrm), _p(wv), _p(wh), _p(pl))
        rec, oidx, opts = pr.rec(xj, want_points=True)
        k = n.value
        assert rec["n_reach"] == k, (name, j)
        assert np.array_equal(oidx, idx[:k])
        assert np.array_equal(_bits(opts), _bits(pts[:k]))
        assert bool(rec["flags"] & 1) == (st != 2), (name, j)
        assert bool(rec["flags"] & 2) == (st == 1), (name, j)
        if st == 0:
            assert np.array_equal(_bits(rec["dist"]), _bits(dist[0])), (name, j)
            assert np.array_equal(_bits(rec["normal"]), _bits(nrm))
            assert np.array_equal(_bits(rec["wpt_vrel"]), _bits(wv)) and np.array_equal(_bits(rec["wpt_hull"]), _bits(wh))
            got = np.concatenate([rec["plane_point"], rec["plane_normal"]]).astype(np.float32)
            assert np.array_equal(_bits(got), _bits(pl))
