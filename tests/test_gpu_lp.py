"""GPU new-velocity LP (lqro_calculate_new_v, one wavefront per agent) vs the
oracle's sequential fp32 restatement of calculateNewV: bit-exact."""
import numpy as np
import pytest

from lp_cases import random_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,max_planes", [(1, 60), (2, 200), (3, 1100)])
def test_lp_bit_exact(lqro_mod, oracle, seed, max_planes):
    cases, goals = random_cases(300 if max_planes < 500 else 60, seed=seed, max_planes=max_planes)
    got = lqro_mod.calculate_new_v(cases, goals)
    ref = np.array([oracle.newv(c, g) for c, g in zip(cases, goals)])
    bad = np.where(~np.all(got == ref, axis=1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:3]], ref[bad[:3]])


def test_lp_c3_hardest_rows(lqro_mod):
    """The C3 swarm's slowest linearProgram4 rows (tests/golden/lp_rows.npz,
    1,023 planes each, made by make_golden_lp_rows.py from the oracle step
    that qhull_order.npz pins): bit-exact new velocities."""
    import os
    from conftest import GOLDEN
    d = np.load(os.path.join(GOLDEN, "lp_rows.npz"))
    got = lqro_mod.calculate_new_v(list(d["planes"]), d["vgoal"], vmax_lp=float(d["vmax_lp"]))
    assert np.array_equal(got.view(np.uint64), d["newv"].view(np.uint64))


@pytest.fixture(scope="module")
def lp_edges(oracle):
    """tests/golden/lp_edges.npz (the reference's calculateNewV on the
    directed families of lp_cases.edge_cases) with the oracle's answers."""
    import os
    from conftest import GOLDEN
    d = np.load(os.path.join(GOLDEN, "lp_edges.npz"))
    offs = d["offsets"]
    cases = [d["planes"][offs[k]:offs[k + 1]] for k in range(offs.size - 1)]
    names = [str(d["families"][f]) for f in d["family"]]
    orc = np.array([oracle.newv(c, g) for c, g in zip(cases, d["vgoal"])])
    return dict(cases=cases, goals=d["vgoal"], names=names, newv=d["newv"], oracle=orc,
                long={int(m): (int(s), v, str(h)) for m, s, v, h in
                      zip(d["long_m"], d["long_seed"], d["long_newv"], d["long_sha"])})


def _assert_rows_equal(got, want, what, cases, names):
    bad = np.where(~np.all(got.view(np.uint64) == want.view(np.uint64), axis=1))[0]
    if bad.size:
        k = int(bad[0])
        fams = sorted({(names[b], len(cases[b])) for b in bad})
        pytest.fail(f"{bad.size} rows differ from {what}; (family, planes): {fams[:12]}; first: row {k} "
                    f"({names[k]}, {len(cases[k])} planes) got {got[k]} want {want[k]}")


def test_lp_edge_families(lqro_mod, lp_edges):
    """Every row of lp_edges.npz in one call (32-B planes in LDS): exactly and
    nearly parallel planes, planes at the speed limit, zero normals and
    subnormal squares, on both sides of the scans' 64-plane chunk borders,
    and the rows with subnormal coordinates (a kernel that flushes subnormals
    to zero fails on those).
    Bit-exact against the oracle and the reference's recorded answers."""
    e = lp_edges
    got = lqro_mod.calculate_new_v(e["cases"], e["goals"])
    _assert_rows_equal(got, e["oracle"], "the oracle", e["cases"], e["names"])
    _assert_rows_equal(got, e["newv"], "lp_edges.npz", e["cases"], e["names"])


# launch_lp (lqro_kern_lp.hip) picks the plane layout from the longest row:
# 32 B a plane in LDS while npr * 32 <= 64 KiB; then 24 B a plane while
# npr * 24 <= 160 KiB (linearProgram4's projections in LDS too while both
# fit: 2 * npr * 24 <= 160 KiB); beyond, everything in global memory
_LDS32, _LDS_CU = 64 * 1024, 160 * 1024
_SWITCHES = (_LDS32 // 32, _LDS_CU // (2 * 24), _LDS_CU // 24)


@pytest.mark.parametrize("m_long", [2048, 2049, 3413, 3414, 6826, 6827])
def test_lp_edge_layouts(lqro_mod, oracle, lp_edges, m_long):
    """The first repetition of every family (52 rows) beside one long row, so
    that the degenerate rows run under each plane layout of launch_lp, at the
    last row length of one layout and the first of the next (dynamic LDS of
    65,536 B at 2,048 planes and 163,824 B at 3,413 and 6,826).  The long row
    ends in a parallel family: linearProgram4 works at plane indices near
    m_long.  Bit-exact against the oracle and the reference's answers."""
    import lp_cases
    assert [m for s in _SWITCHES for m in (s, s + 1)] == [2048, 2049, 3413, 3414, 6826, 6827]
    assert 2 * 3413 * 24 == 6826 * 24 == 163824
    e = lp_edges
    seed, want_long, sha = e["long"][m_long]
    c, g = lp_cases.long_row(m_long, seed)
    assert len(c) == m_long and lp_cases.digest(c, g) == sha, "long_row is not the fixture's row"
    first = lp_cases.edge_first_rep(lp_cases.EDGE_REPS)
    cases = [e["cases"][i] for i in first] + [c]
    names = [e["names"][i] for i in first] + ["long"]
    assert [len(x) for x in cases[:-1]] == list(lp_cases.EDGE_SIZES) * len(lp_cases.FAMILIES)
    goals = np.concatenate([e["goals"][first], g[None]])
    got = lqro_mod.calculate_new_v(cases, goals)   # raises unless LQRO_OK
    orc = np.concatenate([e["oracle"][first], oracle.newv(c, g)[None]])
    _assert_rows_equal(got, orc, "the oracle", cases, names)
    _assert_rows_equal(got, np.concatenate([e["newv"][first], want_long[None]]), "lp_edges.npz", cases, names)
