"""The pair kernel (pair_block, SliceSupport, gjkw_*) on the directed cases of
tests/pair_cases.py, against the CPU oracle: the reachable-count threshold,
single points on the reach sphere, the inside-hull threshold, degenerate and
extreme semi-axes, support ties between slices, a GJK distance of exactly
0.0001, and NP / H at the kernel's lane, word and slot edges.

One context per group, LQRO_FLAG_RECORDS, rows [0, 1): agent 0 is the row and
every other agent one of its columns.  Every comparison is exact: there is no
tolerance and no skipped case.  A group that holds an inside-hull pair runs
under both hull rules (the canonical one and Qhull's order with the carried
normal 0).
"""
import numpy as np
import pytest

import pair_cases as pc
from test_gpu_parity import _hull_pairs_equal

pytestmark = pytest.mark.gpu

EXACT = ("gjk_iters", "simplex_n", "simplex", "dist", "normal", "wpt_vrel", "wpt_hull", "plane_point", "plane_normal")
_oracle = {}


def _oracle_step(name, qhull):
    key = (name, qhull)
    if key not in _oracle:
        _oracle[key] = pc.oracle_step(pc.group(name), qhull)
    return _oracle[key]


def _gpu_step(lqro_mod, g, gains, qhull):
    x, vg = pc.swarm(g)
    flags = lqro_mod.LQRO_FLAG_RECORDS | (lqro_mod.LQRO_FLAG_QHULL_ORDER if qhull else 0)
    cfg = lqro_mod.config(x.shape[0], g["H"], g["NP"], x_dim=g["x_dim"], flags=flags, row_begin=0, row_end=1,
                          **g["cfg"])
    ctx = lqro_mod.Context(cfg)   # (a shape that pair_layout refuses raises here)
    try:
        ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
        newv = ctx.step(x, vg)
        return newv, ctx.records(), ctx.stats()
    finally:
        ctx.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check(lqro_mod, name, rule, newv, recs, st, rv, rrecs):
    what = f"{name} [{rule}]"
    m = len(rrecs)
    assert len(recs) == m
    assert np.array_equal(recs["i"], rrecs["i"]) and np.array_equal(recs["j"], rrecs["j"]), what
    bad = np.flatnonzero(recs["n_reach"] != rrecs["n_reach"])
    if bad.size:
        print(f"{what}: n_reach differs in {bad.size} of {m} columns; first j = {rrecs['j'][bad[0]]}: "
              f"GPU {recs['n_reach'][bad[0]]}, oracle {rrecs['n_reach'][bad[0]]}")
    assert not bad.size, what
    assert np.array_equal(recs["reach_hash"], rrecs["reach_hash"]), what
    assert np.array_equal(recs["flags"] & 7, rrecs["flags"] & 7), what
    inside = (rrecs["flags"] & 2) != 0
    out = ((rrecs["flags"] & 1) != 0) & ~inside
    for f in EXACT:
        a, b = recs[f][out], rrecs[f][out]
        eq = np.array_equal(_bits(a), _bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b)
        if not eq:
            k = np.flatnonzero([not np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b)])[0]
            print(f"{what}: {f} differs, first at j = {rrecs['j'][out][k]}: GPU {a[k]}, oracle {b[k]}")
        assert eq, (what, f)
    # a column without a plane leaves none
    none = (rrecs["flags"] & 1) == 0
    assert not recs["plane_normal"][none].any() and not recs["gjk_iters"][none].any(), what
    _hull_pairs_equal(lqro_mod, recs, rrecs, rule)
    assert st["hull_fail"] == 0, what
    assert st["pairs"] == m and st["inside"] == int(inside.sum()), what
    if not inside.any():
        assert np.array_equal(_bits(newv[0]), _bits(rv[0])), (what, newv[0], rv[0])
    return inside


@pytest.mark.parametrize("name", pc.GROUPS)
def test_pair_edges(lqro_mod, gains, name):
    g = pc.group(name)
    gn = gains if g["x_dim"] == 16 else pc.gains(g["x_dim"])
    rv, rrecs = _oracle_step(name, False)
    newv, recs, st = _gpu_step(lqro_mod, g, gn, False)
    inside = _check(lqro_mod, name, "canonical", newv, recs, st, rv, rrecs)
    if inside.any():
        rv, rrecs = _oracle_step(name, True)
        newv, recs, st = _gpu_step(lqro_mod, g, gn, True)
        _check(lqro_mod, name, "qhull", newv, recs, st, rv, rrecs)
