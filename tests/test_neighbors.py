"""Opt-in neighbour culling (RVO2 computeNeighbors /
insertAgentNeighbor, AGT:74-81,153-174).  The oracle's selection against a
brute-force restatement (CPU), then the GPU step with culling against the
oracle step with culling (bit-exact records and newV)."""
import numpy as np
import pytest


def _brute(x, i, r, k):
    d = x[i, :3] - x[:, :3]   # the kernels' op order: dx*dx + dy*dy + dz*dz
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    cand = [(d2[j], j) for j in range(len(x)) if j != i and d2[j] < r * r]
    keep = sorted(cand)[:k]
    sel = np.zeros(len(x), np.uint8)
    for _, j in keep:
        sel[j] = 1
    return sel


@pytest.mark.parametrize("seed,k,r", [(1, 4, 2.0), (2, 10, 3.0), (3, 100, 1.5), (4, 3, 50.0)])
def test_oracle_selection(oracle, lqro_mod, seed, k, r):
    x, _ = lqro_mod.synthetic_swarm(40, seed=seed, box=4.0)
    for i in range(0, 40, 7):
        assert np.array_equal(oracle.neighbors(x, i, r, k), _brute(x, i, r, k))


def test_oracle_selection_ties(oracle):
    """Equal distances: the lower j is kept (RVO2 keeps the earlier-visited)."""
    x = np.zeros((7, 16))
    for j, p in enumerate([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (2, 0, 0), (0, -1, 0)]):
        x[j, :3] = p
    sel = oracle.neighbors(x, 0, 10.0, 3)
    assert sel.tolist() == [0, 1, 1, 1, 0, 0, 0]


def _lattice(lqro_mod):
    """synthetic_swarm(64) on a 4 x 4 x 4 grid of spacing 2.0: every distance
    is exact, so equal (d2) keys and d2 == r2 are certain."""
    x, vg = lqro_mod.synthetic_swarm(64)
    g = np.arange(4) * 2.0
    x[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(64, 3)
    return x, vg


LATTICE_CASES = [(4, 4.0), (7, 4.0), (20, 4.0), (6, 2.0)]


def _assert_oracle_selection_on_lattice(oracle, x, k, r):
    n_sel = 0
    for i in range(len(x)):
        sel = oracle.neighbors(x, i, r, k)
        assert np.array_equal(sel, _brute(x, i, r, k)), i
        n_sel += int(sel.sum())
    return n_sel


@pytest.mark.parametrize("k,r", LATTICE_CASES)
def test_oracle_selection_lattice(oracle, lqro_mod, k, r):
    """r 4.0: the two-step neighbours sit at d2 == r2 and stay out (strict <);
    k 4 and 7 cut inside a group of equal distances (6 at d2 4, 12 at d2 8);
    r 2.0: nobody is nearer than r."""
    x, _ = _lattice(lqro_mod)
    n_sel = _assert_oracle_selection_on_lattice(oracle, x, k, r)
    if r == 2.0:
        assert n_sel == 0
    else:   # the corner agent 0 has 3 + 3 + 1 agents nearer than 4.0, the inner agent 21 has 26
        assert int(oracle.neighbors(x, 0, r, k).sum()) == min(k, 7)
        assert int(oracle.neighbors(x, 21, r, k).sum()) == min(k, 26)


def _culled_step(lqro_mod, oracle, gains, x, vg, H, NP, k, r, rows=None):
    """One step with culling by the oracle and by the GPU: (oracle newV,
    oracle records [rows, N - 1], Context, GPU newV, GPU records [rows, K])."""
    N = x.shape[0]
    r0, r1 = rows if rows is not None else (0, N)
    T, NCF = oracle.tables(gains["A"], gains["B"], gains["L"], gains["E"], H)
    S = oracle.sphere(NP)
    oracle.set_neighbors(r, k)
    try:
        rv, rrecs = oracle.step(T, NCF, S, x, vg, rows=rows)
    finally:
        oracle.set_neighbors(0.0, 0)
    kw = dict(row_begin=r0, row_end=r1) if rows is not None else {}
    ctx = lqro_mod.Context(lqro_mod.config(N, H, NP, flags=lqro_mod.LQRO_FLAG_RECORDS, **kw))
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    ctx.set_neighbors(r, k)
    newv = ctx.step(x, vg)
    recs = ctx.records()
    K = min(k, N - 1)
    assert recs.shape[0] == (r1 - r0) * K
    return rv, rrecs.reshape(r1 - r0, N - 1), ctx, newv, recs.reshape(r1 - r0, K)


def _assert_culled_rows(lqro_mod, gr, rr, fields, planes):
    """Row by row: the GPU's slots are the oracle's kept pairs in ascending j
    (fields equal, planes and inside-hull facets bit-exact where asked), then
    empty slots.  Returns the number of kept pairs."""
    kept = 0
    for i in range(gr.shape[0]):
        ref_row = rr[i][rr[i]["n_reach"] >= 0]
        c = len(ref_row)
        kept += c
        assert c <= gr.shape[1] and np.all(gr[i][c:]["n_reach"] == -1) and np.all(gr[i][c:]["j"] == -1)
        g = gr[i][:c]
        for f in fields:
            a = g[f] & ~lqro_mod.REC_LOCAL if f == "flags" else g[f]   # the oracle has no local hull
            assert np.array_equal(a, ref_row[f]), (i, f)
        if planes:
            for f in ("plane_point", "plane_normal"):
                assert np.array_equal(g[f].view(np.uint32), ref_row[f].view(np.uint32)), (i, f)
            ins = (g["flags"] & lqro_mod.REC_INSIDE) != 0
            assert np.array_equal(g["facet"][ins], ref_row["facet"][ins]), i
    return kept


ALL_FIELDS = ("i", "j", "n_reach", "flags", "gjk_iters", "simplex_n", "reach_hash")


@pytest.mark.gpu
@pytest.mark.parametrize("k,r,box", [(6, 2.5, 3.0), (1, 1.0, 3.0), (500, 1000.0, 3.0), (8, 3.0, 1.6)])
def test_gpu_step_with_culling(lqro_mod, oracle, gains, k, r, box):
    """box 1.6: a dense swarm, so neighbour pairs reach the in-kernel hull
    (slot -> neighbour mapping in k_hull)."""
    N, H, NP = 48, 40, 50
    x, vg = lqro_mod.synthetic_swarm(N, seed=17, box=box)
    rv, rr, ctx, newv, gr = _culled_step(lqro_mod, oracle, gains, x, vg, H, NP, k, r)
    kept = _assert_culled_rows(lqro_mod, gr, rr, ALL_FIELDS, planes=True)
    assert ctx.stats()["pairs"] == kept == int((rr["n_reach"] >= 0).sum())
    if box < 2:
        assert int(((gr["flags"] & lqro_mod.REC_INSIDE) != 0).sum()) > 0
    np.testing.assert_array_equal(newv, rv)
    # all pairs again
    ctx.set_neighbors(0.0, 0)
    ctx.step(x, vg)
    assert ctx.stats()["pairs"] == N * (N - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k,r", LATTICE_CASES)
def test_gpu_culling_lattice_ties(lqro_mod, oracle, gains, k, r):
    """k_nbr's (d2, j) tie rule and its strict d2 < r2 on the lattice swarm
    (see test_oracle_selection_lattice), against the oracle step with culling:
    records and newV bit-exact, as in test_gpu_step_with_culling."""
    H, NP = 40, 50
    x, vg = _lattice(lqro_mod)
    n_sel = _assert_oracle_selection_on_lattice(oracle, x, k, r)
    rv, rr, ctx, newv, gr = _culled_step(lqro_mod, oracle, gains, x, vg, H, NP, k, r)
    kept = _assert_culled_rows(lqro_mod, gr, rr, ALL_FIELDS, planes=True)
    assert ctx.stats()["pairs"] == kept == n_sel
    if r == 2.0:
        assert kept == 0 and np.all(gr["j"] == -1)
    np.testing.assert_array_equal(newv, rv)


def _many_candidates(lqro_mod, oracle, gains, N, nrows):
    H, NP, k, r = 20, 50, 3, 1.0e4
    x, vg = lqro_mod.synthetic_swarm(N, seed=19)
    rv, rr, ctx, newv, gr = _culled_step(lqro_mod, oracle, gains, x, vg, H, NP, k, r, rows=(0, nrows))
    assert all(int((rr[i]["n_reach"] >= 0).sum()) == k for i in range(nrows))
    _assert_culled_rows(lqro_mod, gr, rr, ("j", "n_reach", "flags", "reach_hash"), planes=False)
    np.testing.assert_array_equal(newv[:nrows], rv[:nrows])


@pytest.mark.gpu
def test_gpu_culling_many_candidates(lqro_mod, oracle, gains):
    """More agents within the radius than k_nbr's LDS candidate list holds
    (1,024): the selection falls back to scanning global memory per round."""
    _many_candidates(lqro_mod, oracle, gains, 1100, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1025, 1026])
def test_gpu_culling_candidate_list_edge(lqro_mod, oracle, gains, N):
    """Every other agent is within the radius: N 1,025 fills k_nbr's LDS
    candidate list to its cap (1,024 candidates), N 1,026 is the first size
    that scans global memory instead."""
    _many_candidates(lqro_mod, oracle, gains, N, 8)
