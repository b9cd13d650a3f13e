"""The horizon conflict prediction's CPU side: the numpy
restatement's licence (pyoracle.tables' NCF value for value, inverse(CG_k)
against T_k, the pair loop against a plain scalar loop), the tie rules, the
exports and struct sizes, merge_prediction over row splits, the C++ consumer
without a device, the kernels' descriptors (no private memory), the link to
the method on the dense swarms and the swap scenario's pinned first hits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import predict_cases as pc
import predict_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREDICT_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_predict_main")
INF = float("inf")
RXY, RZ = 0.26, 0.75


# the licence ----------------------------------------------------------------
@pytest.mark.parametrize("x_dim", [16, 12])
def test_tables_against_the_oracle(oracle, x_dim):
    g = oracle.synthesize(x_dim=x_dim)
    h = 100
    CG, NCF = pr.tables(g["A"], g["B"], g["L"], g["E"], h)
    T, N0 = oracle.tables(g["A"], g["B"], g["L"], g["E"], h, X=x_dim)
    assert np.array_equal(NCF, N0)                       # the F recursion, value for value
    worst = 0.0
    for k in range(h):
        t = T[k].reshape(3, 3)
        d = np.abs(np.linalg.inv(CG[k]) - t).max() / np.abs(t).max()
        assert np.isfinite(d)
        worst = max(worst, d)
    assert worst <= 1e-13, worst


def ref_cases():
    w64 = pr.weights(64, *pc.LATTICE_RADII)
    yield "lattice", pc.lattice_paths(5), 64, w64, None
    yield "lattice-slice", pc.lattice_paths(5, scaled_slice=3), 64, w64, None
    for n, m, h in ((2, 0, 3), (20, 0, 1), (30, 3, 7)):
        P = pc.random_paths(n + m, h, 100 + n)
        yield f"random{n}+{m}", P, n, pr.weights(n, RXY, RZ, np.linspace(0.0, 1.0, m), np.linspace(1.0, 0.0, m)), None
    a = (np.arange(33) % 3 != 1).astype(np.uint8)
    yield "masked", pc.random_paths(33, 4, 9), 30, pr.weights(30, RXY, RZ, [0.1] * 3, [0.2] * 3), a[:30]


@pytest.mark.parametrize("case", list(ref_cases()), ids=lambda c: c[0])
def test_numpy_reference_equals_scalar_loop(case):
    _, P, n, (wxy, wz), active = case
    for ids in (np.arange(n), np.arange(n)[1::3]):
        a = pr.rows(P, n, wxy, wz, ids, active)
        b = pc.scalar_rows(P, wxy, wz, ids, pr.ROW_DTYPE, active, n)
        assert pc.same_rows(a, b), (a[:3], b[:3])
    if active is None:
        assert a["n_conf"].max() >= 1 or n == 2 or case[0] == "lattice"


def test_per_row_obstacle_columns_equal_shared_ones_with_shared_gains(oracle):
    """With one gains set an obstacle's path does not depend on the row: the
    predicting call's per-row columns equal the same paths given as columns."""
    g = oracle.synthesize()
    import lqro
    x, vg = lqro.synthetic_swarm(8, box=3.0, seed=11)
    obs = lqro.obstacle_states(x[:2, :3] + 0.3, [[0.1, 0.2, 0.0], [0.0, 0.0, 0.1]])
    rows, tot, P = pr.predict(x, vg, g, 10, RXY, RZ, obs=obs, obs_xy=[0.1, 0.2], obs_z=[0.3, 0.4])
    CG, NCF = pr.table_sets(g["A"], g["B"], g["L"], g["E"], 10)
    Po = pr.obstacle_paths(CG, NCF, [0], obs)[0]
    r2, t2 = pr.predict_paths(np.concatenate([P, Po]), 8, RXY, RZ, obs_xy=[0.1, 0.2], obs_z=[0.3, 0.4])
    assert pc.same_rows(rows, r2) and pc.same_total(tot, t2)


def test_tie_rules():
    rxy, rz = pc.LATTICE_RADII
    w = pr.weights(64, rxy, rz)
    r = pr.rows(pc.lattice_paths(4), 64, *w, np.arange(64))
    assert np.all(r["s2_min"] == 1.0) and np.all(r["n_conf"] == 0) and np.all(r["k_s2"] == 0)   # the smallest slice
    assert r["j_s2"][0] == 1 and r["j_s2"][21] == 5 and np.all(r["k_first"] == -1)            # the smallest column
    t = pr.total(r, np.arange(64))
    assert (t["s2_min"], t["s2_i"], t["s2_j"], t["s2_k"]) == (1.0, 0, 1, 0) and t["first_k"] == -1
    r = pr.rows(pc.lattice_paths(4, scaled_slice=2), 64, *w, np.arange(64))
    assert np.all(r["k_first"] == 2) and np.all(r["s2_min"] == 0.5625) and r["n_conf"].min() == 3 and r["n_conf"].max() == 6
    assert all(np.all(np.diff(q["conf"][:min(4, q["n_conf"])]) > 0) for q in r)
    # two bodies on one path: a hit with s2 == 0 at slice 0, self skipped by index
    P = np.tile(pc.random_paths(1, 3, 1), (2, 1, 1))
    r = pr.rows(P, 2, *pr.weights(2, RXY, RZ), np.arange(2))
    assert r["s2_min"].tolist() == [0.0, 0.0] and r["j_s2"].tolist() == [1, 0] and r["k_first"].tolist() == [0, 0]
    # since reset: a later equal value does not replace the earliest; a smaller first slice does
    a = dict(pr.empty_total(), s2_min=0.5, s2_i=3, s2_j=4, s2_k=7, first_k=5, first_i=3, first_j=4, n_conf=2, n_measured=1)
    b = dict(pr.empty_total(), s2_min=0.5, s2_i=0, s2_j=1, s2_k=1, first_k=5, first_i=0, first_j=1, n_conf=1, n_measured=1)
    s = pr.fold(pr.fold(pr.empty_total(), a), b)
    assert (s["s2_i"], s["s2_j"], s["s2_k"], s["first_i"], s["n_conf"], s["n_measured"]) == (3, 4, 7, 3, 3, 2)
    s = pr.fold(s, dict(b, first_k=4))
    assert (s["first_k"], s["first_i"], s["first_j"]) == (4, 0, 1)


def test_exports_structs_and_header(lqro_mod):
    names = ("lqro_predict", "lqro_predict_device", "lqro_predict_paths", "lqro_predict_paths_device",
             "lqro_get_prediction", "lqro_get_prediction_rows", "lqro_get_paths")
    L = ctypes.CDLL(lqro_mod.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "lqro.h")).read()
    for sym in names:
        assert sym in lqro_mod.EXPORTS and getattr(L, sym) is not None and ("int " + sym + "(") in hdr
    assert ctypes.sizeof(lqro_mod.PredictRow) == 64 == lqro_mod.PREDICT_ROW_DTYPE.itemsize
    assert ctypes.sizeof(lqro_mod.PredictTotal) == 80
    assert lqro_mod.PREDICT_ROW_DTYPE == pr.ROW_DTYPE and lqro_mod.PREDICT_TILE == pc.TR
    assert "sizeof(lqro_predict_row) == 64" in hdr and "sizeof(lqro_predict_total) == 80" in hdr
    assert f"#define LQRO_PREDICT_TILE {pc.TR}" in hdr
    assert set(pr.empty_total()) == set(lqro_mod.PREDICT_TOTAL_FIELDS)
    for f in ("predict", "predict_device", "predict_paths", "predict_paths_device", "prediction", "prediction_rows",
              "paths"):
        assert callable(getattr(lqro_mod.Context, f))
    assert callable(lqro_mod.Simulator.predict) and callable(lqro_mod.DeviceLoop.predict)
    assert L.lqro_version() == 5                          # (the symbols identify the feature)
    # a null context is refused before any device call
    lib = lqro_mod.lib()
    n = ctypes.c_int64()
    assert lib.lqro_predict(None, None, None, None, None) == -1
    assert lib.lqro_predict_device(None, None, None, None, None) == -1
    assert lib.lqro_predict_paths(None, None, None, None) == -1
    assert lib.lqro_predict_paths_device(None, None, None, None) == -1
    assert lib.lqro_get_prediction(None, None, None, 0) == -1
    assert lib.lqro_get_prediction_rows(None, None, 0, ctypes.byref(n)) == -1
    assert lib.lqro_get_paths(None, None) == -1


def predict_main() -> str:
    if not os.path.exists(PREDICT_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_predict()
    return PREDICT_MAIN


def write_predict_input(path, x, vg, H, NP):
    with open(path, "wb") as f:
        np.array([x.shape[0], H, NP], np.int32).tofile(f)
        for a in (x, vg):
            np.ascontiguousarray(a, np.float64).tofile(f)


def test_cpp_consumer_fails_loudly_without_gpu(lqro_mod, tmp_path):
    import torch
    exe = predict_main()
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    x, vg = lqro_mod.synthetic_swarm(4, box=3.0, seed=11)
    write_predict_input(tmp_path / "in.bin", x, vg, 10, 20)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["block", "cyclic"])
def test_merge_prediction_over_splits(lqro_mod, world, mode):
    n, m = 65, 3
    P = pc.random_paths(n + m, 6, 77)
    w = pr.weights(n, RXY, RZ, [0.0, 0.5, 1.0], [0.0, 0.5, 1.0])
    whole = pr.total(pr.rows(P, n, *w, np.arange(n)), np.arange(n))
    assert whole["n_conf"] > 0 and whole["first_k"] >= 0
    parts = []
    for rank in range(world):
        ids = lqro_mod.shard_row_ids(n, rank, world, mode)
        parts.append(pr.total(pr.rows(P, n, *w, ids), ids))
    assert pc.same_total(lqro_mod.merge_prediction(parts), whole)
    assert pc.same_total(lqro_mod.merge_prediction([]), pr.empty_total())


def test_kernels_keep_no_private_memory():
    from test_codeobj import _kernels, _tools
    _tools()
    ks = _kernels()
    names = {w: [k for k in ks if w in k] for w in ("9k_pred_cg", "12k_pred_paths", "9k_pred_tr", "6k_conf8",
                                                    "10k_conf_obs", "12k_conf_total")}
    assert all(names.values()), sorted(ks)[:20]
    for k in sum(names.values(), []):
        assert ks[k].get("private_segment_fixed_size", -1) == 0, (k, ks[k])
    for k in names["6k_conf8"]:   # (the rows' paths are dynamic LDS on top of this)
        assert 0 < ks[k].get("group_segment_fixed_size", 0) <= 16 * 1024, (k, ks[k])


# the link to the method -----------------------------------------------------
@pytest.mark.parametrize("n,box,seed,h", [(24, 3.0, 11, 50), (24, 3.0, 12, 50), (64, 6.0, 11, 100)])
def test_a_later_hit_well_inside_is_a_pair_the_step_classed_inside(oracle, gains, lqro_mod, n, box, seed, h):
    """Golden gains, shared, v = x[:, 3:6] (the velocity the step itself
    tests): every pair whose first hit is at a slice >= 1 and whose s2_min <
    0.9 carries LQRO_REC_INSIDE in pyoracle.step's record.  The unflagged pairs
    with a later hit sit at s2_min >= 0.959 on these swarms (the 100-point
    hull is inscribed); hits at slice 0 are bodies already overlapping, whose
    slice is out of reach."""
    x, vg = lqro_mod.synthetic_swarm(n, box=box, seed=seed)
    T, NCF = oracle.tables(gains["A"], gains["B"], gains["L"], gains["E"], h)
    _, recs = oracle.step(T, NCF, oracle.sphere(100), x, vg, threads=4)
    inside = ((recs["flags"] & lqro_mod.REC_INSIDE) != 0).reshape(n, n - 1)
    rows, tot, P = pr.predict(x, x[:, 3:6], gains, h, RXY, RZ)
    S = pr.pair_s2(P, *pr.weights(n, RXY, RZ))
    later, unflagged = 0, []
    for i in range(n):
        for q in range(n - 1):
            j = q + (q >= i)
            hit = np.nonzero(S[i, j] < 1.0)[0]
            if len(hit) == 0 or hit[0] == 0:
                continue
            later += 1
            if not inside[i, q]:
                unflagged.append(float(S[i, j].min()))
                assert S[i, j].min() >= 0.9, (i, j, S[i, j].min())
    assert later > 0 and all(v >= 0.959 for v in unflagged), unflagged
    assert tot["n_conf"] >= later


def test_swap_scenario(oracle, gains, lqro_mod):
    """The scripted 4-quad swap at 2 m/s toward the goals, H = 100: every
    agent has three conflicts; the ordered restatement puts the crossing
    pairs' first hit at slice 67 and the opposite pair's at 69."""
    x, goal = lqro_mod.swap_scenario()
    d = goal - x[:, :3]
    v = 2.0 * d / np.linalg.norm(d, axis=1)[:, None]
    rows, tot, P = pr.predict(x, v, gains, 100, RXY, RZ)
    assert rows["n_conf"].tolist() == [3, 3, 3, 3]
    assert rows["conf"].tolist() == [[1, 2, 3, -1], [0, 2, 3, -1], [0, 1, 3, -1], [0, 1, 2, -1]]
    assert rows["k_first"].tolist() == [67] * 4 and rows["j_first"].tolist() == [2, 2, 0, 0]
    S = pr.pair_s2(P, *pr.weights(4, RXY, RZ))
    first = [[int(np.nonzero(S[i, j] < 1.0)[0][0]) for j in range(4) if j != i] for i in range(4)]
    assert first == [[69, 67, 67], [69, 67, 67], [67, 67, 69], [67, 67, 69]]
    assert (tot["first_k"], tot["first_i"], tot["first_j"], tot["n_conf"], tot["n_rows_conf"]) == (67, 0, 2, 12, 4)
