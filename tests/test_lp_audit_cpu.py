"""The LP audit's CPU side: the numpy reference against a plain
scalar loop, the tie rules and that the tie inputs tell wrong rules apart, the
exports, struct sizes and header text, merge_lp_audit over row splits, the C++
consumer without a device, and the two kernels' descriptors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lp_audit_cases as ac
import lp_audit_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIT_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_audit_main")
F = np.float32
NINF = F(-np.inf)


def scalar_rows(lists, newv, vgoal, tol, row_ids=None):
    """lqro.h's formulas as a plain loop over np.float32 scalars."""
    row_ids = range(len(lists)) if row_ids is None else [int(i) for i in row_ids]
    out = np.zeros(len(lists), ar.ROW_DTYPE)
    tol = F(tol)
    with np.errstate(all="ignore"):
        for r, (c, i) in enumerate(zip(lists, row_ids)):
            v = [F(newv[i][q]) for q in range(3)]
            pref = [F(vgoal[i][q]) for q in range(3)]
            m = len(c["planes"])
            n_hard = min(int(c["n_hard"]), m)
            best, hbest = (NINF, -1), (NINF, -1)
            n_viol = n_tol = n_hard_tol = 0
            for k in range(m):
                p = [F(c["planes"][k][q]) for q in range(6)]
                viol = p[3] * (p[0] - v[0])
                viol = viol + p[4] * (p[1] - v[1])
                viol = viol + p[5] * (p[2] - v[2])
                assert type(viol) is np.float32
                if best[1] < 0 or viol > best[0]:
                    best = (viol, k)
                if k < n_hard and (hbest[1] < 0 or viol > hbest[0]):
                    hbest = (viol, k)
                n_viol += bool(viol > F(0.0))
                n_tol += bool(viol > tol)
                n_hard_tol += bool(k < n_hard and viol > tol)
            v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            d = [v[q] - pref[q] for q in range(3)]
            dv2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]

            def src(k):
                return (k, int(c["kind"][k]), int(c["id"][k])) if k >= 0 else (-1, -1, -1)
            out[r] = (best[0], hbest[0], v2, dv2, i, m, n_hard, n_viol, n_tol, n_hard_tol, *src(best[1]), *src(hbest[1]))
    return out


def ref_cases():
    lists, goals, nh, vel = ac.wave_rows()
    yield "wave_edges", ar.plain_lists(lists, nh), goals, vel
    lists, goals, nh, vel = ac.few_planes(257)
    yield "few_planes", ar.plain_lists(lists, nh), goals, vel
    ties = ac.tie_rows()
    yield "ties", ar.plain_lists([c for c, _ in ties.values()], [h for _, h in ties.values()]), \
        np.zeros((len(ties), 3)), np.tile(ac.V0, (len(ties), 1))
    lists, goals, nh, vel = ac.equal_rows()
    yield "equal_rows", ar.plain_lists(lists, nh), goals, vel
    # a step-like list: kinds and ids of all three sources
    rng = np.random.default_rng(8)
    lists, goals, _, vel = ac.few_planes(12, seed=9)
    mixed = []
    for c in lists:
        m = len(c)
        mixed.append(dict(planes=c, n_hard=int(rng.integers(0, m + 2)), kind=rng.integers(0, 3, size=m).astype(np.int32),
                          id=rng.integers(0, 40, size=m).astype(np.int32)))
    yield "mixed_kinds", mixed, goals, vel


@pytest.mark.parametrize("case", list(ref_cases()), ids=lambda c: c[0])
def test_numpy_reference_equals_scalar_loop(case):
    _, lists, goals, vel = case
    for tol in (0.0, ac.TOL):
        a = ar.rows(lists, vel, goals, tol)
        b = scalar_rows(lists, vel, goals, tol)
        assert ar.same_rows(a, b), np.nonzero(a != b)[0][:8]
    ids = np.arange(len(lists))[::-1].copy()           # rows name global agents
    a = ar.rows(lists, vel, goals, ac.TOL, ids)
    assert ar.same_rows(a, scalar_rows(lists, vel, goals, ac.TOL, ids)) and np.array_equal(a["i"], ids)


def _tie_records(tie):
    ties = ac.tie_rows()
    lists = ar.plain_lists([c for c, _ in ties.values()], [h for _, h in ties.values()])
    r = ar.rows(lists, np.tile(ac.V0, (len(ties), 1)), np.zeros((len(ties), 3)), ac.TOL, tie=tie)
    return dict(zip(ties, r))


def test_tie_rules():
    r = _tie_records("lowest")
    a = r["same_lane"]
    assert (a["viol_max"], a["k_viol"], a["id_viol"], a["n_viol"], a["n_viol_tol"]) == (2.0, 3, 3, 3, 3)
    assert (a["n_hard"], a["k_hard"], a["kind_hard"], a["id_hard"]) == (0, -1, -1, -1) and a["hard_viol_max"] == NINF
    a = r["neighbours"]
    assert (a["viol_max"], a["k_viol"], a["n_viol"]) == (2.0, 5, 2)
    a = r["prefix_between"]
    assert (a["k_viol"], a["n_hard"], a["k_hard"], a["hard_viol_max"], a["n_hard_viol"]) == (4, 6, 4, 2.0, 2)
    a = r["signed_zero"]
    assert (a["k_viol"], a["k_hard"], a["n_viol"], a["n_viol_tol"]) == (2, 2, 0, 0)
    assert a["viol_max"].view(np.uint32) == 0x80000000 and a["viol_max"] == 0.0     # -0 equals +0: the lowest k, its bits
    # the inputs tell the rules apart: "highest k wins" and a >= in the lane's running maximum give other records
    hi, ge = _tie_records("highest"), _tie_records("lane_ge")
    assert (hi["same_lane"]["k_viol"], ge["same_lane"]["k_viol"]) == (131, 131)
    assert hi["neighbours"]["k_viol"] == 6
    assert (hi["prefix_between"]["k_viol"], hi["prefix_between"]["k_hard"]) == (6, 5)
    assert hi["signed_zero"]["k_viol"] == 9 and hi["signed_zero"]["viol_max"].view(np.uint32) == 0
    for name in r:
        assert not ar.same_rows(r[name].reshape(1), hi[name].reshape(1)), name
    assert not ar.same_rows(r["same_lane"].reshape(1), ge["same_lane"].reshape(1))
    # two rows with an equal maximum: the total takes the smaller i, then the smaller k
    lists, goals, nh, vel = ac.equal_rows()
    rows = ar.rows(ar.plain_lists(lists, nh), vel, goals, ac.TOL)
    assert rows["viol_max"].tolist() == [1.0, 2.0, -np.inf, 2.0] and rows["k_viol"].tolist() == [7, 66, -1, 66]
    t = ar.total(rows)
    assert (t["viol_max"], t["viol_i"], t["viol_k"], t["viol_kind"], t["viol_id"]) == (2.0, 1, 66, ar.USER, 66)
    assert (t["hard_viol_max"], t["hard_i"], t["hard_k"]) == (2.0, 3, 66)          # row 1 has no hard prefix
    assert (t["n_rows_viol"], t["n_rows_hard_viol"], t["n_viol_tol"], t["n_planes"], t["n_measured"]) == (3, 2, 3, 152, 1)
    assert t["dv2_i"] == 0                                                          # four equal dv2: the smallest i
    # an empty total; since reset: a later equal maximum does not replace the earliest
    e = ar.total(rows[2:3])
    assert e["viol_max"] == NINF and (e["viol_i"], e["viol_k"], e["hard_i"]) == (-1, -1, -1) and e["dv2_i"] == 2
    a = dict(ar.empty_total(), viol_max=F(0.5), viol_i=3, viol_k=4, viol_kind=2, viol_id=9, n_viol_tol=2, n_measured=1)
    b = dict(ar.empty_total(), viol_max=F(0.5), viol_i=0, viol_k=1, viol_kind=0, viol_id=1, n_viol_tol=1, n_measured=1)
    s = ar.fold(ar.fold(ar.empty_total(), a), b)
    assert (s["viol_i"], s["viol_k"], s["viol_id"], s["n_viol_tol"], s["n_measured"]) == (3, 4, 9, 3, 2)
    assert s["hard_viol_max"] == NINF and s["hard_i"] == -1


def test_exports_structs_and_header(lqro_mod):
    names = ("lqro_set_lp_audit", "lqro_get_lp_audit", "lqro_get_lp_audit_rows", "lqro_audit_new_v")
    L = ctypes.CDLL(lqro_mod.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "lqro.h")).read()
    for sym in names:
        assert sym in lqro_mod.EXPORTS and getattr(L, sym) is not None and ("int " + sym + "(") in hdr
    assert ctypes.sizeof(lqro_mod.LpRow) == 64 == lqro_mod.LP_ROW_DTYPE.itemsize
    assert ctypes.sizeof(lqro_mod.LpTotal) == 88
    assert lqro_mod.LP_ROW_DTYPE == ar.ROW_DTYPE
    assert set(lqro_mod.LP_TOTAL_FIELDS) == set(ar.empty_total())
    assert "sizeof(lqro_lp_row) == 64" in hdr and "sizeof(lqro_lp_total) == 88" in hdr
    assert "LQRO_AUDIT_FENCE = 0, LQRO_AUDIT_USER = 1, LQRO_AUDIT_COLUMN = 2" in hdr
    assert (lqro_mod.LQRO_AUDIT_FENCE, lqro_mod.LQRO_AUDIT_USER, lqro_mod.LQRO_AUDIT_COLUMN) == \
        (ar.FENCE, ar.USER, ar.COLUMN) == (0, 1, 2)
    assert L.lqro_version() == 5                       # callers detect the feature by the symbol
    for f in ("set_lp_audit", "lp_audit", "lp_audit_rows"):
        assert callable(getattr(lqro_mod.Context, f))
    assert callable(lqro_mod.audit_new_v) and callable(lqro_mod.merge_lp_audit)
    assert callable(lqro_mod.Simulator.set_lp_audit) and callable(lqro_mod.Simulator.lp_audit)
    assert callable(lqro_mod.DeviceLoop.lp_audit)
    sim = open(os.path.join(ROOT, "include", "lqro_sim.hpp")).read()
    assert "void set_lp_audit(" in sim and "lqro_lp_total lp_audit(" in sim
    # refused before any device call: a null context, and the context-free call's bad arguments
    lib = lqro_mod.lib()
    n = ctypes.c_int64()
    assert lib.lqro_set_lp_audit(None, 1, 0.0) == -1
    assert lib.lqro_get_lp_audit(None, None, None, 0) == -1
    assert lib.lqro_get_lp_audit_rows(None, None, 0, ctypes.byref(n)) == -1
    pl, offs = np.zeros((1, 6), np.float32), np.array([0, 1], np.int64)
    vg, nv = np.zeros((1, 3)), np.zeros((1, 3))
    p = lqro_mod._p
    good = [p(pl), p(offs), None, 1, p(vg), p(nv), 0.0, None, None, 0]
    for k, bad in ((0, None), (1, None), (4, None), (5, None), (3, 0), (6, -1.0), (6, float("inf")), (6, float("nan")),
                   (2, p(np.array([-1], np.int32))), (1, p(np.array([1, 0], np.int64)))):
        a = list(good)
        a[k] = bad
        assert lib.lqro_audit_new_v(*a) == -1, (k, bad)


def test_no_device_fails_loudly(lqro_mod):
    import torch
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu tests cover the run)
    with pytest.raises(lqro_mod.LqroError):
        lqro_mod.audit_new_v([np.zeros((1, 6), np.float32)], np.zeros((1, 3)), np.zeros((1, 3)))


def audit_main() -> str:
    if not os.path.exists(AUDIT_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_audit()
    return AUDIT_MAIN


def write_audit_input(path, x, vg, H, NP, steps, tol, hard=0, lo=None, hi=None, tau=1.0):
    with open(path, "wb") as f:
        np.array([x.shape[0], H, NP, steps, 0 if lo is None else 1, hard], np.int32).tofile(f)
        np.array([tol], np.float32).tofile(f)
        for a in (x, vg, np.zeros(3) if lo is None else lo, np.zeros(3) if hi is None else hi, [tau]):
            np.ascontiguousarray(a, np.float64).tofile(f)


def test_cpp_consumer_fails_loudly_without_gpu(lqro_mod, tmp_path):
    import torch
    exe = audit_main()
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    x, vg = lqro_mod.synthetic_swarm(8, box=3.0, seed=11)
    write_audit_input(tmp_path / "in.bin", x, vg, 10, 20, 1, ac.TOL)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["block", "cyclic"])
def test_merge_lp_audit_over_splits(lqro_mod, world, mode):
    lists, goals, nh, vel = ac.few_planes(65)
    eq, _, enh, _ = ac.equal_rows()
    for k, i in enumerate((60, 7, 33, 8)):             # equal maxima in different shards
        lists[i], nh[i], vel[i] = eq[k], enh[k], ac.V0
    all_lists = ar.plain_lists(lists, nh)
    whole = ar.total(ar.rows(all_lists, vel, goals, ac.TOL))
    assert whole["n_rows_viol"] > 0 and whole["n_rows_hard_viol"] > 0
    parts = []
    for rank in range(world):
        ids = lqro_mod.shard_row_ids(65, rank, world, mode)
        parts.append(ar.total(ar.rows([all_lists[i] for i in ids], vel, goals, ac.TOL, ids)))
    assert ar.same_total(lqro_mod.merge_lp_audit(parts), whole)
    assert ar.same_total(lqro_mod.merge_lp_audit(parts[::-1]), whole)
    assert ar.same_total(lqro_mod.merge_lp_audit([]), ar.empty_total())


def test_audit_kernels_keep_no_private_memory_and_k_lp_audit_no_lds():
    from test_codeobj import _kernels, _tools
    _tools()
    ks = _kernels()
    names = {w: [k for k in ks if w in k] for w in ("10k_lp_audit6LpArgs", "16k_lp_audit_total")}
    assert all(len(v) == 1 for v in names.values()), sorted(ks)[:20]
    for k in sum(names.values(), []):
        assert ks[k].get("private_segment_fixed_size", -1) == 0, (k, ks[k])
    k = names["10k_lp_audit6LpArgs"][0]
    assert ks[k].get("group_segment_fixed_size", -1) == 0, (k, ks[k])
    k = names["16k_lp_audit_total"][0]
    assert 0 < ks[k].get("group_segment_fixed_size", 0) <= 64 * 1024, (k, ks[k])
