"""The clearance measurement's CPU side: the numpy reference
against a plain scalar loop, the tie rules, the exports and struct sizes, the
C++ consumer without a device, merge_clearance over row splits, and k_clear's
kernel descriptor (no private memory)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clearance_cases as cc
import clearance_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAR_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_clear_main")
INF = float("inf")


def scalar_rows(pos, wxy, wz, row_ids, faces=()):
    """lqro.h's formulas as a plain loop over Python floats."""
    pos = [[float(v) for v in p] for p in pos]
    wxy, wz = [float(v) for v in wxy], [float(v) for v in wz]
    out = np.zeros(len(row_ids), cr.ROW_DTYPE)
    for r, i in enumerate(int(v) for v in row_ids):
        s2m, d2m, js, jd, nh, hits = INF, INF, -1, -1, 0, []
        for c in range(len(pos)):
            if c == i:
                continue
            dx = pos[i][0] - pos[c][0]
            dy = pos[i][1] - pos[c][1]
            dz = pos[i][2] - pos[c][2]
            q = dx * dx + dy * dy
            zz = dz * dz
            d2 = q + zz
            s2 = q * wxy[c] + zz * wz[c]
            if s2 < s2m:
                s2m, js = s2, c
            if d2 < d2m:
                d2m, jd = d2, c
            if s2 < 1.0:
                nh += 1
                hits.append(c)
        fm, ff = INF, -1
        for face, a, side, bound in faces:
            g = pos[i][a] - float(bound) if side == 0 else float(bound) - pos[i][a]
            if g < fm:
                fm, ff = g, face
        out[r] = (s2m, d2m, fm, js, jd, nh, ff, (hits[:6] + [-1] * 6)[:6])
    return out


def ref_cases():
    yield "lattice", cc.lattice(1.0), cc.LATTICE_RADII, (), (), None, None
    yield "lattice075", cc.lattice(0.75), cc.LATTICE_RADII, (), (), None, None
    for n, m in ((2, 0), (63, 0), (65, 3), (257, 8)):
        p = cc.random_positions(n + m, 100 + n)
        oxy = np.linspace(0.0, 1.0, m)
        oz = np.linspace(1.0, 0.0, m)
        yield f"random{n}+{m}", p, (0.26, 0.75), oxy, oz, [-2.0, -INF, -1.5], [2.5, 3.0, INF]
    yield "cluster", np.concatenate([cc.cluster(9, 5), cc.random_positions(20, 6)]), (0.26, 0.75), (), (), None, None


@pytest.mark.parametrize("case", list(ref_cases()), ids=lambda c: c[0])
def test_numpy_reference_equals_scalar_loop(case):
    _, pos, (rxy, rz), oxy, oz, lo, hi = case
    n = len(pos) - len(oxy)
    wxy, wz = cr.weights(n, rxy, rz, oxy, oz)
    faces = cr.fence_faces(lo, hi, rxy, rz)
    for ids in (np.arange(n), np.arange(n)[1::3]):
        a = cr.rows(pos, wxy, wz, ids, faces)
        b = scalar_rows(pos, wxy, wz, ids, faces)
        assert cc.same_rows(a, b)


def test_lattice_is_an_exact_border():
    wxy, wz = cr.weights(64, *cc.LATTICE_RADII)
    assert np.all(wxy == 1.0) and np.all(wz == 4.0)
    r = cr.rows(cc.lattice(1.0), wxy, wz, np.arange(64))
    assert np.all(r["s2_min"] == 1.0) and np.all(r["n_hit"] == 0)
    r = cr.rows(cc.lattice(0.75), wxy, wz, np.arange(64))
    assert np.all(r["s2_min"] == 0.5625) and np.array_equal(r["n_hit"], cc.lattice_axis_neighbours())


def test_tie_rules():
    # four agents on a unit square (radii 0.5, 0.25: a = 1): each has two neighbours at s2 == 1
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float64)
    wxy, wz = cr.weights(4, *cc.LATTICE_RADII)
    r = cr.rows(pos, wxy, wz, np.arange(4))
    assert r["j_s2"].tolist() == [1, 0, 0, 1] and r["j_d2"].tolist() == [1, 0, 0, 1]   # the smallest column of equals
    assert r["n_hit"].tolist() == [0, 0, 0, 0]                                        # s2 == 1.0 is no hit
    t = cr.total(r, np.arange(4))
    assert (t["s2_min"], t["s2_i"], t["s2_j"]) == (1.0, 0, 1) and t["n_measured"] == 1
    # two agents at one point: a hit with s2 == 0, self skipped by index
    r = cr.rows(np.zeros((2, 3)), *cr.weights(2, 0.26, 0.75), np.arange(2))
    assert r["s2_min"].tolist() == [0.0, 0.0] and r["j_s2"].tolist() == [1, 0] and r["hit"][:, 0].tolist() == [1, 0]
    # the fence: on a face is 0.0 and not out; two faces at the same margin: the lower index
    faces = cr.fence_faces([0.0, 0.0, 0.0], [4.0, 4.0, 4.0], 0.5, 0.25)
    p = np.array([[0.5, 2.0, 2.0], [1.0, 1.0, 2.0], [0.25, 2.0, 2.0], [2.0, 2.0, 3.5]])
    r = cr.rows(p, *cr.weights(4, 0.5, 0.25), np.arange(4), faces)
    assert r["fence_min"].tolist() == [0.0, 0.5, -0.25, 0.25] and r["fence_face"].tolist() == [0, 0, 0, 5]
    t = cr.total(r, np.arange(4))
    assert t["n_fence_out"] == 1 and (t["fence_min"], t["fence_i"], t["fence_face"]) == (-0.25, 2, 0)
    # since reset: a later equal minimum does not replace the earliest
    a = dict(cr.empty_total(), s2_min=0.5, s2_i=3, s2_j=4, n_hit=2, n_measured=1)
    b = dict(cr.empty_total(), s2_min=0.5, s2_i=0, s2_j=1, n_hit=1, n_measured=1)
    s = cr.fold(cr.fold(cr.empty_total(), a), b)
    assert (s["s2_i"], s["s2_j"], s["n_hit"], s["n_measured"]) == (3, 4, 3, 2)


def test_exports_structs_and_header(lqro_mod):
    names = ("lqro_clearance", "lqro_clearance_device", "lqro_set_monitor", "lqro_get_monitor",
             "lqro_get_monitor_rows", "lqro_get_monitor_pairs")
    L = ctypes.CDLL(lqro_mod.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "lqro.h")).read()
    for sym in names:
        assert sym in lqro_mod.EXPORTS and getattr(L, sym) is not None and ("int " + sym + "(") in hdr
    assert ctypes.sizeof(lqro_mod.ClearanceRow) == 64 == lqro_mod.CLEARANCE_ROW_DTYPE.itemsize
    assert ctypes.sizeof(lqro_mod.ClearanceTotal) == 80
    assert lqro_mod.CLEARANCE_ROW_DTYPE == cr.ROW_DTYPE
    assert "sizeof(lqro_clearance_row) == 64" in hdr and "sizeof(lqro_clearance_total) == 80" in hdr
    for f in ("clearance", "clearance_device", "set_monitor", "monitor", "monitor_rows", "monitor_pairs"):
        assert callable(getattr(lqro_mod.Context, f))
    assert callable(lqro_mod.Simulator.clearance) and callable(lqro_mod.DeviceLoop.monitor)
    # a null context is refused before any device call
    lib = lqro_mod.lib()
    n = ctypes.c_int64()
    assert lib.lqro_clearance(None, None, None, None) == -1
    assert lib.lqro_clearance_device(None, None, None, None) == -1
    assert lib.lqro_set_monitor(None, 1) == -1
    assert lib.lqro_get_monitor(None, None, None, 0) == -1
    assert lib.lqro_get_monitor_rows(None, None, 0, ctypes.byref(n)) == -1
    assert lib.lqro_get_monitor_pairs(None, None, 0, ctypes.byref(n)) == -1


def clear_main() -> str:
    if not os.path.exists(CLEAR_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_clear()
    return CLEAR_MAIN


def write_clear_input(path, x, H, NP, obs, oxy, oz, lo=None, hi=None):
    with open(path, "wb") as f:
        np.array([x.shape[0], H, NP, len(obs), 0 if lo is None else 1], np.int32).tofile(f)
        for a in (x, obs, oxy, oz, np.zeros(3) if lo is None else lo, np.zeros(3) if hi is None else hi):
            np.ascontiguousarray(a, np.float64).tofile(f)


def test_cpp_consumer_fails_loudly_without_gpu(lqro_mod, tmp_path):
    import torch
    exe = clear_main()
    if torch.cuda.device_count() > 0:
        return   # (the -m gpu test covers the run)
    write_clear_input(tmp_path / "in.bin", cc.states(cc.lattice()), 10, 20, cc.states(np.ones((2, 3))), [0.0, 1.0],
                      [0.0, 1.0])
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["block", "cyclic"])
def test_merge_clearance_over_splits(lqro_mod, world, mode):
    n, m = 65, 3
    pos = np.concatenate([cc.cluster(9, 5), cc.random_positions(n - 9 + m, 77)])
    wxy, wz = cr.weights(n, 0.26, 0.75, [0.0, 0.5, 1.0], [0.0, 0.5, 1.0])
    faces = cr.fence_faces([-1.0, -1.0, -1.0], [1.5, 1.5, 1.5], 0.26, 0.75)
    whole = cr.total(cr.rows(pos, wxy, wz, np.arange(n), faces), np.arange(n))
    assert whole["n_hit"] > 0 and whole["n_fence_out"] > 0
    parts = []
    for rank in range(world):
        ids = lqro_mod.shard_row_ids(n, rank, world, mode)
        parts.append(cr.total(cr.rows(pos, wxy, wz, ids, faces), ids))
    assert cc.same_total(lqro_mod.merge_clearance(parts), whole)
    assert cc.same_total(lqro_mod.merge_clearance([]), cr.empty_total())


def test_k_clear_keeps_no_private_memory():
    from test_codeobj import _kernels, _tools
    _tools()
    ks = _kernels()
    names = {w: [k for k in ks if w in k] for w in ("12k_clear_pack", "7k_clear9", "13k_clear_total")}
    assert all(names.values()), sorted(ks)[:20]
    for k in sum(names.values(), []):
        assert ks[k].get("private_segment_fixed_size", -1) == 0, (k, ks[k])
    for k in names["7k_clear9"]:
        assert 0 < ks[k].get("group_segment_fixed_size", 0) <= 64 * 1024, (k, ks[k])
