"""The horizon conflict prediction on the GPU (lqro_predict[_device],
lqro_predict_paths[_device]), bit for bit against
tests/predict_ref.py's numpy restatement of lqro.h's formulas."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import predict_cases as pc
import predict_ref as pr

pytestmark = pytest.mark.gpu

H, NP = 10, 20
RXY, RZ = 0.26, 0.75    # lqro_config_default's radii
INF = float("inf")
E_ARG, E_STATE = -1, -4


def mk(lqro, n, gains=None, per_agent=False, **kw):
    ctx = lqro.Context(lqro.config(n, kw.pop("h", H), kw.pop("npts", NP), **kw))
    if gains is not None:
        ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"], per_agent=per_agent)
    return ctx


def same(ctx, got, want_rows, want_total, what=""):
    rows, tot = got
    assert pc.same_rows(rows, want_rows), (what, np.nonzero(rows != want_rows)[0][:8], rows[:4], want_rows[:4])
    assert pc.same_total(tot, want_total), (what, tot, want_total)
    assert pc.same_total(ctx.prediction()[0], want_total), what
    assert pc.same_rows(ctx.prediction_rows(), want_rows), what
    return rows, tot


def per_agent_gains(lqro, n, x_dim):
    g = lqro.synthesize_gains_batch(lqro.perturbed_models(n), x_dim=x_dim)
    ab = lqro.synthesize_gains(x_dim=x_dim)
    return dict(A=ab["A"], B=ab["B"], L=g["L"], E=g["E"])


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["shared-h10", "shared-h256", "per-agent-x12"])
def test_paths_alone(lqro_mod, gains, case):
    n = 8
    h = 256 if case == "shared-h256" else H
    xd = 12 if case == "per-agent-x12" else 16
    pa = case == "per-agent-x12"
    g = per_agent_gains(lqro_mod, n, xd) if pa else gains
    x, vg = lqro_mod.synthetic_swarm(n, x_dim=xd, box=3.0, seed=11)
    ctx = mk(lqro_mod, n, g, pa, h=h, x_dim=xd)
    want_rows, want_tot, P = pr.predict(x, vg, g, h, RXY, RZ)
    same(ctx, ctx.predict(x, vg), want_rows, want_tot, case)
    got = ctx.paths()
    assert got.shape == (n, h, 3) and got.tobytes() == P.tobytes(), np.abs(got - P).max()
    ctx.close()


# 2 ------------------------------------------------------------------------
def test_exact_border_through_given_paths(lqro_mod):
    rxy, rz = pc.LATTICE_RADII
    ctx = mk(lqro_mod, 64, xy_radius=rxy, z_radius=rz)
    P = pc.lattice_paths(H)
    want, tot = pr.predict_paths(P, 64, rxy, rz)
    rows, got = same(ctx, ctx.predict_paths(P), want, tot, "lattice")
    # every axis neighbour sits at s2 == 1.0 in every slice: no hit, slice 0, the smallest tied column
    assert np.all(rows["s2_min"] == 1.0) and np.all(rows["n_conf"] == 0) and np.all(rows["conf"] == -1)
    assert np.all(rows["k_s2"] == 0) and np.all(rows["k_first"] == -1) and np.all(rows["j_first"] == -1)
    assert rows["j_s2"][0] == 1 and rows["j_s2"][21] == 5 and got["n_conf"] == 0 and got["first_k"] == -1
    ks = 6
    P = pc.lattice_paths(H, scaled_slice=ks)
    want, tot = pr.predict_paths(P, 64, rxy, rz)
    rows, got = same(ctx, ctx.predict_paths(P), want, tot, "one slice x 0.75")
    import clearance_cases as cc
    nb = cc.lattice_axis_neighbours()
    assert np.all(rows["k_first"] == ks) and np.all(rows["k_s2"] == ks) and np.all(rows["s2_min"] == 0.5625)
    assert np.array_equal(rows["n_conf"], nb) and nb.min() == 3 and nb.max() == 6
    for r in rows:
        c = r["conf"][:min(4, r["n_conf"])]
        assert np.all(np.diff(c) > 0) and np.all(c >= 0) and np.all(r["conf"][len(c):] == -1) and r["j_first"] == c[0]
    assert got["n_conf"] == int(nb.sum()) and got["n_rows_conf"] == 64 and got["first_k"] == ks
    ctx.close()


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [2, 63, 64, 65, 255, 256, 257, 513])
def test_column_pass_and_row_tile_borders(lqro_mod, ncols):
    m = 3 if ncols in (65, 257, 513) else 0
    n = ncols - m
    P = pc.random_paths(ncols, H, 2000 + ncols)
    oxy, oz = [0.0, 0.5, 1.0][:m], [1.0, 0.25, 0.0][:m]
    want, _ = pr.predict_paths(P, n, RXY, RZ, obs_xy=oxy, obs_z=oz)
    assert want["n_conf"].max() >= 1 or ncols == 2
    for rb, re in pc.row_windows(n):
        ctx = mk(lqro_mod, n, row_begin=rb, row_end=re)
        if m:
            ctx.set_obstacles(pc.states(P[n:, 0]), oxy, oz)
        ids = np.arange(rb, re)
        same(ctx, ctx.predict_paths(P), want[ids], pr.total(want[ids], ids), (ncols, rb, re))
        ctx.close()


@pytest.mark.parametrize("h", [1, 256])
def test_horizon_1_and_256(lqro_mod, h):
    n = 70
    P = pc.random_paths(n, h, 31 + h)
    want, tot = pr.predict_paths(P, n, RXY, RZ)
    assert tot["n_conf"] > 0
    ctx = mk(lqro_mod, n, h=h)
    same(ctx, ctx.predict_paths(P), want, tot, h)
    ctx.close()


def test_six_conflicts_and_two_bodies_on_one_path(lqro_mod):
    n = 300
    P = pc.random_paths(n, H, 5, clusters=0)
    P[:, :, 0] += 40.0 * np.arange(n)[:, None]          # nobody near anybody
    ring = [3, 70, 130, 131, 255, 256, 299]             # 3 and six others that cross its path, at slices of their own
    for q, c in enumerate(ring[1:]):
        P[c] = P[3] + 50.0
        P[c, 2 + q] = P[3, 2 + q] + [0.1, 0.0, 0.05]
    P[17] = P[200]                                      # two bodies on one path
    want, tot = pr.predict_paths(P, n, RXY, RZ)
    assert want["n_conf"][3] == 6 and want["conf"][3].tolist() == ring[1:5] and want["k_first"][3] == 2
    assert want["s2_min"][17] == 0.0 and want["j_s2"][17] == 200 and want["k_s2"][17] == 0 and want["k_first"][17] == 0
    assert want["j_s2"][200] == 17 and want["n_conf"][200] == 1
    ctx = mk(lqro_mod, n)
    same(ctx, ctx.predict_paths(P), want, tot)
    ctx.close()


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("pa", [False, True], ids=["shared", "per-agent-x12"])
def test_obstacles_in_the_predicting_calls(lqro_mod, gains, pa):
    n, m = 8, 3
    xd = 12 if pa else 16
    g = per_agent_gains(lqro_mod, n, xd) if pa else gains
    x, vg = lqro_mod.synthetic_swarm(n, x_dim=xd, box=4.0, seed=11)
    oxy, oz = [0.0, 1.0, 0.5], [0.0, 1.0, 0.25]
    opos = np.array([[5.0, 5.0, 5.0], [-3.0, 2.0, 1.0], [0.5, 0.5, 0.5]])
    ovel = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 0.0], [0.0, 0.0, 0.125]])
    opos[0] = x[2, :3] + 0.4 * vg[2]                    # an obstacle on agent 2's path
    obs = lqro_mod.obstacle_states(opos, ovel, x_dim=xd)
    ctx = mk(lqro_mod, n, g, pa, x_dim=xd)
    w0 = pr.predict(x, vg, g, H, RXY, RZ)
    same(ctx, ctx.predict(x, vg), w0[0], w0[1], "no obstacles")
    ctx.set_obstacles(obs, oxy, oz)
    w = pr.predict(x, vg, g, H, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz)
    rows, _ = same(ctx, ctx.predict(x, vg), w[0], w[1], "host obstacles")
    assert n in rows["conf"][2] and (rows["j_s2"] >= n).any()
    assert ctx.paths().tobytes() == w[2].tobytes()
    # a device tensor rewritten between two calls: the second prediction sees the new states
    d_obs = torch.from_numpy(obs.copy()).cuda()
    ctx.set_obstacles(d_obs, oxy, oz)
    same(ctx, ctx.predict(x, vg), w[0], w[1], "device obstacles")
    obs2 = obs.copy()
    obs2[:, :3] = opos[::-1] + 0.125
    d_obs.copy_(torch.from_numpy(obs2))
    torch.cuda.synchronize()
    w2 = pr.predict(x, vg, g, H, RXY, RZ, obs=obs2, obs_xy=oxy, obs_z=oz)
    assert not pc.same_rows(w2[0], w[0])
    same(ctx, ctx.predict(x, vg), w2[0], w2[1], "rewritten")
    # fewer obstacles, then none
    ctx.set_obstacles(obs[:2], oxy[:2], oz[:2])
    w = pr.predict(x, vg, g, H, RXY, RZ, obs=obs[:2], obs_xy=oxy[:2], obs_z=oz[:2])
    same(ctx, ctx.predict(x, vg), w[0], w[1], "two obstacles")
    ctx.set_obstacles(None)
    same(ctx, ctx.predict(x, vg), w0[0], w0[1], "cleared")
    ctx.close()


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["half", "none", "one", "two"])
def test_activity_mask(lqro_mod, gains, mask):
    n, m = 24, 2
    x, vg = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    a = np.zeros(n, np.uint8)
    a[{"half": slice(0, n, 2), "none": slice(0, 0), "one": slice(5, 6), "two": slice(5, 24, 14)}[mask]] = 1
    obs = lqro_mod.obstacle_states(x[[5, 9], :3] + 0.05)
    oxy, oz = [0.1, 0.2], [0.1, 0.2]
    ctx = mk(lqro_mod, n, gains)
    ctx.set_obstacles(obs, oxy, oz)
    ctx.set_active(a)
    w = pr.predict(x, vg, gains, H, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz, active=a)
    rows, tot = same(ctx, ctx.predict(x, vg), w[0], w[1], mask)
    off = a == 0
    assert np.all(rows["s2_min"][off] == INF) and np.all(rows["n_conf"][off] == 0) and np.all(rows["j_s2"][off] == -1)
    for f in ("j_s2", "j_d2", "j_first"):
        assert not np.isin(rows[f], np.nonzero(off)[0]).any()
    assert not np.isin(rows["conf"], np.nonzero(off)[0]).any()
    if mask == "one":   # no agent column: the obstacles alone
        assert rows["j_s2"][5] == n and rows["n_conf"][5] >= 1
    # the same mask over given paths: the obstacle columns are the caller's
    P = np.concatenate([w[2], np.repeat(obs[:, None, :3], H, axis=1)])
    wp = pr.predict_paths(P, n, RXY, RZ, obs_xy=oxy, obs_z=oz, active=a)
    same(ctx, ctx.predict_paths(P), wp[0], wp[1], (mask, "given"))
    ctx.set_active(None)
    w = pr.predict(x, vg, gains, H, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz)
    same(ctx, ctx.predict(x, vg), w[0], w[1], "mask cleared")
    ctx.close()


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["reference", "canonical"])
def test_step_then_predict_on_one_stream(lqro_mod, gains, rule):
    """The dense 24-agent swarm: step_device then predict_device(x, newv) with
    no host wait between them, against numpy over the newV read back; the step
    equals that of a context that never predicted."""
    n, h, npts = 24, 50, 100
    x0, vg = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    flags = lqro_mod.LQRO_FLAG_RECORDS | (lqro_mod.LQRO_FLAG_QHULL_ORDER if rule == "reference" else 0)
    ctxs = [mk(lqro_mod, n, gains, h=h, npts=npts, flags=flags) for _ in range(2)]
    pred, plain = ctxs
    d_vg = torch.from_numpy(vg).cuda()
    sid = torch.cuda.current_stream().cuda_stream
    since = pr.empty_total()
    xs = [x0.copy(), x0.copy(), x0.copy()]
    xs[1][:, :3] += 0.05 * xs[1][:, 3:6]
    for t in range(3):
        d_x = torch.from_numpy(xs[t]).cuda()
        out = []
        for c in ctxs:
            d_nv = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda")
            c.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
            if c is pred:
                c.predict_device(d_x.data_ptr(), d_nv.data_ptr(), 0, sid)
            torch.cuda.synchronize()
            out.append((d_nv.cpu().numpy(), c.records(), c.carry_normal(), c.stats()))
        assert out[0][0].tobytes() == out[1][0].tobytes(), t
        assert out[0][1].tobytes() == out[1][1].tobytes(), t
        assert out[0][2].tobytes() == out[1][2].tobytes() and out[0][3] == out[1][3], t
        want, tot, _ = pr.predict(xs[t], out[0][0], gains, h, RXY, RZ)
        since = pr.fold(since, tot)
        last, acc = pred.prediction()
        assert pc.same_total(last, tot) and pc.same_total(acc, since), (t, last, tot, acc, since)
        assert pc.same_rows(pred.prediction_rows(), want), t
    assert tot["n_conf"] > 0 and since["n_measured"] == 3
    # steps 0 and 2 share their x: the equal minimum keeps the indices of the earliest
    last, acc = pred.prediction(reset=True)
    assert pc.same_total(acc, since)
    last2, acc2 = pred.prediction()
    assert pc.same_total(last2, last) and pc.same_total(acc2, pr.empty_total())
    # rows into the caller's own buffer
    d_rows = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_nv = torch.from_numpy(out[0][0]).cuda()
    pred.predict_device(d_x.data_ptr(), d_nv.data_ptr(), d_rows.data_ptr(), sid)
    torch.cuda.synchronize()
    got = np.frombuffer(d_rows.cpu().numpy().tobytes(), dtype=lqro_mod.PREDICT_ROW_DTYPE)
    assert pc.same_rows(got, want) and pc.same_rows(pred.prediction_rows(), want)
    for c in ctxs:
        c.close()


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize("world,mode", [(2, "block"), (3, "block"), (2, "cyclic"), (3, "cyclic")])
def test_row_shards(lqro_mod, gains, world, mode):
    n, m = 24, 2
    x, vg = lqro_mod.synthetic_swarm(n, box=3.0, seed=12)
    obs = lqro_mod.obstacle_states(x[[5, 9], :3] + 0.05, [[0.1, 0.0, 0.0], [0.0, 0.2, 0.0]])
    oxy, oz = [0.1, 0.2], [0.1, 0.2]
    want, tot, _ = pr.predict(x, vg, gains, H, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz)
    assert tot["n_conf"] > 0
    parts = []
    for rank in range(world):
        ctx = mk(lqro_mod, n, gains, **lqro_mod.shard_rows(n, rank, world, mode))
        ctx.set_obstacles(obs, oxy, oz)
        ids = lqro_mod.shard_row_ids(n, rank, world, mode)
        _, t = same(ctx, ctx.predict(x, vg), want[ids], pr.total(want[ids], ids), (rank, world, mode))
        parts.append(t)
        ctx.close()
    assert pc.same_total(lqro_mod.merge_prediction(parts), tot)


# 8 ------------------------------------------------------------------------
def test_python_hosts(lqro_mod):
    n, h, npts = 24, 30, 50
    x0, vg0 = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    g = lqro_mod.synthesize_gains()
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x0[i], vGoal=vg0[i]) for i in range(n)], horizon=h, n_points=npts)
    sim.findMatrices()
    newv = sim.step()
    rows, tot = sim.predict()
    want, wtot, _ = pr.predict(x0, newv, g, h, RXY, RZ)
    assert pc.same_rows(rows, want) and pc.same_total(tot, wtot)
    sim.ctx.close()
    loop = lqro_mod.DeviceLoop(x0, vg0, g, h, npts, predict=True)
    since = pr.empty_total()
    for t in range(3):
        torch.cuda.synchronize()
        x = loop.x.cpu().numpy()
        loop.step()
        torch.cuda.synchronize()
        want, tt, _ = pr.predict(x, loop.newv.cpu().numpy(), g, h, RXY, RZ)
        since = pr.fold(since, tt)
        last, acc = loop.prediction()
        assert pc.same_total(last, tt) and pc.same_total(acc, since), t
        assert pc.same_rows(loop.ctx.prediction_rows(), want), t
        loop.update()
    assert since["n_measured"] == 3
    loop.close()


def test_cpp_host(lqro_mod, tmp_path):
    from test_predict_cpu import predict_main, write_predict_input
    n, h, npts = 24, 30, 50
    x, vg = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    write_predict_input(tmp_path / "in.bin", x, vg, h, npts)
    r = subprocess.run([predict_main(), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 24 * n + 80 + 64 * n
    newv = np.frombuffer(raw[:24 * n], np.float64).reshape(n, 3)
    want, wtot, _ = pr.predict(x, newv, lqro_mod.synthesize_gains(), h, RXY, RZ)
    tot = lqro_mod._predict_total_dict(lqro_mod.PredictTotal.from_buffer_copy(raw[24 * n:24 * n + 80]))
    rows = np.frombuffer(raw[24 * n + 80:], dtype=lqro_mod.PREDICT_ROW_DTYPE)
    assert pc.same_rows(rows, want) and pc.same_total(tot, wtot)
    assert float(r.stdout.split()[1]) == wtot["s2_min"]


# 9 ------------------------------------------------------------------------
def test_argument_and_state_errors(lqro_mod, gains):
    L = lqro_mod.lib()
    n, h, npts = 12, 30, 50
    x, vg = lqro_mod.synthetic_swarm(n, box=6.0)
    P = pc.random_paths(n, h, 1)
    d_x, d_vg, d_P = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda(), torch.from_numpy(P).cuda()
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    xp, vp, pp = x.ctypes.data, vg.ctypes.data, P.ctypes.data
    out = np.zeros((n, h, 3))

    def calls(c):
        return (L.lqro_predict(c._h, xp, vp, None, None),
                L.lqro_predict_device(c._h, d_x.data_ptr(), d_vg.data_ptr(), None, None),
                L.lqro_predict_paths(c._h, pp, None, None),
                L.lqro_predict_paths_device(c._h, d_P.data_ptr(), None, None))

    for bad in (dict(xy_radius=0.0), dict(z_radius=0.0), dict(xy_radius=-0.26), dict(z_radius=INF),
                dict(xy_radius=float("nan"))):
        ctx = mk(lqro_mod, n, gains, h=h, npts=npts, **bad)
        assert calls(ctx) == (E_ARG,) * 4, bad
        ctx.close()
    ctx = mk(lqro_mod, n, h=h, npts=npts)
    # before lqro_set_gains: the predicting calls alone are refused
    assert calls(ctx) == (E_STATE, E_STATE, 0, 0)
    assert L.lqro_get_paths(ctx._h, out.ctypes.data) == E_STATE      # the last measurement used given paths
    ctx.close()
    ctx = mk(lqro_mod, n, gains, h=h, npts=npts)
    assert L.lqro_get_paths(ctx._h, out.ctypes.data) == E_STATE      # none yet
    assert L.lqro_predict(ctx._h, None, vp, None, None) == E_ARG and L.lqro_predict(ctx._h, xp, None, None, None) == E_ARG
    assert L.lqro_predict_device(ctx._h, None, d_vg.data_ptr(), None, None) == E_ARG
    assert L.lqro_predict_device(ctx._h, d_x.data_ptr(), None, None, None) == E_ARG
    assert L.lqro_predict_paths(ctx._h, None, None, None) == E_ARG
    assert L.lqro_predict_paths_device(ctx._h, None, None, None) == E_ARG
    assert L.lqro_get_paths(ctx._h, None) == E_ARG
    nn = ctypes.c_int64(-1)
    assert L.lqro_get_prediction_rows(ctx._h, None, 0, None) == E_ARG
    # before any prediction: cleared totals, no rows
    last, acc = ctx.prediction()
    assert pc.same_total(last, pr.empty_total()) and pc.same_total(acc, pr.empty_total())
    assert len(ctx.prediction_rows()) == 0
    # NULL rows and NULL total are fine
    want, wtot, wP = pr.predict(x, vg, gains, h, RXY, RZ)
    assert L.lqro_predict(ctx._h, xp, vp, None, None) == 0
    t = lqro_mod.PredictTotal()
    assert L.lqro_predict(ctx._h, xp, vp, None, ctypes.byref(t)) == 0
    assert pc.same_total(lqro_mod._predict_total_dict(t), wtot)
    rows = np.zeros(n, lqro_mod.PREDICT_ROW_DTYPE)
    assert L.lqro_predict(ctx._h, xp, vp, rows.ctypes.data, None) == 0 and pc.same_rows(rows, want)
    assert L.lqro_get_prediction(ctx._h, None, None, 0) == 0
    assert L.lqro_get_prediction_rows(ctx._h, rows.ctypes.data, n - 1, ctypes.byref(nn)) == E_ARG
    assert ctx.prediction()[1]["n_measured"] == 3 and ctx.paths().tobytes() == wP.tobytes()
    # new gains: the next predicting call rebuilds C G_k
    g2 = lqro_mod.synthesize_gains(lqro_mod.perturbed_models(1, rel=0.05, seed=3)[0])
    ctx.set_gains(gains["A"], gains["B"], g2["L"], g2["E"])
    w2 = pr.predict(x, vg, dict(gains, L=g2["L"], E=g2["E"]), h, RXY, RZ)
    assert not pc.same_rows(w2[0], want)
    same(ctx, ctx.predict(x, vg), w2[0], w2[1], "new gains")
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    # given paths: lqro_get_paths has nothing to return
    wp = pr.predict_paths(P, n, RXY, RZ)
    same(ctx, ctx.predict_paths(P), wp[0], wp[1], "given")
    assert L.lqro_get_paths(ctx._h, out.ctypes.data) == E_STATE
    ctx.predict_paths_device(d_P.data_ptr())
    assert pc.same_rows(ctx.prediction_rows(), wp[0])
    # LQRO_E_STATE between _begin and _end
    ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), 0)
    assert calls(ctx) == (E_STATE,) * 4
    assert L.lqro_get_prediction(ctx._h, None, None, 0) == E_STATE
    assert L.lqro_get_prediction_rows(ctx._h, rows.ctypes.data, n, ctypes.byref(nn)) == E_STATE
    assert L.lqro_get_paths(ctx._h, out.ctypes.data) == E_STATE
    ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), 0)
    torch.cuda.synchronize()
    same(ctx, ctx.predict(x, vg), want, wtot, "after the step")
    # lqro_set_obstacles keeps the since-reset total and resizes the buffers
    nm = ctx.prediction()[1]["n_measured"]
    obs = lqro_mod.obstacle_states(x[:2, :3] + 0.1)
    ctx.set_obstacles(obs, 0.5, 0.5)
    assert L.lqro_get_paths(ctx._h, out.ctypes.data) == E_STATE      # (the old paths went with the old buffer)
    w = pr.predict(x, vg, gains, h, RXY, RZ, obs=obs, obs_xy=[0.5, 0.5], obs_z=[0.5, 0.5])
    same(ctx, ctx.predict(x, vg), w[0], w[1], "obstacles set")
    assert ctx.prediction()[1]["n_measured"] == nm + 1
    ctx.close()
