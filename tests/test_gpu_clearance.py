"""The clearance measurement on the GPU (lqro_clearance[_device],
lqro_set_monitor), bit for bit against tests/clearance_ref.py's
numpy restatement of lqro.h's formulas."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import clearance_cases as cc
import clearance_ref as cr

pytestmark = pytest.mark.gpu

H, NP = 10, 20          # (no step in most tests: the smallest tables)
RXY, RZ = 0.26, 0.75    # lqro_config_default's radii
INF = float("inf")
E_ARG, E_STATE = -1, -4


def mk(lqro, n, **kw):
    return lqro.Context(lqro.config(n, kw.pop("h", H), kw.pop("npts", NP), **kw))


def check(lqro, ctx, x, want_rows, want_total, what=""):
    rows, tot = ctx.clearance(x)
    assert cc.same_rows(rows, want_rows), (what, np.nonzero(rows != want_rows)[0][:8])
    assert cc.same_total(tot, want_total), (what, tot, want_total)
    last, _ = ctx.monitor()
    assert cc.same_total(last, want_total), what
    assert cc.same_rows(ctx.monitor_rows(), want_rows), what
    assert np.array_equal(ctx.monitor_pairs(), cr.pairs(want_rows, ctx.row_ids)), what
    return rows, tot


# 1 ------------------------------------------------------------------------
def test_exact_border(lqro_mod):
    rxy, rz = cc.LATTICE_RADII
    ctx = mk(lqro_mod, 64, xy_radius=rxy, z_radius=rz)
    x = cc.states(cc.lattice(1.0))
    want, tot = cr.measure(x, 64, rxy, rz)
    rows, _ = check(lqro_mod, ctx, x, want, tot, "lattice")
    # every axis neighbour sits at s2 == 1.0 exactly: no hit, the smallest tied column
    assert np.all(rows["s2_min"] == 1.0) and np.all(rows["n_hit"] == 0) and np.all(rows["hit"] == -1)
    assert rows["j_s2"][0] == 1 and rows["j_s2"][21] == 5 and tot["n_hit"] == 0 and tot["s2_min"] == 1.0
    x = cc.states(cc.lattice(0.75))
    want, tot = cr.measure(x, 64, rxy, rz)
    rows, got = check(lqro_mod, ctx, x, want, tot, "lattice x 0.75")
    nb = cc.lattice_axis_neighbours()
    assert np.all(rows["s2_min"] == 0.5625) and np.array_equal(rows["n_hit"], nb) and nb.min() == 3 and nb.max() == 6
    for r in rows:
        h = r["hit"][:r["n_hit"]]
        assert np.all(np.diff(h) > 0) and np.all(r["hit"][r["n_hit"]:] == -1)
    assert got["n_hit"] == int(nb.sum()) and got["n_rows_hit"] == 64
    ctx.close()


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_self_by_index(lqro_mod, n):
    ctx = mk(lqro_mod, n)
    x = cc.states(np.tile([[0.3, -1.25, 2.0]], (n, 1)))
    want, tot = cr.measure(x, n, RXY, RZ)
    rows, got = check(lqro_mod, ctx, x, want, tot)
    assert np.all(rows["s2_min"] == 0.0) and np.all(rows["d2_min"] == 0.0) and np.all(rows["n_hit"] == n - 1)
    for i, r in enumerate(rows):
        assert r["hit"][:n - 1].tolist() == [c for c in range(n) if c != i] and r["j_s2"] == (1 if i == 0 else 0)
    assert got["n_hit"] == n * (n - 1) and (got["s2_i"], got["s2_j"]) == (0, 1)
    ctx.close()


# 3 ------------------------------------------------------------------------
def row_windows(n):
    """Own-row ranges of TR - 1, TR and TR + 1 rows around the lanes 0 and
    CHUNK - 1 of every column pass, and every row."""
    tr, ch = cc.TR, cc.CHUNK
    out = {(0, n)}
    for b, k in ((0, tr - 1), (0, tr), (0, tr + 1), (ch - tr + 1, tr - 1), (ch - 8, tr), (ch - 8, tr + 1),
                 (2 * ch - tr, tr), (2 * ch - tr, tr + 1), (n - tr + 1, tr - 1)):
        if b >= 0 and b + k <= n:
            out.add((b, b + k))
    return sorted(out)


@pytest.mark.parametrize("ncols", [2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_chunk_and_tile_borders(lqro_mod, ncols):
    m = 3 if ncols in (65, 257, 513) else 0
    n = ncols - m
    pos = cc.random_positions(ncols, 1000 + ncols)
    x, obs = cc.states(pos[:n]), cc.states(pos[n:])
    oxy, oz = [0.0, 0.5, 1.0][:m], [1.0, 0.25, 0.0][:m]
    want, _ = cr.measure(x, n, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz)
    assert want["n_hit"].max() >= 1 or ncols == 2
    for rb, re in row_windows(n):
        ctx = mk(lqro_mod, n, row_begin=rb, row_end=re)
        if m:
            ctx.set_obstacles(obs, oxy, oz)
        ids = np.arange(rb, re)
        check(lqro_mod, ctx, x, want[ids], cr.total(want[ids], ids), (ncols, rb, re))
        ctx.close()


def test_more_than_six_hits(lqro_mod):
    pos = np.concatenate([cc.random_positions(300, 3, box=12.0), cc.cluster(9, 5, centre=(20.0, 0.0, 0.0))])
    n = len(pos)
    x = cc.states(pos)
    want, tot = cr.measure(x, n, RXY, RZ)
    assert np.all(want["n_hit"][300:] == 8) and np.all(want["hit"][300:] >= 300)
    ctx = mk(lqro_mod, n)
    check(lqro_mod, ctx, x, want, tot)
    pairs = ctx.monitor_pairs()
    assert len(pairs) < tot["n_hit"]          # six a row at the most: the caller compares
    ctx.close()


# 4 ------------------------------------------------------------------------
def test_obstacles(lqro_mod):
    n, m = 24, 6
    x, _ = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    oxy = [0.0, 1.0, 0.5, RXY, 0.0, 1.0]
    oz = [0.0, 1.0, 0.25, RZ, 0.0, 1.0]
    opos = cc.random_positions(m, 9, box=3.0)
    opos[0], opos[3] = x[3, :3], x[7, :3]            # obstacles on agents' positions
    obs = lqro_mod.obstacle_states(opos)
    ctx = mk(lqro_mod, n)
    want0, tot0 = cr.measure(x, n, RXY, RZ)
    check(lqro_mod, ctx, x, want0, tot0, "no obstacles")
    ctx.set_obstacles(obs, oxy, oz)
    want, tot = cr.measure(x, n, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz)
    rows, _ = check(lqro_mod, ctx, x, want, tot, "host obstacles")
    assert rows["s2_min"][3] == 0.0 and rows["j_s2"][3] == n and rows["s2_min"][7] == 0.0 and rows["j_s2"][7] == n + 3
    assert (rows["hit"] >= n).any()
    # a device tensor rewritten between two calls: the second measurement sees the new states
    d_obs = torch.from_numpy(obs.copy()).cuda()
    ctx.set_obstacles(d_obs, oxy, oz)
    check(lqro_mod, ctx, x, want, tot, "device obstacles")
    obs2 = obs.copy()
    obs2[:, :3] = opos[::-1] + 0.125
    d_obs.copy_(torch.from_numpy(obs2))
    torch.cuda.synchronize()
    want2, tot2 = cr.measure(x, n, RXY, RZ, obs=obs2, obs_xy=oxy, obs_z=oz)
    assert not cc.same_rows(want2, want)
    check(lqro_mod, ctx, x, want2, tot2, "rewritten")
    # fewer obstacles, then none: the columns return to N
    ctx.set_obstacles(obs[:2], oxy[:2], oz[:2])
    w, t = cr.measure(x, n, RXY, RZ, obs=obs[:2], obs_xy=oxy[:2], obs_z=oz[:2])
    check(lqro_mod, ctx, x, w, t, "two obstacles")
    ctx.set_obstacles(None)
    check(lqro_mod, ctx, x, want0, tot0, "cleared")
    ctx.close()


# 5 ------------------------------------------------------------------------
def test_fence(lqro_mod):
    lo, hi = np.array([-2.0, -3.0, 0.0]), np.array([2.0, 3.0, 4.0])
    m = np.array([RXY, RXY, RZ])
    p = np.array([
        [0.0, 0.0, 2.0],                       # inside
        [-2.0 + RXY + 0.1, 0.0, 2.0],          # within m of a face's bound: inside the margin still
        [-2.0 + 0.1, 0.0, 2.0],                # the ellipsoid crosses the face: out
        [0.0, 0.0, 0.0],                       # the centre on the floor: out by z_radius
        [5.0, 0.0, 2.0],                       # outside
        [0.0, 0.0, 9.0],                       # above
        [1.0, 1.0, 1.0],
        [0.5, -0.5, 3.0],
    ])
    p[6] = lo + m                              # exactly on three faces: 0.0, not out, the lowest face
    p[7, 0], p[7, 1] = (hi - m)[0], (lo + m)[1]   # on an upper x and a lower y face: face 1
    n = len(p)
    x = cc.states(p)
    ctx = mk(lqro_mod, n)
    want, tot = cr.measure(x, n, RXY, RZ)
    rows, _ = check(lqro_mod, ctx, x, want, tot, "no fence")
    assert np.all(rows["fence_min"] == INF) and np.all(rows["fence_face"] == -1) and tot["fence_i"] == -1
    flo, fhi = np.array([-INF, -INF, 0.0]), np.array([INF, INF, INF])
    ctx.set_fence(flo, fhi, 2.0)               # a floor alone
    want, tot = cr.measure(x, n, RXY, RZ, lo=flo, hi=fhi)
    rows, got = check(lqro_mod, ctx, x, want, tot, "floor")
    assert np.all(rows["fence_face"] == 4) and rows["fence_min"][6] == 0.0 and rows["fence_min"][3] == -RZ
    assert got["n_fence_out"] == 1 and (got["fence_i"], got["fence_face"]) == (3, 4)
    ctx.set_fence(lo, hi, 2.0)                 # six faces
    want, tot = cr.measure(x, n, RXY, RZ, lo=lo, hi=hi)
    rows, got = check(lqro_mod, ctx, x, want, tot, "box")
    assert rows["fence_min"][6] == 0.0 and rows["fence_face"][6] == 0
    assert rows["fence_min"][7] == 0.0 and rows["fence_face"][7] == 1
    assert rows["fence_min"][1] > 0 and rows["fence_face"][1] == 0
    assert (rows["fence_min"] < 0).tolist() == [False, False, True, True, True, True, False, False]
    assert got["n_fence_out"] == 4 and rows["fence_face"][4] == 1 and rows["fence_face"][5] == 5
    ctx.set_fence(None, None, 0.0)
    want, tot = cr.measure(x, n, RXY, RZ)
    check(lqro_mod, ctx, x, want, tot, "fence off")
    ctx.close()


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("halves", [False, True], ids=["step_device", "begin_end"])
def test_monitor_in_the_step(lqro_mod, gains, halves):
    """The 257-agent hot swarm of tests/test_gpu_obstacles.py with its 8
    obstacles: a context with the monitor against one without."""
    from test_gpu_obstacles import HOT, HOT_HI, HOT_LO, HOT_RADII, HOT_TAU, hot_obstacles, obstacle_swarm
    n, m = HOT["n"], HOT["m"]
    x_all, vg = obstacle_swarm(lqro_mod, n, m, HOT["seed"], box=HOT["box"])
    obs = [hot_obstacles(lqro_mod, x_all, w) for w in (0, 1)]
    xs = [x_all[:n].copy() for _ in range(3)]
    xs[1][:, :3] += 0.02 * xs[1][:, 3:6]      # (steps 1 and 2 share their x: an equal minimum twice)
    xs[2] = xs[1].copy()
    flags = lqro_mod.LQRO_FLAG_RECORDS | lqro_mod.LQRO_FLAG_QHULL_ORDER
    ctxs, d_obs = [], []
    for on in (1, 0):
        c = lqro_mod.Context(lqro_mod.config(n, HOT["H"], HOT["NP"], flags=flags))
        c.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
        d_obs.append(torch.from_numpy(obs[0].copy()).cuda())
        c.set_obstacles(d_obs[-1], *HOT_RADII)
        c.set_fence(HOT_LO, HOT_HI, HOT_TAU)
        c.set_monitor(on)
        ctxs.append(c)
    mon, plain = ctxs
    d_vg = torch.from_numpy(vg[:n].copy()).cuda()
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    since = cr.empty_total()
    for t in range(3):
        o = obs[0] if t < 2 else obs[1]
        d_x = torch.from_numpy(xs[t]).cuda()
        out = []
        for c, d_o in zip(ctxs, d_obs):
            d_o.copy_(torch.from_numpy(o.copy()))
            d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            if halves:
                c.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
                c.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
            else:
                c.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
            torch.cuda.synchronize()
            out.append((d_nv.cpu().numpy(), c.records(), c.carry_normal(), c.stats()))
        # nothing in the step reads the measurement
        assert out[0][0].tobytes() == out[1][0].tobytes(), t
        assert out[0][1].tobytes() == out[1][1].tobytes(), t
        assert out[0][2].tobytes() == out[1][2].tobytes() and out[0][3] == out[1][3], t
        want, tot = cr.measure(xs[t], n, RXY, RZ, obs=o, obs_xy=[HOT_RADII[0]] * m, obs_z=[HOT_RADII[1]] * m,
                               lo=HOT_LO, hi=HOT_HI)
        since = cr.fold(since, tot)
        last, acc = mon.monitor()
        assert cc.same_total(last, tot) and cc.same_total(acc, since), (t, last, tot, acc, since)
        assert cc.same_rows(mon.monitor_rows(), want), t
        check(lqro_mod, plain, xs[t], want, tot, ("explicit", t))     # the explicit call on the same x
    assert since["n_measured"] == 3 and tot["n_hit"] > 0
    assert plain.monitor()[1]["n_measured"] == 3                       # (its three explicit calls)
    last, acc = mon.monitor(reset=True)
    assert cc.same_total(acc, since)
    last2, acc2 = mon.monitor()
    assert cc.same_total(last2, last) and cc.same_total(acc2, cr.empty_total())
    # off again: no launch, the totals stay where they were
    mon.set_monitor(0)
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    mon.step_device(torch.from_numpy(xs[0]).cuda().data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
    torch.cuda.synchronize()
    last3, acc3 = mon.monitor()
    assert cc.same_total(last3, last) and cc.same_total(acc3, cr.empty_total())
    for c in ctxs:
        c.close()


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize("x_dim", [16, 12])
@pytest.mark.parametrize("world,mode", [(2, "block"), (3, "block"), (2, "cyclic"), (3, "cyclic")])
def test_row_shards(lqro_mod, world, mode, x_dim):
    n, m = 65, 3
    pos = np.concatenate([cc.cluster(9, 5), cc.random_positions(n - 9 + m, 77)])
    x, obs = cc.states(pos[:n], x_dim), cc.states(pos[n:], x_dim)
    oxy, oz = [0.0, 0.5, 1.0], [0.0, 0.5, 1.0]
    lo, hi = [-1.0, -1.0, -1.0], [1.5, 1.5, 1.5]
    want, tot = cr.measure(x, n, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz, lo=lo, hi=hi)
    whole = mk(lqro_mod, n, x_dim=x_dim)
    whole.set_obstacles(obs, oxy, oz)
    whole.set_fence(lo, hi, 1.0)
    check(lqro_mod, whole, x, want, tot, "whole")
    whole.close()
    parts = []
    for rank in range(world):
        ctx = mk(lqro_mod, n, x_dim=x_dim, **lqro_mod.shard_rows(n, rank, world, mode))
        ctx.set_obstacles(obs, oxy, oz)
        ctx.set_fence(lo, hi, 1.0)
        ids = lqro_mod.shard_row_ids(n, rank, world, mode)
        assert np.array_equal(ctx.row_ids, ids)
        _, t = check(lqro_mod, ctx, x, want[ids], cr.total(want[ids], ids), (rank, world, mode))
        parts.append(t)
        ctx.close()
    assert cc.same_total(lqro_mod.merge_clearance(parts), tot)


# 8 ------------------------------------------------------------------------
def test_python_hosts(lqro_mod):
    n, h, npts = 32, 30, 50
    x0, vg0 = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x0[i], vGoal=vg0[i]) for i in range(n)], horizon=h, n_points=npts)
    rows, tot = sim.clearance()
    want, wtot = cr.measure(x0, n, RXY, RZ)
    assert cc.same_rows(rows, want) and cc.same_total(tot, wtot) and wtot["n_hit"] > 0
    sim.ctx.close()
    g = lqro_mod.synthesize_gains()
    loop = lqro_mod.DeviceLoop(x0, vg0, g, h, npts, monitor=True)
    since = cr.empty_total()
    for t in range(5):
        torch.cuda.synchronize()
        x = loop.x.cpu().numpy()
        loop.step()
        loop.update()
        _, tt = cr.measure(x, n, RXY, RZ)
        since = cr.fold(since, tt)
        if t == 0:
            assert cc.same_total(tt, wtot)
    last, acc = loop.monitor()
    assert cc.same_total(last, tt) and cc.same_total(acc, since) and acc["n_measured"] == 5
    # the true states, on the loop's stream, without a host wait
    xt = loop.own["x_true"]
    loop.ctx.clearance_device(xt.data_ptr(), 0, loop._sid())
    want, wtot = cr.measure(xt.cpu().numpy(), n, RXY, RZ)
    last, acc = loop.monitor()
    assert cc.same_total(last, wtot) and cc.same_rows(loop.ctx.monitor_rows(), want)
    assert cc.same_total(acc, cr.fold(since, wtot))
    # rows into the caller's own buffer
    d_rows = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    loop.ctx.clearance_device(xt.data_ptr(), d_rows.data_ptr(), loop._sid())
    torch.cuda.synchronize()
    got = np.frombuffer(d_rows.cpu().numpy().tobytes(), dtype=lqro_mod.CLEARANCE_ROW_DTYPE)
    assert cc.same_rows(got, want) and cc.same_rows(loop.ctx.monitor_rows(), want)
    loop.close()


def test_cpp_host(lqro_mod, tmp_path):
    from test_clearance_cpu import clear_main, write_clear_input
    n, m = 24, 2
    x, _ = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    obs = lqro_mod.obstacle_states(cc.random_positions(m, 4, box=3.0))
    oxy, oz = [0.0, 1.0], [0.0, 1.0]
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.5, 1.5, 2.0])
    write_clear_input(tmp_path / "in.bin", x, 30, 50, obs, oxy, oz, lo, hi)
    r = subprocess.run([clear_main(), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, wtot = cr.measure(x, n, RXY, RZ, obs=obs, obs_xy=oxy, obs_z=oz, lo=lo, hi=hi)
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 80 + 64 * n + 160
    tots = [lqro_mod._total_dict(lqro_mod.ClearanceTotal.from_buffer_copy(raw[o:o + 80]))
            for o in (0, 80 + 64 * n, 160 + 64 * n)]
    rows = np.frombuffer(raw[80:80 + 64 * n], dtype=lqro_mod.CLEARANCE_ROW_DTYPE)
    assert cc.same_rows(rows, want) and cc.same_total(tots[0], wtot)
    assert cc.same_total(tots[1], wtot)                                  # the monitor's step read the same x
    assert cc.same_total(tots[2], cr.fold(cr.fold(cr.empty_total(), wtot), wtot))
    assert float(r.stdout.split()[1]) == wtot["s2_min"]


# 9 ------------------------------------------------------------------------
def test_argument_and_state_errors(lqro_mod, gains):
    L = lqro_mod.lib()
    n = 12
    x, vg = lqro_mod.synthetic_swarm(n, box=6.0)
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    xp = x.ctypes.data
    for bad in (dict(xy_radius=0.0), dict(z_radius=0.0), dict(xy_radius=-0.26), dict(z_radius=INF),
                dict(xy_radius=float("nan"))):
        ctx = mk(lqro_mod, n, **bad)
        assert L.lqro_clearance(ctx._h, xp, None, None) == E_ARG, bad
        assert L.lqro_clearance_device(ctx._h, d_x.data_ptr(), None, None) == E_ARG, bad
        assert L.lqro_set_monitor(ctx._h, 1) == E_ARG, bad
        ctx.close()
    ctx = mk(lqro_mod, n, h=30, npts=50)
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    assert L.lqro_clearance(ctx._h, None, None, None) == E_ARG
    assert L.lqro_clearance_device(ctx._h, None, None, None) == E_ARG
    for on in (-1, 2, 7):
        assert L.lqro_set_monitor(ctx._h, on) == E_ARG
    nn = ctypes.c_int64(-1)
    assert L.lqro_get_monitor_rows(ctx._h, None, 0, None) == E_ARG
    assert L.lqro_get_monitor_pairs(ctx._h, None, 0, None) == E_ARG
    # before any measurement: cleared totals, no rows
    last, acc = ctx.monitor()
    assert cc.same_total(last, cr.empty_total()) and cc.same_total(acc, cr.empty_total())
    assert len(ctx.monitor_rows()) == 0 and len(ctx.monitor_pairs()) == 0
    # NULL rows and NULL total are fine
    want, wtot = cr.measure(x, n, RXY, RZ)
    assert L.lqro_clearance(ctx._h, xp, None, None) == 0
    t = lqro_mod.ClearanceTotal()
    assert L.lqro_clearance(ctx._h, xp, None, ctypes.byref(t)) == 0 and cc.same_total(lqro_mod._total_dict(t), wtot)
    rows = np.zeros(n, lqro_mod.CLEARANCE_ROW_DTYPE)
    assert L.lqro_clearance(ctx._h, xp, rows.ctypes.data, None) == 0 and cc.same_rows(rows, want)
    assert L.lqro_get_monitor(ctx._h, None, None, 0) == 0
    assert L.lqro_get_monitor_rows(ctx._h, rows.ctypes.data, n - 1, ctypes.byref(nn)) == E_ARG
    assert ctx.monitor()[1]["n_measured"] == 3
    # LQRO_E_STATE between _begin and _end
    ctx.set_monitor(1)
    ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), 0)
    assert L.lqro_set_monitor(ctx._h, 0) == E_STATE and L.lqro_set_monitor(ctx._h, 1) == E_STATE
    assert L.lqro_clearance(ctx._h, xp, None, None) == E_STATE
    assert L.lqro_clearance_device(ctx._h, d_x.data_ptr(), None, None) == E_STATE
    assert L.lqro_get_monitor(ctx._h, None, None, 0) == E_STATE
    ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), 0)
    torch.cuda.synchronize()
    last, acc = ctx.monitor()
    assert cc.same_total(last, wtot) and acc["n_measured"] == 4
    # the setters keep the monitor setting and the since-reset total
    ctx.set_fence([-9.0] * 3, [9.0] * 3, 1.0)
    ctx.set_obstacles(lqro_mod.obstacle_states(np.zeros((2, 3))), 0.5, 0.5)
    assert ctx.monitor()[1]["n_measured"] == 4
    ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), 0)
    torch.cuda.synchronize()
    last, acc = ctx.monitor()
    assert acc["n_measured"] == 5 and last["fence_face"] >= 0 and len(ctx.monitor_rows()) == n
    ctx.close()
