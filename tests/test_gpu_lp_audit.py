"""The LP audit on the GPU (lqro_set_lp_audit, lqro_audit_new_v),
every record and total bit for bit against tests/lp_audit_ref.py's numpy
restatement of lqro.h's formulas."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import lp_audit_cases as ac
import lp_audit_ref as ar
from test_gpu_user_planes import box_for, user_planes_for

pytestmark = pytest.mark.gpu

H, NP = 50, 100
N = 24                                  # the dense swarm of tests/test_gpu_user_planes.py
TOL = ac.TOL
E_ARG, E_STATE = -1, -4
NINF = np.float32(-np.inf)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_plain(lqro, lists, goals, newv, nh, tol=TOL, what=""):
    rows, tot = lqro.audit_new_v(lists, goals, newv, tol, n_hard=nh)
    want, wtot = ar.audit(ar.plain_lists(lists, nh), newv, goals, tol)
    assert ar.same_rows(rows, want), (what, np.nonzero(rows != want)[0][:8])
    assert ar.same_total(tot, wtot), (what, tot, wtot)
    return rows, tot


# 1 ------------------------------------------------------------------------
def test_wave_edges(lqro_mod):
    lists, goals, nh, vel = ac.wave_rows()
    assert sorted({len(c) for c in lists}) == list(ac.WAVE_SIZES)
    rows, tot = check_plain(lqro_mod, lists, goals, vel, nh, what="arbitrary velocities")
    m = np.array([len(c) for c in lists])
    assert np.array_equal(rows["m"], m) and np.array_equal(rows["n_hard"], np.minimum(nh, m))
    assert (rows["n_hard"] < nh).any() and tot["n_planes"] == m.sum() and tot["n_rows_viol"] > 0
    assert np.all(rows["kind_viol"][m > 0] == lqro_mod.LQRO_AUDIT_USER) and np.all(rows["id_viol"] == rows["k_viol"])
    assert np.all(rows["k_viol"][m == 0] == -1) and np.all(rows["viol_max"][m == 0] == NINF)
    newv = lqro_mod.calculate_new_v(lists, goals, n_hard=nh)
    rows, _ = check_plain(lqro_mod, lists, goals, newv, nh, what="the LP's own result")
    assert (rows["n_viol_tol"] == 0).any() and (rows["n_viol_tol"] > 0).any()
    check_plain(lqro_mod, lists, goals, newv, None, tol=0.0, what="no hard prefix")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_total_reduction_edges(lqro_mod, n):
    lists, goals, nh, vel = ac.few_planes(n)
    _, tot = check_plain(lqro_mod, lists, goals, vel, nh, what=n)
    assert tot["n_measured"] == 1 and tot["dv2_i"] >= 0


# 2 ------------------------------------------------------------------------
def test_ties(lqro_mod):
    ties = ac.tie_rows()
    lists, nh = [c for c, _ in ties.values()], np.array([h for _, h in ties.values()], np.int32)
    vel = np.tile(ac.V0, (len(ties), 1))
    rows, _ = check_plain(lqro_mod, lists, np.zeros((len(ties), 3)), vel, nh)
    r = dict(zip(ties, rows))
    assert (r["same_lane"]["viol_max"], r["same_lane"]["k_viol"], r["same_lane"]["n_viol"]) == (2.0, 3, 3)
    assert r["neighbours"]["k_viol"] == 5
    assert (r["prefix_between"]["k_viol"], r["prefix_between"]["k_hard"], r["prefix_between"]["n_hard_viol"]) == (4, 4, 2)
    z = r["signed_zero"]
    assert (z["k_viol"], z["k_hard"], z["n_viol"]) == (2, 2, 0) and z["viol_max"].view(np.uint32) == 0x80000000
    lists, goals, nh, vel = ac.equal_rows()
    _, tot = check_plain(lqro_mod, lists, goals, vel, nh)
    assert (tot["viol_max"], tot["viol_i"], tot["viol_k"]) == (2.0, 1, 66) and (tot["hard_i"], tot["hard_k"]) == (3, 66)


# 3 ------------------------------------------------------------------------
def test_known_outcome(lqro_mod):
    c, goal = [ac.opposing()], np.zeros((1, 3))
    for nh in (0, 1):
        newv = lqro_mod.calculate_new_v(c, goal, n_hard=[nh])
        rows, tot = check_plain(lqro_mod, c, goal, newv, [nh], what=nh)
        r = rows[0]
        if nh == 1:     # the hard plane holds; the soft one gave way, and the record names it
            assert r["n_hard_viol"] == 0 and r["n_viol_tol"] == 1
            assert (r["k_viol"], r["kind_viol"], r["id_viol"]) == (1, lqro_mod.LQRO_AUDIT_USER, 1)
            assert (tot["viol_i"], tot["viol_k"]) == (0, 1) and tot["n_rows_hard_viol"] == 0
        else:           # both gave way alike: the lowest k
            assert r["n_viol_tol"] == 2 and r["k_viol"] == 0 and r["n_hard"] == 0 and r["k_hard"] == -1


# 4 ------------------------------------------------------------------------
def _flags(lqro, rule):
    return lqro.LQRO_FLAG_RECORDS | (lqro.LQRO_FLAG_QHULL_ORDER if rule == "qhull" else 0)


def _ctx(lqro, g, n, flags, h=H, npts=NP, **kw):
    c = lqro.Context(lqro.config(n, h, npts, flags=flags, **kw))
    c.set_gains(g["A"], g["B"], g["L"], g["E"])
    return c


def _step(lqro, ctx, x, vg):
    try:
        return ctx.step(x, vg)
    except lqro.QhullMergeSuspect as e:   # (the step completed; the LP saw the planes the records hold)
        return e.newv


@pytest.fixture(scope="module")
def dense(lqro_mod):
    x, vg = lqro_mod.synthetic_swarm(N, box=3.0, seed=11)
    pos = [x[5 * o + 1, 0:3] + 0.6 * x[5 * o + 1, 3:6] / np.linalg.norm(x[5 * o + 1, 3:6]) for o in range(3)]
    return x, vg, user_planes_for(x), lqro_mod.obstacle_states(np.array(pos))


def _configure(lqro, ctx, dense, config):
    """Sets the configuration; returns what assemble() needs of it."""
    x, vg, user, obs = dense
    inf = np.inf
    fence, faces, usr = None, (), None
    lo = hi = None
    if config in ("box", "all"):
        lo, hi = box_for(x)                               # two agents outside, one within m of a face
    elif config == "floor":
        lo, hi = np.array([-inf, -inf, np.sort(x[:, 2])[3]]), np.array([inf, inf, inf])   # agents below it
    if lo is not None:
        ctx.set_fence(lo, hi, 1.0)
        fence, faces = ar.fence_planes(x, lo, hi, 1.0)
    if config in ("user", "all"):
        ctx.set_user_planes(user)
        usr = user
    if config in ("obstacles", "all"):
        ctx.set_obstacles(obs, responsibility=1.0)
    return fence, faces, usr


CONFIGS = ("none", "box", "floor", "user", "obstacles", "all")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("rule", ["qhull", "canonical"])
def test_in_the_step(lqro_mod, gains, dense, rule, config):
    x, vg, user, obs = dense
    aud, plain = (_ctx(lqro_mod, gains, N, _flags(lqro_mod, rule)) for _ in range(2))
    aud.set_lp_audit(1, TOL)
    for c in (aud, plain):
        fence, faces, usr = _configure(lqro_mod, c, dense, config)
    since = ar.empty_total()
    seen = set()
    for level in (0, 1, 2, 3):
        for c in (aud, plain):
            c.set_hard_planes(level)
        for t in range(3 if config == "all" else 1):
            nv, nv0 = _step(lqro_mod, aud, x, vg), _step(lqro_mod, plain, x, vg)
            recs = aud.records()
            # nothing in the step reads the audit
            assert np.array_equal(_bits(nv), _bits(nv0)) and recs.tobytes() == plain.records().tobytes(), (level, t)
            assert aud.stats() == plain.stats() and aud.carry_normal().tobytes() == plain.carry_normal().tobytes()
            lists = ar.assemble(recs, range(N), N, level, fence, faces, usr)
            want, wtot = ar.audit(lists, nv, vg, TOL)
            rows = aud.lp_audit_rows()
            assert ar.same_rows(rows, want), (level, t, np.nonzero(rows != want)[0][:8])
            since = ar.fold(since, wtot)
            last, acc = aud.lp_audit()
            assert ar.same_total(last, wtot) and ar.same_total(acc, since), (level, t, last, wtot, acc, since)
            assert np.array_equal(rows["i"], np.arange(N)) and np.array_equal(rows["m"], [len(c["planes"]) for c in lists])
            assert np.array_equal(rows["n_hard"], [c["n_hard"] for c in lists])
            seen |= set(rows["kind_viol"].tolist()) | set(rows["kind_hard"].tolist())
            # each source's id
            fv, fh = rows["kind_viol"] == ar.FENCE, rows["kind_hard"] == ar.FENCE
            if config == "floor":
                assert np.all(rows["id_viol"][fv] == 4)                   # the face, not the emitted position 0
                if level >= 1:
                    assert fh.all() and np.all(rows["id_hard"] == 4) and np.all(rows["k_hard"] == 0)
            if config == "box":
                assert set(rows["id_viol"][fv]) <= set(range(6))
                if level == 1:   # (the two agents outside the lower x face: that face is their worst hard plane)
                    assert fh.all() and np.all(rows["id_hard"] == rows["k_hard"])
                    assert (rows["id_hard"] == 0).sum() >= 2
            if config == "user" and level >= 2:
                cnt = np.array([len(u) for u in user])
                assert np.all(rows["kind_hard"][cnt > 0] == ar.USER) and np.all(rows["id_hard"] < np.maximum(cnt, 1))
                assert np.all(rows["k_hard"][cnt == 0] == -1)
            if config == "obstacles" and level == 3:
                has = rows["n_hard"] > 0
                assert has.any() and np.all(rows["kind_hard"][has] == ar.COLUMN) and np.all(rows["id_hard"][has] >= N)
                assert np.all(rows["k_hard"][has] < rows["n_hard"][has])
            cv = rows["kind_viol"] == ar.COLUMN
            assert np.all(rows["id_viol"][cv] != rows["i"][cv]) and np.all(rows["id_viol"][cv] < N + 3)
        if level == 1:   # reset: the since-reset total starts again, the last one stays
            last, acc = aud.lp_audit(reset=True)
            assert ar.same_total(acc, since)
            last2, acc2 = aud.lp_audit()
            assert ar.same_total(last2, last) and ar.same_total(acc2, ar.empty_total())
            since = ar.empty_total()
    assert ar.COLUMN in seen and (config not in ("box", "floor", "all") or ar.FENCE in seen)
    assert config not in ("user", "all") or ar.USER in seen
    if config == "all":
        # culling on (k = 6) at level 3: the obstacle slots as lp_row finds them, ids from the neighbour list
        for c in (aud, plain):
            c.set_neighbors(1.5, 6)
        nv, nv0 = _step(lqro_mod, aud, x, vg), _step(lqro_mod, plain, x, vg)
        recs = aud.records()
        assert len(recs) == N * 6 and np.array_equal(_bits(nv), _bits(nv0))
        lists = ar.assemble(recs, range(N), N, 3, fence, faces, usr)
        want, wtot = ar.audit(lists, nv, vg, TOL)
        assert sum(((r["j"] >= N) & ((r["flags"] & 1) != 0)).any() for r in recs.reshape(N, 6)) >= 2
        assert ar.same_rows(aud.lp_audit_rows(), want)
        since = ar.fold(since, wtot)
        last, acc = aud.lp_audit()
        assert ar.same_total(last, wtot) and ar.same_total(acc, since)
        # off again: no launch, the totals and rows stay where they were
        aud.set_lp_audit(0)
        _step(lqro_mod, aud, x + 0.01, vg)
        last2, acc2 = aud.lp_audit()
        assert ar.same_total(last2, wtot) and ar.same_total(acc2, since) and ar.same_rows(aud.lp_audit_rows(), want)
    aud.close()
    plain.close()


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("halves", [False, True], ids=["step_device", "begin_end"])
def test_schedules(lqro_mod, gains, halves):
    """The 257-agent hot swarm of tests/test_gpu_clearance.py's monitor test
    (8 obstacles, a fence, hard level 3): rows an early LP ran and rows
    k_copy_claimed copied are audited from the caller's newV."""
    from test_gpu_obstacles import HOT, HOT_HI, HOT_LO, HOT_RADII, HOT_TAU, hot_obstacles, obstacle_swarm
    n, m = HOT["n"], HOT["m"]
    x_all, vg = obstacle_swarm(lqro_mod, n, m, HOT["seed"], box=HOT["box"])
    obs = hot_obstacles(lqro_mod, x_all, 0)
    xs = [x_all[:n].copy() for _ in range(3)]
    xs[1][:, :3] += 0.02 * xs[1][:, 3:6]
    xs[2] = xs[1].copy()
    ctxs = []
    for on in (1, 0):
        c = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "qhull"), h=HOT["H"], npts=HOT["NP"])
        c.set_obstacles(obs, *HOT_RADII)
        c.set_fence(HOT_LO, HOT_HI, HOT_TAU)
        c.set_hard_planes(3)
        c.set_lp_audit(on, TOL)
        ctxs.append(c)
    aud = ctxs[0]
    vgn = vg[:n].copy()
    d_vg = torch.from_numpy(vgn).cuda()
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    since = ar.empty_total()
    for t in range(3):
        d_x = torch.from_numpy(xs[t]).cuda()
        out = []
        for c in ctxs:
            d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            if halves:
                c.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
                c.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
            else:
                c.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
            torch.cuda.synchronize()
            out.append((d_nv.cpu().numpy(), c.records(), c.carry_normal(), c.stats()))
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes(), t
        assert out[0][2].tobytes() == out[1][2].tobytes() and out[0][3] == out[1][3], t
        fence, faces = ar.fence_planes(xs[t], HOT_LO, HOT_HI, HOT_TAU)
        lists = ar.assemble(out[0][1], range(n), n, 3, fence, faces)
        want, wtot = ar.audit(lists, out[0][0], vgn, TOL)
        rows = aud.lp_audit_rows()
        assert ar.same_rows(rows, want), (t, np.nonzero(rows != want)[0][:8])
        since = ar.fold(since, wtot)
        last, acc = aud.lp_audit()
        assert ar.same_total(last, wtot) and ar.same_total(acc, since), (t, last, wtot)
    assert since["n_measured"] == 3 and want["m"].max() > 64 and (want["n_hard"] > 6).any()
    for c in ctxs:
        c.close()


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("x_dim", [16, 12])
@pytest.mark.parametrize("world,mode", [(2, "block"), (3, "block"), (2, "cyclic"), (3, "cyclic")])
def test_row_shards(lqro_mod, dense, world, mode, x_dim):
    x, vg = lqro_mod.synthetic_swarm(N, box=3.0, seed=11, x_dim=x_dim)
    g = lqro_mod.synthesize_gains(x_dim=x_dim)
    user = dense[2]
    lo, hi = box_for(x)
    fence, faces = ar.fence_planes(x, lo, hi, 1.0)
    parts, rows_all = [], np.zeros(N, ar.ROW_DTYPE)
    for rank in range(world + 1):      # the last: one context over every row
        kw = lqro_mod.shard_rows(N, rank, world, mode) if rank < world else {}
        ctx = _ctx(lqro_mod, g, N, lqro_mod.LQRO_FLAG_RECORDS, x_dim=x_dim, **kw)
        ctx.set_fence(lo, hi, 1.0)
        ctx.set_user_planes(user)
        ctx.set_hard_planes(2)
        ctx.set_lp_audit(1, TOL)
        nv = _step(lqro_mod, ctx, x, vg)
        ids = ctx.row_ids
        lists = ar.assemble(ctx.records(), ids, N, 2, fence, faces, user)
        want, wtot = ar.audit(lists, nv, vg, TOL, ids)
        rows, (last, _) = ctx.lp_audit_rows(), ctx.lp_audit()
        assert ar.same_rows(rows, want) and ar.same_total(last, wtot), (rank, world, mode)
        if rank < world:
            assert np.array_equal(ids, lqro_mod.shard_row_ids(N, rank, world, mode))
            parts.append(last)
            rows_all[ids] = rows
        else:
            assert ar.same_rows(rows, rows_all) and ar.same_total(lqro_mod.merge_lp_audit(parts), last)
        ctx.close()


# 7 ------------------------------------------------------------------------
def test_python_hosts(lqro_mod):
    n, h, npts = 32, 30, 50
    x0, vg0 = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    g = lqro_mod.synthesize_gains()
    loop = lqro_mod.DeviceLoop(x0, vg0, g, h, npts, lp_audit=TOL, flags=lqro_mod.LQRO_FLAG_RECORDS |
                               lqro_mod.LQRO_FLAG_QHULL_ORDER)
    since = ar.empty_total()
    for t in range(5):
        torch.cuda.synchronize()
        vg = loop.vgoal.cpu().numpy()
        loop.step()
        torch.cuda.synchronize()
        nv = loop.newv.cpu().numpy()
        want, wtot = ar.audit(ar.assemble(loop.ctx.records(), range(n), n), nv, vg, TOL)
        assert ar.same_rows(loop.ctx.lp_audit_rows(), want), t
        since = ar.fold(since, wtot)
        loop.update()
    last, acc = loop.lp_audit()
    assert ar.same_total(last, wtot) and ar.same_total(acc, since) and acc["n_measured"] == 5
    loop.close()
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x0[i], vGoal=vg0[i]) for i in range(n)], horizon=h, n_points=npts)
    sim.set_lp_audit(1)
    sim.findMatrices()
    try:
        sim.step()
    except lqro_mod.QhullMergeSuspect:
        pass
    last, acc = sim.lp_audit()
    assert last["n_measured"] == 1 and acc["n_measured"] == 1 and last["n_planes"] > 0 and last["dv2_i"] >= 0
    nv = np.stack([q.newV for q in sim.qlist])
    rows = sim.ctx.lp_audit_rows()
    v = nv.astype(np.float32)
    assert np.array_equal(rows["v2"], (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    sim.ctx.close()


def test_cpp_host(lqro_mod, tmp_path):
    from test_lp_audit_cpu import audit_main, write_audit_input
    n, steps, h, npts = N, 2, 30, 50
    x, vg = lqro_mod.synthetic_swarm(n, box=3.0, seed=11)
    lo, hi = box_for(x)
    write_audit_input(tmp_path / "in.bin", x, vg, h, npts, steps, TOL, hard=1, lo=lo, hi=hi, tau=1.0)
    r = subprocess.run([audit_main(), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    per = 24 * n + 88 * 2 + 64 * n
    assert len(raw) == steps * per
    fence, faces = ar.fence_planes(x, lo, hi, 1.0)
    since = ar.empty_total()
    for t in range(steps):
        o = t * per
        nv = np.frombuffer(raw[o:o + 24 * n], np.float64).reshape(n, 3)
        o += 24 * n
        last, acc = (lqro_mod._lp_total_dict(lqro_mod.LpTotal.from_buffer_copy(raw[o + 88 * k:o + 88 * (k + 1)]))
                     for k in range(2))
        rows = np.frombuffer(raw[o + 176:o + 176 + 64 * n], lqro_mod.LP_ROW_DTYPE)
        # (no records from the C++ host: each row's fence head and the totals are checked, the rest by its counts)
        v = nv.astype(np.float32)
        viol = fence[:, :, 3:] * (fence[:, :, :3] - v[:, None, :])
        viol = (viol[:, :, 0] + viol[:, :, 1]) + viol[:, :, 2]
        assert np.array_equal(rows["n_hard"], np.full(n, len(faces))) and np.array_equal(rows["i"], np.arange(n))
        assert np.array_equal(rows["hard_viol_max"], viol.max(axis=1))
        assert np.array_equal(rows["id_hard"], np.asarray(faces)[viol.argmax(axis=1)])
        assert ar.same_total(last, ar.total(rows))
        since = ar.fold(since, last)
        assert ar.same_total(acc, since)


# 8 ------------------------------------------------------------------------
def test_argument_and_state_errors(lqro_mod, gains):
    L = lqro_mod.lib()
    n = 12
    x, vg = lqro_mod.synthetic_swarm(n, box=6.0)
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    ctx = _ctx(lqro_mod, gains, n, lqro_mod.LQRO_FLAG_RECORDS, h=30, npts=50)
    for on, tol in ((-1, 0.0), (2, 0.0), (7, 0.0), (1, -1e-9), (1, float("inf")), (1, float("nan")), (0, -1.0)):
        assert L.lqro_set_lp_audit(ctx._h, on, tol) == E_ARG, (on, tol)
    nn = ctypes.c_int64(-1)
    assert L.lqro_get_lp_audit_rows(ctx._h, None, 0, None) == E_ARG
    # before any audit: cleared totals, no rows; NULL totals are fine
    last, acc = ctx.lp_audit()
    assert ar.same_total(last, ar.empty_total()) and ar.same_total(acc, ar.empty_total())
    assert len(ctx.lp_audit_rows()) == 0 and L.lqro_get_lp_audit(ctx._h, None, None, 0) == 0
    ctx.set_lp_audit(1, TOL)
    assert len(ctx.lp_audit_rows()) == 0               # on, but no step yet
    nv = _step(lqro_mod, ctx, x, vg)
    want, wtot = ar.audit(ar.assemble(ctx.records(), range(n), n), nv, vg, TOL)
    rows = np.zeros(n, lqro_mod.LP_ROW_DTYPE)
    assert L.lqro_get_lp_audit_rows(ctx._h, rows.ctypes.data, n - 1, ctypes.byref(nn)) == E_ARG
    assert L.lqro_get_lp_audit_rows(ctx._h, rows.ctypes.data, n, ctypes.byref(nn)) == 0 and nn.value == n
    assert ar.same_rows(rows, want) and ar.same_total(ctx.lp_audit()[0], wtot)
    # LQRO_E_STATE between _begin and _end; the half-step's audit comes with its _end
    ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), 0)
    assert L.lqro_set_lp_audit(ctx._h, 0, 0.0) == E_STATE and L.lqro_set_lp_audit(ctx._h, 1, 0.0) == E_STATE
    assert L.lqro_get_lp_audit(ctx._h, None, None, 0) == E_STATE
    assert L.lqro_get_lp_audit_rows(ctx._h, rows.ctypes.data, n, ctypes.byref(nn)) == E_STATE
    ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), 0)
    torch.cuda.synchronize()
    assert ctx.lp_audit()[1]["n_measured"] == 2
    # the setters keep the setting and the since-reset total
    ctx.set_fence([-9.0] * 3, [9.0] * 3, 1.0)
    ctx.set_obstacles(lqro_mod.obstacle_states(np.zeros((2, 3))), 0.5, 0.5)
    ctx.set_user_planes([np.zeros((0, 6), np.float32)] * n)
    ctx.set_neighbors(50.0, 8)
    ctx.set_hard_planes(1)
    assert ctx.lp_audit()[1]["n_measured"] == 2
    ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), 0)
    torch.cuda.synchronize()
    last, acc = ctx.lp_audit()
    rows = ctx.lp_audit_rows()
    assert acc["n_measured"] == 3 and len(rows) == n and np.all(rows["n_hard"] == 6) and np.all(rows["kind_hard"] == 0)
    # the context-free call: NULL rows, NULL total, both
    c, goal = [ac.opposing()], np.zeros((1, 3))
    p = lqro_mod._p
    pl, offs, nvv = np.ascontiguousarray(c[0]), np.array([0, 2], np.int64), np.zeros((1, 3))
    t = lqro_mod.LpTotal()
    r1 = np.zeros(1, lqro_mod.LP_ROW_DTYPE)
    assert L.lqro_audit_new_v(p(pl), p(offs), None, 1, p(goal), p(nvv), 0.0, None, None, 0) == 0
    assert L.lqro_audit_new_v(p(pl), p(offs), None, 1, p(goal), p(nvv), 0.0, p(r1), None, 0) == 0
    assert L.lqro_audit_new_v(p(pl), p(offs), None, 1, p(goal), p(nvv), 0.0, None, ctypes.byref(t), 0) == 0
    want, wtot = ar.audit(ar.plain_lists(c), nvv, goal, 0.0)
    assert ar.same_rows(r1, want) and ar.same_total(lqro_mod._lp_total_dict(t), wtot) and wtot["n_viol_tol"] == 2
    ctx.close()
