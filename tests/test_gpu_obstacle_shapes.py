"""Obstacles with a shape and a responsibility each (lqro_set_obstacles_ex,
lqro_set_obstacles_ex_device), bit for bit against the oracle as it stands.

The method of tests/test_gpu_obstacles.py, generalised: one
`pyoracle.step(..., rows=(0, N))` over the (N + M) bodies per distinct shape,
the first with the agents' sphere S, each other with
`oracle.sphere(NP, (RXY + oxy) / 2, (RZ + oz) / 2)`.  Obstacle column o's
pair-local fields come from the step of its own shape, the agent columns' from
the first; then that file's (i, j)-order walk with

    d = rec.dist * (responsibility[o] if j = N + o else 0.5)

redoes the normal, the plane and each row's newV (pyoracle.newv over the
walked planes).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

from conftest import ROOT
from test_gpu_obstacles import (H, HOT, N, NP, PAIR_LOCAL, RULES, RXY, RZ, Oracle, _bits, _ctx, _flags, _step,
                                assert_records, equal_for, hot_obstacles, obstacle_swarm)

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "lqr-obstacles_amd")
E_ARG, E_STATE = -1, -4
AGENTS = (RXY, RZ)
# three classes of their own, one obstacle with the agents' shape, two repeats
MIX_RADII = [(0.0, 0.0), (0.5, 0.25), (1.0, 1.0), (0.5, 0.25), AGENTS, (1.0, 1.0)]
MIX_RESP = [1.0, 0.5, 0.75, 1.0, 0.5, 0.25]
MIX_M = 6
MIX_INSIDE = [1, 2, 8, 4, 2, 9]      # inside-hull pairs per obstacle column (seed 11, both rules)


def arrays(radii, resp):
    return [r[0] for r in radii], [r[1] for r in radii], list(resp)


def set_ex(ctx, obs, radii, resp):
    oxy, oz, rs = arrays(radii, resp)
    ctx.set_obstacles(obs, oxy, oz, rs)


def raw_ex(lqro, ctx, obs, radii, resp, device=False):
    """The C call's status (obs: a host array, or a device pointer with device=True)."""
    oxy, oz, rs = (np.ascontiguousarray(a, np.float64) for a in arrays(radii, resp))
    f = lqro.lib().lqro_set_obstacles_ex_device if device else lqro.lib().lqro_set_obstacles_ex
    p = obs if device else obs.ctypes.data
    return f(ctx._h, p, len(radii), oxy.ctypes.data, oz.ctypes.data, rs.ctypes.data)


_SHAPE_STEPS = {}


def mixed_local(orc, key, x_all, vg, n, rule, radii, rows=None):
    """Records (rows, n + m - 1): the agent columns from the step with S,
    obstacle column o from the step with its own sphere; the walked fields are
    not yet valid.  key: names the swarm (one oracle step per (key, rule,
    shape), shared by the tests)."""
    rows = n if rows is None else rows

    def shape_step(shape):
        k = (key, rule, shape, rows)
        if k not in _SHAPE_STEPS:
            S = None if shape == AGENTS else orc.obstacle_sphere(*shape)
            _SHAPE_STEPS[k] = orc.steps(x_all, vg, rows, rule, S=S)[0][1]
        return _SHAPE_STEPS[k]

    exp = shape_step(AGENTS).copy()
    for o, shape in enumerate(radii):
        if tuple(shape) != AGENTS:
            exp[:, n - 1 + o] = shape_step(tuple(shape))[:, n - 1 + o]
    return exp


def walk_ex(lqro, oracle, local, x_all, vg, n, resp, carry, rows=None):
    """The walk of tests/test_gpu_obstacles.py with one responsibility per
    obstacle: (records with the walked fields, newV per row, carry out)."""
    exp = local.copy()
    carry = np.array(carry, np.float64)
    rows = range(exp.shape[0]) if rows is None else rows
    nv = np.zeros((len(rows), 3))
    for r, i in enumerate(rows):
        planes = []
        for q in range(exp.shape[1]):
            rec = exp[r, q]
            fl = int(rec["flags"])
            if not (fl & lqro.REC_PLANE) or (fl & lqro.REC_HULLFAIL):
                continue
            nrm = carry.copy() if fl & lqro.REC_STALE else rec["normal"].copy()
            carry = nrm
            j = int(rec["j"])
            d = rec["dist"] * (np.float64(resp[j - n]) if j >= n else 0.5)
            mult = 1.0 if fl & lqro.REC_INSIDE else -1.0
            pt = np.array([x_all[i, 3 + k] + mult * d * nrm[k] for k in range(3)]).astype(np.float32)
            exp[r, q]["normal"] = nrm
            exp[r, q]["plane_point"] = pt
            exp[r, q]["plane_normal"] = nrm.astype(np.float32)
            planes.append(np.concatenate([pt, nrm.astype(np.float32)])[None])
        nv[r] = oracle.newv(np.concatenate(planes) if planes else np.zeros((0, 6), np.float32), vg[i], 100.0)
    return exp, nv, carry


def column_counts(lqro, recs, n, m):
    """Per obstacle column (planes, inside-hull pairs, stale pairs)."""
    fl = recs["flags"][:, n - 1:n - 1 + m]
    return ([int(v) for v in ((fl & lqro.REC_PLANE) != 0).sum(0)], [int(v) for v in ((fl & lqro.REC_INSIDE) != 0).sum(0)],
            [int(v) for v in ((fl & lqro.REC_STALE) != 0).sum(0)])


@pytest.fixture(scope="module")
def orc(oracle, gains):
    return Oracle(oracle, gains)


def mix_swarm(lqro, seed):
    return obstacle_swarm(lqro, N, MIX_M, seed)


def two_steps(lqro, ctx, x, vg, zero_carry=True):
    """[(newV, records bytes, carry out)] of two steps."""
    if zero_carry:
        ctx.carry_normal(np.zeros(3))
    out = []
    for _ in range(2):
        nv = _step(lqro, ctx, x, vg)
        out.append((nv, ctx.records().tobytes(), ctx.carry_normal()))
    return out


def same_steps(a, b):
    return all(np.array_equal(_bits(p[0]), _bits(q[0])) and p[1] == q[1] and np.array_equal(_bits(p[2]), _bits(q[2]))
               for p, q in zip(a, b))


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule,seed", [("qhull", 11), ("canonical", 11), ("qhull", 12)])
def test_mixed_shapes_and_responsibilities(lqro_mod, oracle, orc, gains, rule, seed):
    x_all, vg = mix_swarm(lqro_mod, seed)
    local = mixed_local(orc, ("mix", seed), x_all, vg, N, rule, MIX_RADII)
    planes, inside, stale = column_counts(lqro_mod, local, N, MIX_M)
    assert not (local["flags"] & lqro_mod.REC_HULLFAIL).any()
    if seed == 11:
        assert planes == [N] * MIX_M and inside == MIX_INSIDE, (planes, inside)
        # every class (0: the agents' shape, 1..3 in order of first appearance) has a plane and an inside-hull pair
        cls = [[(0.0, 0.0), (0.5, 0.25), (1.0, 1.0)].index(r) + 1 if r != AGENTS else 0 for r in MIX_RADII]
        for c in range(4):
            cols = [o for o in range(MIX_M) if cls[o] == c]
            assert sum(planes[o] for o in cols) >= 1 and sum(inside[o] for o in cols) >= 1, c
    else:   # (run for the carried normal: a stale obstacle pair)
        assert stale[MIX_M - 1] >= 1, "no stale obstacle pair in the last column"
    ctx = _ctx(lqro_mod, gains, N, rule)
    set_ex(ctx, x_all[N:], MIX_RADII, MIX_RESP)
    ctx.carry_normal(np.zeros(3))
    carry = np.zeros(3)
    for t in range(2):
        want, nv_w, carry = walk_ex(lqro_mod, oracle, local, x_all, vg, N, MIX_RESP, carry)
        nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
        recs = ctx.records()
        assert len(recs) == N * (N - 1 + MIX_M)
        assert not (recs["flags"] & lqro_mod.REC_HULLFAIL).any()
        assert_records(lqro_mod, recs, want, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_w)), (t, np.nonzero((_bits(nv) != _bits(nv_w)).any(1))[0])
        if rule == "qhull":
            assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
        if t == 0:
            first = nv
    assert ctx.stats()["hull_fail"] == 0
    ctx.close()
    # a kernel that ignores the class gives one of these
    for uniform in ((0.5, 0.25), (1.0, 1.0)):
        u = _ctx(lqro_mod, gains, N, rule)
        set_ex(u, x_all[N:], [uniform] * MIX_M, MIX_RESP)
        u.carry_normal(np.zeros(3))
        nv_u = _step(lqro_mod, u, x_all[:N], vg[:N])
        u.close()
        assert (_bits(nv_u) != _bits(first)).any(1).sum() >= 1, uniform


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((0.5, 0.25), 1.0), (AGENTS, 0.5)], ids=["own_shape", "agents_shape"])
@pytest.mark.parametrize("rule", RULES)
def test_equal_arrays_are_the_one_shape_call(lqro_mod, orc, gains, rule, case):
    radii, resp = case
    x_all, vg, ref = equal_for(orc, lqro_mod, 11, rule)     # (N + 4 bodies)
    m = x_all.shape[0] - N
    old = _ctx(lqro_mod, gains, N, rule)
    old.set_obstacles(x_all[N:], radii[0], radii[1], resp)
    a = two_steps(lqro_mod, old, x_all[:N], vg[:N])
    old.close()
    new = _ctx(lqro_mod, gains, N, rule)
    assert raw_ex(lqro_mod, new, np.ascontiguousarray(x_all[N:]), [radii] * m, [resp] * m) == 0
    new.n_obstacles = m
    b = two_steps(lqro_mod, new, x_all[:N], vg[:N])
    # NULL arrays: the agents' radii and 1.0
    if radii == AGENTS:
        obs = np.ascontiguousarray(x_all[N:])
        assert lqro_mod.lib().lqro_set_obstacles_ex(new._h, obs.ctypes.data, m, None, None, None) == 0
        c = two_steps(lqro_mod, new, x_all[:N], vg[:N])
        old = _ctx(lqro_mod, gains, N, rule)
        old.set_obstacles(x_all[N:])
        assert same_steps(c, two_steps(lqro_mod, old, x_all[:N], vg[:N]))
        old.close()
    new.close()
    assert same_steps(a, b)
    if radii == AGENTS:   # ... and the all-agents oracle step
        for t, (nv_o, recs_o, carry_o) in enumerate(ref):
            assert np.array_equal(_bits(b[t][0]), _bits(nv_o)), t
            assert_records(lqro_mod, np.frombuffer(b[t][1], lqro_mod.RECORD_DTYPE), recs_o, what=(t,))
            if rule == "qhull":
                assert np.array_equal(_bits(b[t][2]), _bits(carry_o)), t


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_permuting_obstacles_permutes_their_columns(lqro_mod, gains, rule):
    x_all, vg = mix_swarm(lqro_mod, 11)
    perm = [4, 2, 0, 5, 1, 3]
    got = []
    for order in (list(range(MIX_M)), perm):
        ctx = _ctx(lqro_mod, gains, N, rule)
        set_ex(ctx, x_all[N:][order], [MIX_RADII[o] for o in order], [MIX_RESP[o] for o in order])
        ctx.carry_normal(np.zeros(3))
        _step(lqro_mod, ctx, x_all[:N], vg[:N])
        got.append(ctx.records().reshape(N, N - 1 + MIX_M).copy())
        ctx.close()
    a, b = got
    for f in PAIR_LOCAL:
        assert np.array_equal(a[f][:, :N - 1], b[f][:, :N - 1]), f       # the agent columns: nothing moves
        if f == "j":
            assert np.array_equal(b[f][:, N - 1:], np.tile(np.arange(N, N + MIX_M), (N, 1)))
            continue
        x, y = a[f][:, N - 1:][:, perm], b[f][:, N - 1:]
        if x.dtype.kind == "f":
            x, y = _bits(x), _bits(y)
        assert np.array_equal(x, y), f


# 4 ------------------------------------------------------------------------
EIGHT = [(0.05 * k, 0.1 * k) for k in range(1, 9)]


def test_class_limit(lqro_mod, oracle, orc, gains):
    """LQRO_OBS_SHAPES_MAX = 8 shapes of their own work (the obstacle columns
    of the first 8 rows against the oracle); a 9th is LQRO_E_ARG and leaves the
    context as it was."""
    m, rows = 8, 8
    assert lqro_mod.LQRO_OBS_SHAPES_MAX == m
    x_all, vg = obstacle_swarm(lqro_mod, N, m + 1, 11)
    x8 = np.ascontiguousarray(x_all[:N + m])
    resp = [1.0, 0.5, 0.75, 0.25, 1.0, 0.5, 0.75, 0.25]
    local = mixed_local(orc, ("eight", 11), x8, vg[:N + m], N, "qhull", EIGHT, rows=rows)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    set_ex(ctx, x8[N:], EIGHT, resp)
    before = two_steps(lqro_mod, ctx, x_all[:N], vg[:N])
    recs = np.frombuffer(before[0][1], lqro_mod.RECORD_DTYPE).reshape(N, N - 1 + m)
    assert_records(lqro_mod, recs[:rows], local, fields=PAIR_LOCAL)
    planes, inside, _ = column_counts(lqro_mod, local, N, m)
    assert min(planes) >= 1 and sum(inside) >= 1, (planes, inside)
    nine = EIGHT + [(0.45, 0.95)]
    obs9 = np.ascontiguousarray(x_all[N:])
    assert raw_ex(lqro_mod, ctx, obs9, nine, resp + [1.0]) == E_ARG
    d9 = torch.from_numpy(obs9).cuda()
    assert raw_ex(lqro_mod, ctx, d9.data_ptr(), nine, resp + [1.0], device=True) == E_ARG
    assert same_steps(before, two_steps(lqro_mod, ctx, x_all[:N], vg[:N]))
    # 9 obstacles in 8 classes of their own and the agents' are fine
    assert raw_ex(lqro_mod, ctx, obs9, EIGHT + [AGENTS], resp + [1.0]) == 0
    ctx.n_obstacles = m + 1
    _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert len(ctx.records()) == N * (N - 1 + m + 1)
    ctx.close()


# 5 ------------------------------------------------------------------------
def test_lds_border(lqro_mod, oracle, gains, tmp_path):
    """H = 256, NP = 100: the class blocks take the waves' LDS.  The largest K
    that leaves one wave (from the layout function) works with fewer waves
    than the plain context's and is bit-exact; K + 1 is LQRO_E_ARG."""
    from test_obstacle_shapes_cpu import build_plan_shapes, max_classes, pair_layouts
    h, npts, n, rows = 256, 100, 12, 4
    exe = build_plan_shapes(tmp_path)
    K = max_classes(exe, h, npts, 16)
    assert 1 <= K < lqro_mod.LQRO_OBS_SHAPES_MAX
    plain_l, k_l = pair_layouts(exe, [(h, npts, 16, 0), (h, npts, 16, K)])
    assert 1 <= k_l["waves"] < plain_l["waves"], (k_l, plain_l)
    shapes = [(0.1 * (k + 1), 0.05 * (k + 1)) for k in range(K + 1)]
    resp = [(1.0, 0.5, 0.75)[k % 3] for k in range(K + 1)]
    x_all, vg = obstacle_swarm(lqro_mod, n, K + 1, 11, box=2.5)
    xk = np.ascontiguousarray(x_all[:n + K])
    orc_h = Oracle(oracle, gains, h=h, npts=npts)
    local = mixed_local(orc_h, ("lds", K), xk, vg[:n + K], n, "qhull", shapes[:K], rows=rows)
    planes, _, _ = column_counts(lqro_mod, local, n, K)
    assert min(planes) >= 1, planes
    want, nv_w, _ = walk_ex(lqro_mod, oracle, local, xk, vg, n, resp[:K], np.zeros(3), rows=range(rows))
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=h, npts=npts)
    set_ex(ctx, xk[n:], shapes[:K], resp[:K])
    before = two_steps(lqro_mod, ctx, x_all[:n], vg[:n])
    recs = np.frombuffer(before[0][1], lqro_mod.RECORD_DTYPE).reshape(n, n - 1 + K)
    # rows [0, rows) enter with the zero carry: the whole walk holds for them
    assert_records(lqro_mod, recs[:rows], want)
    assert np.array_equal(_bits(before[0][0][:rows]), _bits(nv_w))
    obs = np.ascontiguousarray(x_all[n:])
    assert raw_ex(lqro_mod, ctx, obs, shapes, resp) == E_ARG
    assert same_steps(before, two_steps(lqro_mod, ctx, x_all[:n], vg[:n]))
    # K + 1 obstacles in K classes still fit
    assert raw_ex(lqro_mod, ctx, obs, shapes[:K] + [shapes[0]], resp) == 0
    ctx.close()


# 6 ------------------------------------------------------------------------
HOT_SHAPES = [(1.0, 1.0), (0.5, 0.25), AGENTS, (1.0, 1.0), (0.5, 0.25), AGENTS, (1.0, 1.0), (0.5, 0.25)]
HOT_RESP = [1.0, 0.5, 0.75, 0.5, 1.0, 1.0, 0.25, 0.75]


@pytest.fixture(scope="module")
def hot3(lqro_mod, oracle, gains):
    """The 257-agent hot swarm of tests/test_gpu_obstacles.py, its 8
    obstacles in 3 classes: per step (records, newV, carry out) of four steps,
    the obstacles moved between the second and the third."""
    n, m = HOT["n"], HOT["m"]
    x_all, vg = obstacle_swarm(lqro_mod, n, m, HOT["seed"], box=HOT["box"])
    orc = Oracle(oracle, gains, h=HOT["H"], npts=HOT["NP"], threads=8)
    halves = []
    for which in (0, 1):
        xa = x_all.copy()
        xa[n:] = hot_obstacles(lqro_mod, x_all, which)
        halves.append((xa, mixed_local(orc, ("hot", which), xa, vg, n, "qhull", HOT_SHAPES)))
    carry, want = np.zeros(3), []
    for t in range(HOT["steps"]):
        xa, local = halves[t // 2]
        recs, nv, carry = walk_ex(lqro_mod, oracle, local, xa, vg, n, HOT_RESP, carry)
        want.append((recs, nv, carry))
    # the hot launch takes the pairs that were inside-hull a step before, the
    # early LP their rows: obstacle pairs of two or more classes among them
    for _, local in halves:
        _, inside, _ = column_counts(lqro_mod, local, n, m)
        by_shape = {s: sum(inside[o] for o in range(m) if HOT_SHAPES[o] == s) for s in set(HOT_SHAPES)}
        assert sum(v >= 1 for v in by_shape.values()) >= 2, by_shape
    return x_all, vg, halves, want


@pytest.mark.parametrize("hot_split", ["1", "0"])
@pytest.mark.parametrize("halves", [False, True], ids=["step_device", "begin_end"])
def test_device_path_and_schedules(lqro_mod, gains, hot3, monkeypatch, halves, hot_split):
    """257 x 264 slots: the hot schedule from the third step.  The obstacle
    states are a torch tensor rewritten between the second and the third step
    (lqro_set_obstacles_ex_device reads it when the step runs)."""
    monkeypatch.setenv("LQRO_HOT_SPLIT", hot_split)
    x_all, vg, hv, want = hot3
    n = HOT["n"]
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=HOT["H"], npts=HOT["NP"])
    d_obs = torch.from_numpy(hv[0][0][n:].copy()).cuda()
    set_ex(ctx, d_obs, HOT_SHAPES, HOT_RESP)
    d_x, d_vg = torch.from_numpy(x_all[:n].copy()).cuda(), torch.from_numpy(vg[:n].copy()).cuda()
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    for t in range(HOT["steps"]):
        if t == 2:
            d_obs.copy_(torch.from_numpy(hv[1][0][n:].copy()))
        d_nv.zero_()
        if halves:
            ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
            if t == 0:   # the pending half-step still reads the slots: LQRO_E_STATE
                assert raw_ex(lqro_mod, ctx, d_obs.data_ptr(), HOT_SHAPES, HOT_RESP, device=True) == E_STATE
                assert raw_ex(lqro_mod, ctx, hv[0][0][n:].copy(), HOT_SHAPES, HOT_RESP) == E_STATE
                assert lqro_mod.lib().lqro_set_obstacles_ex(ctx._h, None, 0, None, None, None) == E_STATE
            ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
        else:
            ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
        torch.cuda.synchronize()
        recs_w, nv_w, carry = want[t]
        assert_records(lqro_mod, ctx.records(), recs_w, what=(t,))
        got = d_nv.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(nv_w)), (t, np.nonzero((_bits(got) != _bits(nv_w)).any(1))[0])
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
    ctx.close()


# 7 ------------------------------------------------------------------------
def test_per_agent_gains(lqro_mod, oracle):
    """X = 12, N = 12, M = 3 in 2 classes, per-agent gains: each row agent's
    own tables and its own slice bound per class."""
    n, m, X, h = 12, 3, 12, 40
    shapes, resp = [(0.5, 0.25), (1.0, 1.0), (0.5, 0.25)], [1.0, 0.5, 0.75]
    models = lqro_mod.perturbed_models(n)
    g = lqro_mod.synthesize_gains_batch(models, x_dim=X)
    AB = lqro_mod.synthesize_gains(x_dim=X)
    x_all, vg = obstacle_swarm(lqro_mod, n, m, 11, box=2.5, x_dim=X)
    T, NCF = np.zeros((n + m, h, 9)), np.zeros((n + m, h, 3, X))
    for r in range(n):   # (the obstacles have no tables: a row's pair reads the row agent's)
        T[r], NCF[r] = oracle.tables(AB["A"], AB["B"], g["L"][r], g["E"][r], h, X=X)
    orc = Oracle(oracle, None, h=h, npts=NP, tabs=(T, NCF), per_agent=True)
    local = mixed_local(orc, ("x12", 11), x_all, vg, n, "qhull", shapes)
    planes, _, _ = column_counts(lqro_mod, local, n, m)
    assert min(planes) >= 1, planes
    # set before the gains: lqro_set_gains builds the classes' slice bounds
    ctx = lqro_mod.Context(lqro_mod.config(n, h, NP, x_dim=X, flags=_flags(lqro_mod, "qhull")))
    set_ex(ctx, x_all[n:], shapes, resp)
    ctx.set_gains(AB["A"], AB["B"], g["L"], g["E"], per_agent=True)
    carry = np.zeros(3)
    for t in range(2):
        want, nv_w, carry = walk_ex(lqro_mod, oracle, local, x_all, vg, n, resp, carry)
        nv = _step(lqro_mod, ctx, x_all[:n], vg[:n])
        assert_records(lqro_mod, ctx.records(), want, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_w)), t
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
    ctx.close()


def test_per_agent_gains_hot_launch(lqro_mod, oracle, hot3):
    """Per-agent gains on the hot swarm: from the third step the hot launch
    reads the row agent's tables in place (kHotPerAgent), the classes' slice
    bounds [class][agent][H] among them."""
    x_all, vg, hv, _ = hot3
    n, m, h, npts = HOT["n"], HOT["m"], HOT["H"], HOT["NP"]
    xa = hv[0][0]
    g = lqro_mod.synthesize_gains_batch(lqro_mod.perturbed_models(n))
    AB = lqro_mod.synthesize_gains()
    T, NCF = np.zeros((n + m, h, 9)), np.zeros((n + m, h, 3, 16))
    for r in range(n):
        T[r], NCF[r] = oracle.tables(AB["A"], AB["B"], g["L"][r], g["E"][r], h)
    orc = Oracle(oracle, None, h=h, npts=npts, tabs=(T, NCF), per_agent=True, threads=8)
    local = mixed_local(orc, ("hot_pa", 0), xa, vg, n, "qhull", HOT_SHAPES)
    _, inside, _ = column_counts(lqro_mod, local, n, m)
    by_shape = {s: sum(inside[o] for o in range(m) if HOT_SHAPES[o] == s) for s in set(HOT_SHAPES) - {AGENTS}}
    assert all(v >= 1 for v in by_shape.values()), by_shape
    ctx = lqro_mod.Context(lqro_mod.config(n, h, npts, flags=_flags(lqro_mod, "qhull")))
    ctx.set_gains(AB["A"], AB["B"], g["L"], g["E"], per_agent=True)
    set_ex(ctx, xa[n:], HOT_SHAPES, HOT_RESP)
    carry = np.zeros(3)
    for t in range(3):
        want, nv_w, carry = walk_ex(lqro_mod, oracle, local, xa, vg, n, HOT_RESP, carry)
        nv = _step(lqro_mod, ctx, xa[:n], vg[:n])
        assert_records(lqro_mod, ctx.records(), want, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_w)), t
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
    ctx.close()


# 8 ------------------------------------------------------------------------
def test_culling(lqro_mod, oracle, orc, gains):
    """Obstacles of different classes among a row's K neighbours: the
    oracle's culled step per shape (the ranking is by centre distance, so a
    slot holds the same column under every shape), then the walk."""
    dist, k = 2.0, 12
    x_all, vg = mix_swarm(lqro_mod, 11)
    oracle.set_neighbors(dist, k)
    try:
        local = mixed_local(orc, ("mix_culled", 11), x_all, vg, N, "qhull", MIX_RADII)
    finally:
        oracle.set_neighbors(0.0, 0)
    want, nv_w, carry = walk_ex(lqro_mod, oracle, local, x_all, vg, N, MIX_RESP, np.zeros(3))
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_neighbors(dist, k)
    set_ex(ctx, x_all[N:], MIX_RADII, MIX_RESP)
    ctx.carry_normal(np.zeros(3))
    nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
    K = min(k, N + MIX_M - 1)
    recs = ctx.records().reshape(N, K)
    kept_shapes = set()
    for i in range(N):
        ref_row = want[i][want[i]["n_reach"] >= 0]
        c = len(ref_row)
        assert c <= K and np.all(recs[i][c:]["n_reach"] == -1)
        assert_records(lqro_mod, recs[i][:c][None], ref_row[None], what=(i,))
        kept_shapes |= {MIX_RADII[j - N] for j in ref_row["j"] if j >= N}
    assert len(kept_shapes) >= 3, kept_shapes
    assert np.array_equal(_bits(nv), _bits(nv_w))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry))
    ctx.close()


@pytest.fixture(scope="module")
def mix_one(lqro_mod, gains):
    """Two steps of one context with the mixed obstacles (pinned against the
    oracle by test_mixed_shapes_and_responsibilities): (newV, records, carry)."""
    x_all, vg = mix_swarm(lqro_mod, 11)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    set_ex(ctx, x_all[N:], MIX_RADII, MIX_RESP)
    ctx.carry_normal(np.zeros(3))
    out = []
    for _ in range(2):
        nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
        out.append((nv, ctx.records().reshape(N, N - 1 + MIX_M).copy(), ctx.carry_normal()))
    ctx.close()
    return x_all, vg, out


def test_hard_obstacles_with_mixed_responsibilities(lqro_mod, gains, mix_one):
    """LQRO_HARD_OBSTACLES: the records are the soft context's, the LP takes
    the obstacle planes (each at its own responsibility) first and hard."""
    from test_gpu_hard_planes import expected
    x_all, vg, one = mix_one
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    set_ex(ctx, x_all[N:], MIX_RADII, MIX_RESP)
    ctx.set_hard_planes(lqro_mod.LQRO_HARD_OBSTACLES)
    ctx.carry_normal(np.zeros(3))
    nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert ctx.records().tobytes() == one[0][1].tobytes()
    want = expected(one[0][1], range(N), N, vg, 3)
    assert np.array_equal(_bits(nv), _bits(want)), np.nonzero((_bits(nv) != _bits(want)).any(1))[0]
    ctx.close()


@pytest.mark.parametrize("world,mode", [(2, "block"), (3, "block"), (2, "cyclic"), (3, "cyclic")])
def test_row_shards(lqro_mod, gains, mix_one, world, mode):
    x_all, vg, ref = mix_one
    x, vgn = x_all[:N], vg[:N]
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vgn.copy()).cuda()
    ctxs = []
    for g in range(world):
        c = _ctx(lqro_mod, gains, N, "qhull", **lqro_mod.shard_rows(N, g, world, mode))
        set_ex(c, x_all[N:], MIX_RADII, MIX_RESP)
        c.carry_normal(np.zeros(3))
        ctxs.append(c)
    for t in range(2):
        tabs = [torch.zeros((N, 4), dtype=torch.float64, device="cuda") for _ in range(world)]
        newv = [torch.zeros((N, 3), dtype=torch.float64, device="cuda") for _ in range(world)]
        for g, c in enumerate(ctxs):
            c.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), tabs[g].data_ptr(), 0)
        torch.cuda.synchronize()
        whole = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        for g in range(world):   # the all-gather: each rank's own rows
            ids = torch.from_numpy(lqro_mod.shard_row_ids(N, g, world, mode).astype(np.int64)).cuda()
            whole[ids] = tabs[g][ids]
        torch.cuda.synchronize()
        for g, c in enumerate(ctxs):
            c.step_device_end(whole.data_ptr(), newv[g].data_ptr(), 0)
        torch.cuda.synchronize()
        nv_r, recs_r, carry_r = ref[t]
        for g, c in enumerate(ctxs):
            ids = lqro_mod.shard_row_ids(N, g, world, mode)
            got = newv[g].cpu().numpy()[ids]
            assert np.array_equal(_bits(got), _bits(nv_r[ids])), (t, g)
            assert c.records().reshape(len(ids), -1).tobytes() == recs_r[ids].tobytes(), (t, g)
            assert np.array_equal(_bits(c.carry_normal()), _bits(carry_r)), (t, g)
    for c in ctxs:
        c.close()


def test_python_hosts_pass_them_through(lqro_mod, gains, mix_one):
    x_all, vg, ref = mix_one
    oxy, oz, rs = arrays(MIX_RADII, MIX_RESP)
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x_all[i], vGoal=vg[i]) for i in range(N)], horizon=H, n_points=NP,
                             records=True)
    sim.findMatrices()
    sim.set_obstacles(lqro_mod.obstacle_states(x_all[N:, 0:3], x_all[N:, 3:6]), oxy, oz, rs)
    sim.ctx.carry_normal(np.zeros(3))
    for t in range(2):
        try:
            sim.step()
        except lqro_mod.QhullMergeSuspect:
            pass                             # (newV is stored before the raise)
        got = np.stack([q.newV for q in sim.qlist])
        assert np.array_equal(_bits(got), _bits(ref[t][0])), t
    sim.ctx.close()
    g = dict(gains, l=np.zeros(4))
    loop = lqro_mod.DeviceLoop(x_all[:N], vg[:N], g, H, NP, flags=_flags(lqro_mod, "qhull"),
                               obstacles=(torch.from_numpy(x_all[N:].copy()).cuda(), oxy, np.array(oz), tuple(rs)))
    for t in range(2):
        nv = loop.step()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(nv.cpu().numpy()), _bits(ref[t][0])), t
    loop.close()


def test_cpp_hosts_pass_them_through(lqro_mod, gains, mix_one, tmp_path):
    """lqro::Simulator and a one-rank lqro::ShardedSimulator through the
    std::vector overloads of setObstacles (tests/cpp/lqro_shapes_main.cpp)."""
    from test_obstacle_shapes_cpu import shapes_main, write_shapes_input
    x_all, vg, ref = mix_one
    steps = 2
    write_shapes_input(tmp_path / "in.bin", x_all[:N], vg[:N], -x_all[:N, :3], H, NP, steps, 11, x_all[N:], MIX_RADII,
                       MIX_RESP)
    r = subprocess.run([shapes_main(), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(steps, 2, N * 19)
    for t in range(steps):
        assert np.array_equal(out[t, 0].view(np.uint64), out[t, 1].view(np.uint64)), t
    # the first step starts from the swarm as it is: one context's newV
    assert np.array_equal(_bits(out[0, 0, :N * 3].reshape(N, 3)), _bits(ref[0][0]))


def test_clearing(lqro_mod, gains):
    """Cleared through either call, the context equals one that never had obstacles."""
    x_all, vg = mix_swarm(lqro_mod, 11)
    x, vgn = x_all[:N], vg[:N]
    plain = _ctx(lqro_mod, gains, N, "qhull")
    p = []
    for t in range(3):
        nv = _step(lqro_mod, plain, x, vgn)
        p.append((nv, plain.records().tobytes(), plain.carry_normal()))
    plain.close()
    far = x_all[N:].copy()
    far[:, 0] += 1000.0          # (no plane: the carried normal stays the plain context's)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    set_ex(ctx, far, MIX_RADII, MIX_RESP)
    nv = _step(lqro_mod, ctx, x, vgn)
    assert np.array_equal(_bits(nv), _bits(p[0][0]))
    assert lqro_mod.lib().lqro_set_obstacles_ex(ctx._h, None, 0, None, None, None) == 0
    ctx.n_obstacles = 0
    nv = _step(lqro_mod, ctx, x, vgn)
    assert np.array_equal(_bits(nv), _bits(p[1][0])) and ctx.records().tobytes() == p[1][1]
    set_ex(ctx, far, MIX_RADII, MIX_RESP)
    ctx.set_obstacles(None)
    nv = _step(lqro_mod, ctx, x, vgn)
    assert np.array_equal(_bits(nv), _bits(p[2][0])) and ctx.records().tobytes() == p[2][1]
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(p[2][2]))
    ctx.close()


def test_argument_and_state_errors(lqro_mod, gains):
    from test_gpu_dyn import _Hip
    x_all, vg = mix_swarm(lqro_mod, 11)
    obs = np.ascontiguousarray(x_all[N:])
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    L = lqro_mod.lib()
    d_obs = torch.from_numpy(obs).cuda()
    inf, nan = np.inf, np.nan
    # one bad value in any position of any array
    for pos in (0, MIX_M - 1):
        for which, bad in [(0, -0.1), (0, inf), (0, nan), (1, -0.1), (1, inf), (1, nan), (2, 0.0), (2, -0.5),
                           (2, 1.0000001), (2, nan), (2, inf)]:
            radii, resp = [list(r) for r in MIX_RADII], list(MIX_RESP)
            if which == 2:
                resp[pos] = bad
            else:
                radii[pos][which] = bad
            assert raw_ex(lqro_mod, ctx, obs, radii, resp) == E_ARG, (pos, which, bad)
            assert raw_ex(lqro_mod, ctx, d_obs.data_ptr(), radii, resp, device=True) == E_ARG, (pos, which, bad)
    assert L.lqro_set_obstacles_ex(None, obs.ctypes.data, MIX_M, None, None, None) == E_ARG
    assert L.lqro_set_obstacles_ex_device(None, d_obs.data_ptr(), MIX_M, None, None, None) == E_ARG
    with pytest.raises(lqro_mod.LqroError):
        ctx.set_obstacles(obs, [0.5] * (MIX_M - 1))
    assert ctx.n_obstacles == 0 and len(_step(lqro_mod, ctx, x_all[:N], vg[:N])) == N   # (a refused call changes nothing)
    assert len(ctx.records()) == N * (N - 1)
    # n_obstacles <= 0 or a null pointer clears, whatever the rest
    set_ex(ctx, obs, MIX_RADII, MIX_RESP)
    bad = np.full(MIX_M, -1.0)
    assert L.lqro_set_obstacles_ex(ctx._h, obs.ctypes.data, 0, bad.ctypes.data, bad.ctypes.data, bad.ctypes.data) == 0
    ctx.n_obstacles = 0
    _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert len(ctx.records()) == N * (N - 1)
    set_ex(ctx, obs, MIX_RADII, MIX_RESP)
    assert L.lqro_set_obstacles_ex_device(ctx._h, None, MIX_M, None, None, None) == 0
    ctx.n_obstacles = 0
    _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert len(ctx.records()) == N * (N - 1)
    # LQRO_E_STATE between _begin and _end
    hip = _Hip()
    d_x, d_vg = hip.put(x_all[:N]), hip.put(vg[:N])
    tab, nv = hip.put(np.zeros((N, 4))), hip.put(np.zeros((N, 3)))
    try:
        ctx.step_device_begin(d_x, d_vg, tab, 0)
        assert raw_ex(lqro_mod, ctx, obs, MIX_RADII, MIX_RESP) == E_STATE
        assert raw_ex(lqro_mod, ctx, d_obs.data_ptr(), MIX_RADII, MIX_RESP, device=True) == E_STATE
        assert L.lqro_set_obstacles_ex(ctx._h, None, 0, None, None, None) == E_STATE
        ctx.step_device_end(tab, nv, 0)
        hip.sync()
        assert raw_ex(lqro_mod, ctx, obs, MIX_RADII, MIX_RESP) == 0
    finally:
        ctx.close()
        hip.free()
