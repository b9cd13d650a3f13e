"""Hard planes (lqro_set_hard_planes, lqro_calculate_new_v_hard) on the GPU,
bit for bit.

The expected value of every row is tests/lp_hard_ref.py (the numpy float32
restatement of the LP with the n_hard rule, pinned to the oracle's LP at
n_hard = 0 by tests/test_hard_planes_cpu.py) over the row's plane list.  At
step level that list is rebuilt from the step's own records (their parity
with the oracle is pinned by the rest of the suite), the numpy fence of
tests/test_gpu_user_planes.py and the user planes: fence, user, then the pair
planes in record order, or at LQRO_HARD_OBSTACLES the obstacle columns'
planes (records with j >= n_agents) ahead of the agent columns'.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import lp_cases
import lp_hard_ref as ref
from conftest import ROOT
from test_gpu_user_planes import fence_planes, hot_user_planes, user_planes_for
from test_hard_planes_cpu import (build_hard_main, sharded_hard_main, violation, write_hard_input,
                                  write_sharded_hard_input)

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "lqr-obstacles_amd")
RULES = ("qhull", "canonical")
H, NP = 50, 100
N, M = 24, 4
# tight enough that the soft step crosses a face on most rows of the dense swarm
LO, HI, TAU = (-1.7, -1.7, -1.8), (1.7, 1.7, 1.8), 1.0


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _flags(lqro, rule, records=True):
    return (lqro.LQRO_FLAG_RECORDS if records else 0) | (lqro.LQRO_FLAG_QHULL_ORDER if rule == "qhull" else 0)


def _ctx(lqro, gains, n, flags, h=H, npts=NP, **kw):
    c = lqro.Context(lqro.config(n, h, npts, flags=flags, **kw))
    c.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    return c


def _step(lqro, ctx, x, vg):
    try:
        return ctx.step(x, vg)
    except lqro.QhullMergeSuspect as e:   # (the step completed; the LP saw the planes the records hold)
        return e.newv


# ---------------------------------------------------------------------------
# kernel level: lqro_calculate_new_v_hard
# ---------------------------------------------------------------------------
N_HARD = {"0": lambda m: 0, "1": lambda m: 1, "3": lambda m: 3, "63": lambda m: 63, "64": lambda m: 64,
          "65": lambda m: 65, "half": lambda m: m // 2, "m": lambda m: m, "m+5": lambda m: m + 5}
_WANT = {}   # (row, clamped n_hard) -> the checker's newV, shared by the cases


@pytest.fixture(scope="module")
def fixture_rows():
    cases, goals, _ = lp_cases.fixture_rows()
    runs_lp4 = []
    for k, (c, g) in enumerate(zip(cases, goals)):
        info = {}
        _WANT[(k, 0)] = ref.new_v(c, g, info=info)
        runs_lp4.append(info["fail"] < info["m"])
    return cases, goals, runs_lp4


def _want(k, c, g, nh, runs_lp4):
    nh = min(nh, len(c)) if runs_lp4 else 0   # (linearProgram4 does not run: n_hard is not read)
    if (k, nh) not in _WANT:
        _WANT[(k, nh)] = ref.new_v(c, g, n_hard=nh)
    return _WANT[(k, nh)]


@pytest.mark.parametrize("which", list(N_HARD))
def test_fixture_rows(lqro_mod, fixture_rows, which):
    """Every row of lp_cases.fixture_rows() with a hard prefix that ends
    before, on and after the 64-lane chunk borders, at half the row, at the
    whole row and past it (clamped by the library)."""
    cases, goals, runs_lp4 = fixture_rows
    nh = np.array([N_HARD[which](len(c)) for c in cases], np.int32)
    got = lqro_mod.calculate_new_v(cases, goals, n_hard=nh)
    want = np.stack([_want(k, c, g, int(nh[k]), runs_lp4[k]) for k, (c, g) in enumerate(zip(cases, goals))])
    bad = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
    assert len(bad) == 0, (which, bad[:8], [len(cases[b]) for b in bad[:8]])
    if which in ("half", "m"):
        soft = np.stack([_WANT[(k, 0)] for k in range(len(cases))])
        assert (_bits(want) != _bits(soft)).any(1).sum() >= 20, "the hard prefix changes too few rows"


def test_null_is_the_soft_lp(lqro_mod, fixture_rows):
    cases, goals, _ = fixture_rows
    soft = lqro_mod.calculate_new_v(cases, goals)
    want = np.stack([_WANT[(k, 0)] for k in range(len(cases))])
    assert np.array_equal(_bits(soft), _bits(want))
    assert np.array_equal(_bits(lqro_mod.calculate_new_v(cases, goals, n_hard=np.zeros(len(cases), np.int32))),
                          _bits(soft))
    # NULL through the C ABI itself
    n = len(cases)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(c) for c in cases])
    flat = np.concatenate([np.asarray(c, np.float32).reshape(-1, 6) for c in cases])
    vg, out = np.ascontiguousarray(goals, np.float64), np.zeros((n, 3))
    L = lqro_mod.lib()
    assert L.lqro_calculate_new_v_hard(flat.ctypes.data, offs.ctypes.data, None, n, vg.ctypes.data, 100.0,
                                       out.ctypes.data, 0) == 0
    assert np.array_equal(_bits(out), _bits(soft))
    nh = np.zeros(n, np.int32)
    nh[n // 2] = -1
    assert L.lqro_calculate_new_v_hard(flat.ctypes.data, offs.ctypes.data, nh.ctypes.data, n, vg.ctypes.data, 100.0,
                                       out.ctypes.data, 0) == -1


def test_batch_mixing_hard_and_soft_agents(lqro_mod):
    cases, goals = lp_cases.random_cases(60, seed=2, max_planes=200)
    nh = np.array([(0, len(c) // 2, 1, len(c))[k % 4] for k, c in enumerate(cases)], np.int32)
    got = lqro_mod.calculate_new_v(cases, goals, n_hard=nh)
    want = np.stack([ref.new_v(c, g, n_hard=int(h)) for c, g, h in zip(cases, goals, nh)])
    soft = np.stack([ref.new_v(c, g) for c, g in zip(cases, goals)])
    assert np.array_equal(_bits(got), _bits(want)), np.nonzero((_bits(got) != _bits(want)).any(1))[0]
    changed = (_bits(want) != _bits(soft)).any(1)
    assert changed.sum() >= 5 and not changed[nh == 0].any()


@pytest.mark.parametrize("tail", [100, 0], ids=["m-100", "m"])
@pytest.mark.parametrize("m", lp_cases.LONG_SIZES)
def test_layout_borders(lqro_mod, m, tail):
    """The last row of each launch_lp layout and the first of the next, with a
    hard prefix longer than the projected part of every violated plane's list."""
    c, g = lp_cases.long_row(m, 77)
    soft, want = ref.new_v(c, g), ref.new_v(c, g, n_hard=m - tail)
    assert not np.array_equal(_bits(want), _bits(soft)), "the hard prefix does not show on this row"
    got = lqro_mod.calculate_new_v([c], g[None], n_hard=[m - tail])
    assert np.array_equal(_bits(got[0]), _bits(want)), (m, tail, got, want)


# ---------------------------------------------------------------------------
# step level
# ---------------------------------------------------------------------------
def row_lists(recs, nrows, n_agents):
    """Per row (agent planes, obstacle planes), each (k, 6) float32 in record order."""
    out = []
    for row in recs.reshape(nrows, -1):
        k = (row["flags"] & 1) != 0
        pl = np.concatenate([row["plane_point"], row["plane_normal"]], 1).astype(np.float32)
        ob = row["j"] >= n_agents
        out.append((pl[k & ~ob], pl[k & ob]))
    return out


def expected(recs, row_ids, n_agents, vg, level, fence=None, user=None, soft_too=False):
    """The checker over each row's list at `level`: (newV[, the soft LP's over
    the same list, the rows' fence planes' worst violation by it])."""
    lists = row_lists(recs, len(row_ids), n_agents)
    none = np.zeros((0, 6), np.float32)
    out, soft, cross = np.zeros((len(row_ids), 3)), np.zeros((len(row_ids), 3)), []
    for k, i in enumerate(row_ids):
        f = fence[i] if fence is not None else none
        u = np.asarray(user[i], np.float32).reshape(-1, 6) if user is not None else none
        agents, obs = lists[k]
        if level >= 3:
            c, nh = np.concatenate([f, u, obs, agents]), len(f) + len(u) + len(obs)
        else:
            c, nh = np.concatenate([f, u, agents, obs]), (0, len(f), len(f) + len(u))[level]
        out[k] = ref.new_v(c, vg[i], n_hard=nh)
        if soft_too:
            soft[k] = ref.new_v(c, vg[i])
            cross.append(violation(f, soft[k]) if len(f) else 0.0)
    return (out, soft, np.array(cross)) if soft_too else out


def obstacles_on_paths(lqro, x, m=M):
    """m obstacles at rest, obstacle o 0.6 m ahead of agent 5 o + 1 along its velocity."""
    pos = []
    for o in range(m):
        a = x[5 * o + 1]
        pos.append(a[0:3] + 0.6 * a[3:6] / np.linalg.norm(a[3:6]))
    return lqro.obstacle_states(np.array(pos))


@pytest.fixture(scope="module")
def dense(lqro_mod):
    x, vg = lqro_mod.synthetic_swarm(N, box=3.0, seed=11)
    return x, vg, user_planes_for(x), obstacles_on_paths(lqro_mod, x), fence_planes(x, np.array(LO), np.array(HI), TAU)


def _dense_ctx(lqro, gains, dense, rule, level, records=True, **kw):
    x, vg, user, obs, _ = dense
    ctx = _ctx(lqro, gains, N, _flags(lqro, rule, records), **kw)
    ctx.set_fence(LO, HI, TAU)
    ctx.set_user_planes(user)
    ctx.set_obstacles(obs, responsibility=1.0)
    ctx.set_hard_planes(level)
    return ctx


_SOFT = {}   # rule -> (records, newV, statistics) of the level-0 context
COUNTS = ("pairs", "planes", "inside", "hull_ok", "hull_fail", "gjk_backups", "sum_n_reach")


def _counts(ctx):
    st = ctx.stats()
    return {k: st[k] for k in COUNTS}


def _soft_step(lqro, gains, dense, rule):
    if rule not in _SOFT:
        ctx = _dense_ctx(lqro, gains, dense, rule, 0)
        nv = _step(lqro, ctx, dense[0], dense[1])
        _SOFT[rule] = (ctx.records(), nv, _counts(ctx))
        ctx.close()
    return _SOFT[rule]


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("rule", RULES)
def test_levels(lqro_mod, gains, dense, rule, level):
    x, vg, user, obs, fence = dense
    recs0, nv0, stats0 = _soft_step(lqro_mod, gains, dense, rule)
    assert stats0["inside"] > 0
    ctx = _dense_ctx(lqro_mod, gains, dense, rule, level)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    # only the LP's view moves: records, their order and the statistics are the soft context's
    assert len(recs) == N * (N - 1 + M) and recs.tobytes() == recs0.tobytes()
    assert _counts(ctx) == stats0
    want, soft, cross = expected(recs, range(N), N, vg, level, fence, user, soft_too=True)
    if level < 3:   # (the soft LP over the same list is the level-0 step)
        assert np.array_equal(_bits(soft), _bits(nv0))
    assert (cross > 1e-3).sum() >= 1, "the soft step crosses no fence face"
    assert (_bits(want) != _bits(soft)).any(1).sum() >= 1, "the level changes no row"
    assert np.array_equal(_bits(nv), _bits(want)), (rule, level, np.nonzero((_bits(nv) != _bits(want)).any(1))[0])
    if level == 3:
        lists = row_lists(recs, N, N)
        assert sum(len(o) > 0 and len(a) > 0 for a, o in lists) >= 2, "no row has obstacle and agent planes"
        in_order = expected(recs, range(N), N, vg, 2, fence, user)
        assert (_bits(want) != _bits(in_order)).any(), "the obstacle planes' place and hardness show in no row"
    ctx.close()


def test_level_with_an_empty_head_is_a_plain_context(lqro_mod, gains, dense):
    x, vg = dense[0], dense[1]
    plain = _ctx(lqro_mod, gains, N, _flags(lqro_mod, "qhull"))
    ctx = _ctx(lqro_mod, gains, N, _flags(lqro_mod, "qhull"))
    ctx.set_hard_planes(lqro_mod.LQRO_HARD_OBSTACLES)
    for t in range(2):
        a, b = _step(lqro_mod, plain, x, vg), _step(lqro_mod, ctx, x, vg)
        assert np.array_equal(_bits(a), _bits(b)), t
        assert plain.records().tobytes() == ctx.records().tobytes() and _counts(plain) == _counts(ctx)
        assert np.array_equal(_bits(plain.carry_normal()), _bits(ctx.carry_normal()))
    # a fence with every face at infinity, user lists that are all empty: still nothing in the head
    inf = np.inf
    ctx.set_fence([-inf] * 3, [inf] * 3, 2.0)
    ctx.set_user_planes([np.zeros((0, 6), np.float32)] * N)
    assert np.array_equal(_bits(_step(lqro_mod, plain, x, vg)), _bits(_step(lqro_mod, ctx, x, vg)))
    plain.close()
    ctx.close()


def test_arguments_state_and_the_level_staying(lqro_mod, gains, dense):
    x, vg, user, obs, fence = dense
    L = lqro_mod.lib()
    ctx = _dense_ctx(lqro_mod, gains, dense, "qhull", 3)
    for bad in (-1, 4, 1 << 20):
        assert L.lqro_set_hard_planes(ctx._h, bad) == -1
    assert L.lqro_set_hard_planes(None, 1) == -1
    first = _step(lqro_mod, ctx, x, vg)
    assert np.array_equal(_bits(first), _bits(expected(ctx.records(), range(N), N, vg, 3, fence, user)))
    # a refused level changed nothing; the level survives clearing and re-setting what it covers
    ctx.set_obstacles(None)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    assert len(recs) == N * (N - 1)
    assert np.array_equal(_bits(nv), _bits(expected(recs, range(N), N, vg, 3, fence, user)))
    ctx.set_fence(None, None, 0.0)
    ctx.set_user_planes(None)
    ctx.set_fence(LO, HI, TAU)
    ctx.set_user_planes(user)
    ctx.set_obstacles(obs, responsibility=1.0)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    want, soft, _ = expected(recs, range(N), N, vg, 3, fence, user, soft_too=True)
    assert np.array_equal(_bits(nv), _bits(want)) and (_bits(want) != _bits(soft)).any()
    # pending half-step: LQRO_E_STATE, and the level in force stays
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_nv = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    d_tab = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
    assert L.lqro_set_hard_planes(ctx._h, 0) == -4
    ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_nv.cpu().numpy()), _bits(expected(ctx.records(), range(N), N, vg, 3, fence, user)))
    ctx.set_hard_planes(0)
    nv = _step(lqro_mod, ctx, x, vg)
    assert np.array_equal(_bits(nv), _bits(expected(ctx.records(), range(N), N, vg, 0, fence, user)))
    ctx.close()


CULL_DIST, CULL_K = 1.5, 8   # some rows have fewer than 8 bodies in range, some more


def test_culling_with_obstacles_in_range(lqro_mod, gains, dense):
    x, vg, user, obs, fence = dense
    K = CULL_K
    ctx = _dense_ctx(lqro_mod, gains, dense, "qhull", 3)
    ctx.set_neighbors(CULL_DIST, K)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    assert len(recs) == N * K
    r = recs.reshape(N, K)
    # the obstacle slots are the last of a row's kept slots, and some rows keep fewer than K
    kept, ob = r["j"] >= 0, r["j"] >= N
    assert not (~kept[:, :-1] & kept[:, 1:]).any() and not (ob[:, :-1] & kept[:, 1:] & ~ob[:, 1:]).any()
    assert (~kept).any() and kept.all(1).any()
    lists = row_lists(recs, N, N)
    assert sum(len(o) > 0 and len(a) > 0 for a, o in lists) >= 2
    want = expected(recs, range(N), N, vg, 3, fence, user)
    assert (_bits(want) != _bits(expected(recs, range(N), N, vg, 2, fence, user))).any()
    assert np.array_equal(_bits(nv), _bits(want)), np.nonzero((_bits(nv) != _bits(want)).any(1))[0]
    ctx.close()


@pytest.mark.parametrize("mode", ["block", "cyclic"])
def test_row_shards_take_the_level(lqro_mod, gains, dense, mode):
    x, vg, user, obs, fence = dense
    world = 2
    seen = []
    for r in range(world):
        ctx = _dense_ctx(lqro_mod, gains, dense, "canonical", 3, **lqro_mod.shard_rows(N, r, world, mode))
        nv = _step(lqro_mod, ctx, x, vg)
        ids = ctx.row_ids
        assert np.array_equal(ids, lqro_mod.shard_row_ids(N, r, world, mode))
        want, soft, _ = expected(ctx.records(), ids, N, vg, 3, fence, user, soft_too=True)
        assert np.array_equal(_bits(nv[ids]), _bits(want)), (r, mode)
        assert (_bits(want) != _bits(soft)).any()
        seen.extend(ids)
        ctx.close()
    assert sorted(seen) == list(range(N))


def _context_two_steps(lqro_mod, gains, dense, level):
    ctx = _dense_ctx(lqro_mod, gains, dense, "qhull", level, records=False)
    out = [_step(lqro_mod, ctx, dense[0], dense[1]) for _ in range(2)]
    ctx.close()
    return out


def test_python_hosts_pass_the_level_through(lqro_mod, gains, dense):
    x, vg, user, obs, _ = dense
    want = _context_two_steps(lqro_mod, gains, dense, 3)
    soft = _context_two_steps(lqro_mod, gains, dense, 0)
    assert (_bits(want[0]) != _bits(soft[0])).any()
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x[i], vGoal=vg[i]) for i in range(N)], horizon=H, n_points=NP,
                             fence=(LO, HI, TAU))
    sim.findMatrices()
    sim.set_hard_planes(lqro_mod.LQRO_HARD_OBSTACLES)
    sim.ctx.set_user_planes(user)
    sim.set_obstacles(obs, responsibility=1.0)
    for t in range(2):
        try:
            sim.step()
        except lqro_mod.QhullMergeSuspect:
            pass                             # (newV is stored before the raise)
        assert np.array_equal(_bits(np.stack([q.newV for q in sim.qlist])), _bits(want[t])), t
    sim.ctx.close()
    loop = lqro_mod.DeviceLoop(x, vg, dict(gains, l=np.zeros(4)), H, NP, fence=(LO, HI, TAU), user_planes=user,
                               obstacles=(obs, None, None, 1.0))
    loop.set_hard_planes(lqro_mod.LQRO_HARD_OBSTACLES)
    for t in range(2):
        nv = loop.step()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(nv.cpu().numpy()), _bits(want[t])), t
    loop.close()


def test_cpp_host_passes_the_level_through(lqro_mod, gains, dense, tmp_path):
    x, vg, user, obs, _ = dense
    want = _context_two_steps(lqro_mod, gains, dense, 3)
    exe = build_hard_main(tmp_path)
    write_hard_input(tmp_path / "in.bin", x, vg, H, NP, 2, 3, LO, HI, TAU, obs, (0.26, 0.75), 1.0, user)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    # (a merge-suspect step ends the program with status 1 after storing newV; this swarm has none)
    assert r.returncode == 0, r.stderr
    got = np.zeros((2, N, 3))
    for line in r.stdout.splitlines():
        t, i, a, b, c = line.split()
        got[int(t), int(i)] = [float.fromhex(a), float.fromhex(b), float.fromhex(c)]
    for t in range(2):
        assert np.array_equal(_bits(got[t]), _bits(want[t])), t


def test_cpp_sharded_host_passes_the_level_through(lqro_mod, gains, dense, tmp_path):
    """lqro::ShardedSimulator (a world of one rank) replays lqro::Simulator's
    trajectory with a fence, obstacles and level 3, and the first step is the
    context's with that level, not the soft one's."""
    x, vg, user, obs, fence = dense
    steps = 2
    write_sharded_hard_input(tmp_path / "in.bin", x, vg, -x[:, :3], H, NP, steps, 11, 3, LO, HI, TAU, obs, (0.26, 0.75),
                             1.0)
    r = subprocess.run([sharded_hard_main(), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(steps, 2, N * 19)
    for t in range(steps):
        assert np.array_equal(out[t, 0].view(np.uint64), out[t, 1].view(np.uint64)), t
    first = {}
    for level in (0, 3):
        ctx = _ctx(lqro_mod, gains, N, _flags(lqro_mod, "qhull", records=False))
        ctx.set_fence(LO, HI, TAU)
        ctx.set_obstacles(obs, responsibility=1.0)
        ctx.set_hard_planes(level)
        first[level] = _step(lqro_mod, ctx, x, vg)
        ctx.close()
    got = out[0, 1][:N * 3].reshape(N, 3)
    assert np.array_equal(_bits(got), _bits(first[3])) and (_bits(first[3]) != _bits(first[0])).any()


# ---------------------------------------------------------------------------
# the hot schedule: the early LP launch, the closing job's LP left to the tail
# ---------------------------------------------------------------------------
HOT = dict(n=257, m=8, box=14.0, seed=7, H=50, NP=50, steps=4)
HOT_LO, HOT_HI, HOT_TAU = (-6.0, -6.0, -6.5), (6.0, 6.0, 6.5), 2.0
HOT_RADII = (1.0, 1.0)


def hot_user(x):
    """tests/test_gpu_user_planes.py's two planes per agent; agents 0-15 get
    two more that contradict each other (3 m/s along n, and 3 m/s against
    it): hard planes that are infeasible among themselves, where the result
    is kept as RVO2 keeps it."""
    base = hot_user_planes(x)
    rng = np.random.default_rng(23)
    out = []
    for i in range(x.shape[0]):
        u = base[i]
        if i < 16:
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
            v = x[i, 3:6]
            u = np.concatenate([u, np.array([np.concatenate([v + 3.0 * n, n]), np.concatenate([v - 3.0 * n, -n])],
                                            np.float32)])
        out.append(u.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def hot(lqro_mod):
    n, m = HOT["n"], HOT["m"]
    x_all, vg = lqro_mod.synthetic_swarm(n + m, box=HOT["box"], seed=HOT["seed"])
    x = x_all[:n].copy()
    pos = []
    for o in range(m):   # obstacle o 0.6 m ahead of agent 16 o + 3 along its velocity, at rest
        a = x[16 * o + 3]
        pos.append(a[0:3] + 0.6 * a[3:6] / np.linalg.norm(a[3:6]))
    return (x, vg[:n].copy(), hot_user(x), lqro_mod.obstacle_states(np.array(pos)),
            fence_planes(x, np.array(HOT_LO), np.array(HOT_HI), HOT_TAU))


def _hot_check(hot, recs, got, t):
    x, vg, user, _, fence = hot
    n = x.shape[0]
    want, soft, _ = expected(recs, range(n), n, vg, 3, fence, user, soft_too=True)
    assert (_bits(want) != _bits(soft)).any(1).sum() >= 16, "the level changes fewer rows than have contradicting planes"
    assert np.array_equal(_bits(got), _bits(want)), (t, np.nonzero((_bits(got) != _bits(want)).any(1))[0])


@pytest.mark.parametrize("split", [False, True], ids=["step_device", "begin_end"])
def test_early_lp_takes_the_level(lqro_mod, gains, hot, split):
    """257 x 264 slots at LQRO_HARD_OBSTACLES: the hot schedule with the early
    LP launch from the third step; the k_qhull job that closes a row leaves
    its LP to the tail (StepPlan::row_lp = 0).  Steps 0 and 3 are compared
    (the plain schedule and the hot one)."""
    x, vg, user, obs, fence = hot
    n = x.shape[0]
    ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "qhull"), h=HOT["H"], npts=HOT["NP"])
    ctx.set_fence(HOT_LO, HOT_HI, HOT_TAU)
    ctx.set_user_planes(user)
    ctx.set_obstacles(obs, *HOT_RADII)
    ctx.set_hard_planes(3)
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    for t in range(HOT["steps"]):
        d_nv.zero_()
        if split:
            ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
            ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
        else:
            ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
        torch.cuda.synchronize()
        if t in (0, HOT["steps"] - 1):
            _hot_check(hot, ctx.records(), d_nv.cpu().numpy(), t)
    assert ctx.stats()["inside"] > 0
    ctx.close()


HOT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import lqro
a = np.load(sys.argv[2], allow_pickle=True)
x, vg = a["x"], a["vg"]
g = lqro.synthesize_gains()
c = lqro.Context(lqro.config(x.shape[0], int(a["H"]), int(a["NP"]),
                             flags=lqro.LQRO_FLAG_RECORDS | lqro.LQRO_FLAG_QHULL_ORDER))
c.set_gains(g["A"], g["B"], g["L"], g["E"])
c.set_fence(a["lo"], a["hi"], float(a["tau"]))
c.set_user_planes(list(a["user"]))
c.set_obstacles(a["obs"], float(a["oxy"]), float(a["oz"]))
c.set_hard_planes(3)
for t in range(int(a["steps"])):
    try:
        nv = c.step(x, vg)
    except lqro.QhullMergeSuspect as e:
        nv = e.newv
np.savez(sys.argv[3], nv=nv, recs=c.records())
"""


def test_early_lp_off_takes_the_level(lqro_mod, hot, tmp_path):
    """The same steps with LQRO_EARLY_LP=0 (read when the context is created:
    a child process); the last step is compared."""
    x, vg, user, obs, fence = hot
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "hot.npz")
    uarr = np.empty(len(user), object)
    for i, u in enumerate(user):
        uarr[i] = u
    np.savez(inp, x=x, vg=vg, user=uarr, obs=obs, oxy=HOT_RADII[0], oz=HOT_RADII[1], lo=HOT_LO, hi=HOT_HI, tau=HOT_TAU,
             H=HOT["H"], NP=HOT["NP"], steps=HOT["steps"])
    env = dict(os.environ, LQRO_EARLY_LP="0")
    r = subprocess.run([sys.executable, "-c", HOT_CHILD, PKG, inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    _hot_check(hot, d["recs"], d["nv"], HOT["steps"] - 1)
