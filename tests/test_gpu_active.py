"""The activity mask (lqro_set_active, lqro_set_active_device),
bit for bit against the oracle as it stands: the step over N agents with mask
a is `pyoracle.step` over the compacted swarm x[a], vgoal[a], its records
mapped back to the N-agent slots by tests/active_ref.py (a slot whose row or
column is inactive: i, j set, every other field zero), its newV scattered into
+0.0 rows, its carried normal as it is.  tests/test_active_cpu.py pins, on the
CPU, what these expectations contain (planes, inside-hull pairs, facet-0
pairs, another carry than the all-active step's)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import active_ref as ar
import clearance_cases as cc
import clearance_ref as cr
import lp_audit_ref as au
import lp_hard_ref as hr
from conftest import ROOT
from test_active_cpu import HOT, TABLE, hot_dropped
from test_gpu_obstacles import Oracle, _bits, _ctx, _flags, _step, assert_records, obstacle_swarm, walk

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "lqr-obstacles_amd")
ACTIVE_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_active_main")
RULES = ("qhull", "canonical")
N, BOX, H, NP = 24, 3.0, 50, 100
RXY, RZ = 0.26, 0.75


@pytest.fixture(scope="module")
def orc(oracle, gains):
    return Oracle(oracle, gains, h=H, npts=NP)


_WANT = {}


def want_for(lqro, orc, seed, name, rule, steps=2):
    """(x, vg, a, [(newV, records, carry out)] of `steps` chained oracle steps
    over the compacted dense swarm), once."""
    key = (seed, name, rule, steps)
    if key not in _WANT:
        x, vg = lqro.synthetic_swarm(N, box=BOX, seed=seed)
        a = ar.mask(name, N)
        xc, vc = ar.compact(a, x, vg)
        _WANT[key] = (x, vg, a, orc.steps(xc, vc, len(xc), rule, steps=steps))
    return _WANT[key]


def step_nan(lqro, ctx, x, vg):
    """lqro_step into a newV prefilled with NaN."""
    nv = np.full((x.shape[0], 3), np.nan)
    x, vg = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(vg, np.float64)
    rc = lqro.lib().lqro_step(ctx._h, lqro._p(x), lqro._p(vg), lqro._p(nv))
    assert rc in (0, -9), rc   # (LQRO_E_QHMERGE: the step completed; the records say which pair)
    return nv


def check(lqro, ctx, a, nv, ref, n, m=0, rows=None, what="", nv_full=None):
    """One step's records, newV, carry and pairs counter against the compacted
    oracle step `ref` (nv_full: the expected N x 3 newV where it is not the
    oracle's own, as under hard planes)."""
    nv_c, recs_c, carry_c = ref
    want, live = ar.expand_records(a, recs_c, n, m, rows=rows)
    got = ctx.records().reshape(want.shape)
    assert_records(lqro, got, want, what=what)                 # (a skipped slot: i, j and zeros)
    assert not got["flags"][~live].any() and not got["n_reach"][~live].any(), what
    ids = np.arange(n) if rows is None else np.asarray(rows)
    full = ar.expand_newv(a, nv_c, n) if nv_full is None else nv_full
    assert np.array_equal(_bits(nv[ids]), _bits(full[ids])), (what, np.nonzero((_bits(nv) != _bits(full)).any(1))[0])
    if ctx.cfg.flags & lqro.LQRO_FLAG_QHULL_ORDER:            # (the canonical rule carries no normal)
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_c)), what
    assert ctx.stats()["pairs"] == ar.pairs(a, m, rows=rows), what


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_all_ones_and_cleared_equal_no_mask(lqro_mod, gains, rule):
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    runs = {}
    for kind in ("never", "ones", "cleared"):
        ctx = _ctx(lqro_mod, gains, N, rule)
        if kind == "ones":
            ctx.set_active(np.ones(N, bool))
        if kind == "cleared":
            ctx.set_active(ar.mask("mod3", N))
            ctx.set_active(None)
        out = []
        for t in range(2):
            nv = step_nan(lqro_mod, ctx, x, vg)
            out.append((nv.tobytes(), ctx.records().tobytes(), ctx.carry_normal().tobytes(), ctx.stats()))
        runs[kind] = out
        ctx.close()
    assert runs["ones"] == runs["never"] and runs["cleared"] == runs["never"]
    assert runs["never"][0][3]["pairs"] == N * (N - 1)


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("seed,name", sorted(TABLE))
def test_table_rows(lqro_mod, orc, gains, seed, name, rule):
    x, vg, a, ref = want_for(lqro_mod, orc, seed, name, rule)
    *_, ref_all = want_for(lqro_mod, orc, seed, "all", rule)
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_active(a.astype(bool))
    for t in range(2):      # (the second step enters with the first's carry)
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, a, nv, ref[t], N, what=(seed, name, rule, t))
        on = ar.ids(a)
        assert not np.signbit(nv[a == 0]).any() and (nv[a == 0] == 0.0).all()
        assert (_bits(nv[on]) != _bits(ref_all[t][0][on])).any()   # the mask shows in an active row
    ctx.close()


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_few_active_agents(lqro_mod, oracle, orc, gains, rule):
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    ctx = _ctx(lqro_mod, gains, N, rule)
    carry = np.array([0.6, 0.0, -0.8])
    # nobody: newV zero, the carry as it entered, nothing built
    ctx.set_active(np.zeros(N, np.uint8))
    ctx.carry_normal(carry)
    nv = step_nan(lqro_mod, ctx, x, vg)
    assert np.array_equal(_bits(nv), _bits(np.zeros((N, 3))))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)) or rule != "qhull"
    st = ctx.stats()
    assert (st["pairs"], st["planes"], st["inside"], st["sum_n_reach"]) == (0, 0, 0, 0) and len(ctx.hull_builds()) == 0
    recs = ctx.records().reshape(N, N - 1)
    assert not recs["flags"].any() and np.array_equal(recs["i"], np.repeat(np.arange(N), N - 1).reshape(N, N - 1))
    # a lone agent: its LP over an empty plane list
    a = np.zeros(N, np.uint8)
    a[7] = 1
    ctx.set_active(a)
    nv = step_nan(lqro_mod, ctx, x, vg)
    lone = np.zeros((N, 3))
    lone[7] = oracle.newv(np.zeros((0, 6), np.float32), vg[7], 100.0)
    assert np.array_equal(_bits(nv), _bits(lone)) and lone[7].any()
    assert ctx.stats()["pairs"] == 0 and not ctx.records()["flags"].any()
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)) or rule != "qhull"
    # two agents: the oracle's two-agent step (the closest pair of the swarm)
    d2 = ((x[:, None, :3] - x[None, :, :3]) ** 2).sum(2) + 1e9 * np.eye(N)
    i, j = np.unravel_index(np.argmin(d2), d2.shape)
    a = np.zeros(N, np.uint8)
    a[[i, j]] = 1
    xc, vc = ar.compact(a, x, vg)
    ref = orc.steps(xc, vc, 2, rule, carry=carry)[0]
    assert (ref[1]["flags"] & lqro_mod.REC_PLANE).all()
    ctx.set_active(a)
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, a, nv, ref, N, what="two")
    ctx.close()


# 4 ------------------------------------------------------------------------
def test_membership_over_time(lqro_mod, orc, gains):
    """ends, all, half, mod3, all: a column that held a plane or a pending hull
    job in one step is inactive in the next; the carry chained through the
    oracle's carry argument."""
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    carry = np.zeros(3)
    for t, name in enumerate(("ends", "all", "half", "mod3", "all")):
        a = ar.mask(name, N)
        xc, vc = ar.compact(a, x, vg)
        ref = orc.steps(xc, vc, len(xc), "qhull", carry=carry)[0]
        ctx.set_active(None if name == "all" and t == 1 else a)
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, a, nv, ref, N, what=(t, name))
        carry = ref[2]
    ctx.close()


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("off", [4, 5, 6])
def test_wave_width_borders(lqro_mod, oracle, gains, rule, off):
    """N = 70: 65, 64 or 63 active columns a row."""
    n = 70
    x, vg = lqro_mod.synthetic_swarm(n)
    a = (np.arange(n) >= off).astype(np.uint8)
    xc, vc = ar.compact(a, x, vg)
    o = Oracle(oracle, gains, h=H, npts=NP, threads=4)
    ref = o.steps(xc, vc, len(xc), rule)[0]
    ctx = _ctx(lqro_mod, gains, n, rule)
    ctx.set_active(a)
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, a, nv, ref, n, what=(rule, off))
    ctx.close()


# 6 ------------------------------------------------------------------------
HOT_STEPS = 6


@pytest.fixture(scope="module")
def hot(lqro_mod, oracle, gains):
    """The 257-agent hot swarm; per step (mask, oracle step): all active in
    steps 0-1 and 4-5, D inactive in steps 2-3."""
    n = HOT["n"]
    x, vg = lqro_mod.synthetic_swarm(n, box=HOT["box"], seed=HOT["seed"])
    o = Oracle(oracle, gains, h=HOT["H"], npts=HOT["NP"], threads=8)
    ones = np.ones(n, np.uint8)
    first = o.steps(x, vg, n, "qhull", steps=2)
    D = hot_dropped(lqro_mod, first[1][1])
    a = ones.copy()
    a[D] = 0
    xc, vc = ar.compact(a, x, vg)
    mid = o.steps(xc, vc, len(xc), "qhull", steps=2, carry=first[1][2])
    last = o.steps(x, vg, n, "qhull", steps=2, carry=mid[1][2])
    # the carried-over inside-hull pairs of step 1: 94 have an agent of D, 25 stay (and are inside again)
    r1 = first[1][1]
    ins = (r1["flags"] & lqro_mod.REC_INSIDE) != 0
    gone = np.isin(r1["i"][ins], D) | np.isin(r1["j"][ins], D)
    assert (int(ins.sum()), int(gone.sum())) == (119, 94)
    assert int(((mid[0][1]["flags"] & lqro_mod.REC_INSIDE) != 0).sum()) == 25
    return x, vg, D, [(ones, first[0]), (ones, first[1]), (a, mid[0]), (a, mid[1]), (ones, last[0]), (ones, last[1])]


@pytest.mark.parametrize("hot_split", ["1", "0"])
@pytest.mark.parametrize("halves", [False, True], ids=["step_device", "begin_end"])
def test_hot_schedule_device_mask(lqro_mod, gains, hot, monkeypatch, halves, hot_split):
    """257 x 256 slots: the hot schedule from the third step, which is the
    first with D inactive.  The mask is a torch tensor given once and rewritten
    in place between the steps."""
    monkeypatch.setenv("LQRO_HOT_SPLIT", hot_split)
    x, vg, D, steps = hot
    n = HOT["n"]
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=HOT["H"], npts=HOT["NP"])
    d_a = torch.ones(n, dtype=torch.uint8, device="cuda")
    ctx.set_active(d_a)
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    L = lqro_mod.lib()
    for t, (a, ref) in enumerate(steps):
        d_a.copy_(torch.from_numpy(a * (1 + t)))          # (any non-zero byte: takes part)
        d_nv.fill_(float("nan"))
        if halves:
            ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
            if t in (0, 2):   # the pending half-step was enqueued under the old mask: LQRO_E_STATE
                assert L.lqro_set_active(ctx._h, None) == -4
                assert L.lqro_set_active_device(ctx._h, d_a.data_ptr()) == -4
            ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
        else:
            ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
        torch.cuda.synchronize()
        check(lqro_mod, ctx, a, d_nv.cpu().numpy(), ref, n, what=(t,))
        b = ctx.hull_builds()
        if t in (2, 3):
            assert len(b) >= 25 and not np.isin(b["i"], D).any() and not np.isin(b["j"], D).any(), t
    ctx.close()


HOT_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import lqro
a = np.load(sys.argv[2])
x, vg, masks = a["x"], a["vg"], a["masks"]
n = x.shape[0]
g = lqro.synthesize_gains()
c = lqro.Context(lqro.config(n, int(a["H"]), int(a["NP"]), flags=lqro.LQRO_FLAG_RECORDS | lqro.LQRO_FLAG_QHULL_ORDER))
c.set_gains(g["A"], g["B"], g["L"], g["E"])
d_a = torch.ones(n, dtype=torch.uint8, device="cuda")
c.set_active(d_a)
d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
sid = torch.cuda.current_stream().cuda_stream
nv, recs, carry, pairs = [], [], [], []
for t in range(len(masks)):
    d_a.copy_(torch.from_numpy(masks[t]))
    d_nv.fill_(float("nan"))
    c.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
    torch.cuda.synchronize()
    nv.append(d_nv.cpu().numpy())
    recs.append(c.records())
    carry.append(c.carry_normal())
    pairs.append(c.stats()["pairs"])
np.savez(sys.argv[3], nv=np.stack(nv), recs=np.stack(recs), carry=np.stack(carry), pairs=np.array(pairs))
"""


def test_hot_schedule_early_lp_off(lqro_mod, hot, tmp_path):
    """The same six steps with LQRO_EARLY_LP=0, in a child process."""
    x, vg, D, steps = hot
    n = HOT["n"]
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "hot.npz")
    np.savez(inp, x=x, vg=vg, masks=np.stack([a for a, _ in steps]), H=HOT["H"], NP=HOT["NP"])
    env = dict(os.environ, LQRO_EARLY_LP="0")
    r = subprocess.run([sys.executable, "-c", HOT_CHILD, PKG, inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    for t, (a, (nv_c, recs_c, carry_c)) in enumerate(steps):
        want, _ = ar.expand_records(a, recs_c, n)
        assert_records(lqro_mod, d["recs"][t], want, what=(t,))
        assert np.array_equal(_bits(d["nv"][t]), _bits(ar.expand_newv(a, nv_c, n))), t
        assert np.array_equal(_bits(d["carry"][t]), _bits(carry_c)), t
        assert d["pairs"][t] == ar.pairs(a), t


# 7 ------------------------------------------------------------------------
M = 4


@pytest.mark.parametrize("rule", RULES)
def test_with_obstacles(lqro_mod, orc, gains, rule):
    """4 obstacles with the agents' radii and responsibility 0.5: the oracle
    over the compacted agents + M bodies; the obstacle columns are not masked."""
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    a = ar.mask("mod3", N)
    xc, vc = ar.compact(a, x_all, vg)
    na = int(a.sum())
    ref = orc.steps(xc, vc, na, rule, steps=2)
    assert ((ref[0][1]["flags"][:, na - 1:] & lqro_mod.REC_PLANE) != 0).any()
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_active(a)
    ctx.set_obstacles(x_all[N:], responsibility=0.5)         # (the obstacle setter keeps the mask)
    for t in range(2):
        nv = step_nan(lqro_mod, ctx, x_all[:N], vg[:N])
        check(lqro_mod, ctx, a, nv, ref[t], N, m=M, what=(rule, t))
    ctx.close()


def test_with_culling(lqro_mod, oracle, orc, gains):
    """pyoracle.set_neighbors on the compacted swarm.  k and r are such that an
    inactive agent would have been among some active row's nearest k."""
    dist, k = 2.0, 3
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    a = ar.mask("mod3", N)
    on = ar.ids(a)
    d2 = ((x[:, None, :3] - x[None, :, :3]) ** 2).sum(2) + 1e9 * np.eye(N)
    near = np.argsort(d2, axis=1, kind="stable")[:, :k]
    assert any((a[near[i]] == 0).any() and (d2[i, near[i]] < dist * dist).all() for i in on)
    xc, vc = ar.compact(a, x, vg)
    oracle.set_neighbors(dist, k)
    try:
        nv_o, recs_o, carry_o = orc.steps(xc, vc, len(xc), "qhull")[0]
    finally:
        oracle.set_neighbors(0.0, 0)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_active(a)
    ctx.set_neighbors(dist, k)                                 # (the neighbour setter keeps the mask)
    nv = step_nan(lqro_mod, ctx, x, vg)
    recs = ctx.records().reshape(N, k)
    kept = 0
    for i in range(N):
        if not a[i]:                                           # an inactive row's list is all -1
            assert np.all(recs[i]["j"] == -1) and np.all(recs[i]["n_reach"] == -1) and not recs[i]["flags"].any()
            continue
        ic = int(np.nonzero(on == i)[0][0])
        ref_row = recs_o[ic][recs_o[ic]["n_reach"] >= 0].copy()
        c = len(ref_row)
        kept += c
        ref_row["i"], ref_row["j"] = i, on[ref_row["j"]]
        assert np.all(recs[i][c:]["n_reach"] == -1) and np.all(recs[i][c:]["j"] == -1)
        assert_records(lqro_mod, recs[i][:c][None], ref_row[None], what=(i,))
    assert ctx.stats()["pairs"] == kept and kept > 0
    assert np.array_equal(_bits(nv), _bits(ar.expand_newv(a, nv_o, N)))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_o))
    ctx.close()


def test_with_per_agent_gains(lqro_mod, oracle):
    """X = 12, per-agent gains: the row agent's own tables, compacted with it."""
    n, X, h = 12, 12, 40
    models = lqro_mod.perturbed_models(n)
    g = lqro_mod.synthesize_gains_batch(models, x_dim=X)
    AB = lqro_mod.synthesize_gains(x_dim=X)
    x, vg = lqro_mod.synthetic_swarm(n, box=2.5, seed=11, x_dim=X)
    a = ar.mask("mod3", n)
    on = ar.ids(a)
    T, NCF = np.zeros((len(on), h, 9)), np.zeros((len(on), h, 3, X))
    for r, i in enumerate(on):
        T[r], NCF[r] = oracle.tables(AB["A"], AB["B"], g["L"][i], g["E"][i], h, X=X)
    o = Oracle(oracle, None, h=h, npts=NP, tabs=(T, NCF), per_agent=True)
    xc, vc = ar.compact(a, x, vg)
    ref = o.steps(xc, vc, len(on), "qhull", steps=2)
    assert (ref[0][1]["flags"] & lqro_mod.REC_PLANE).any()
    ctx = lqro_mod.Context(lqro_mod.config(n, h, NP, x_dim=X, flags=_flags(lqro_mod, "qhull")))
    ctx.set_gains(AB["A"], AB["B"], g["L"], g["E"], per_agent=True)
    ctx.set_active(a)
    for t in range(2):
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, a, nv, ref[t], n, what=(t,))
    ctx.close()


def test_with_fence_and_user_planes(lqro_mod, oracle, orc, gains):
    """Fence and user planes are indexed by the global agent id and go ahead of
    the pair planes of the active rows; an inactive row gets none (its newV is
    +0.0 whatever they say)."""
    lo, hi, tau = (-1.2, -1.2, -1.4), (1.2, 1.2, 1.4), 2.0
    x, vg, a, ref = want_for(lqro_mod, orc, 11, "mod3", "qhull")
    rng = np.random.default_rng(5)
    user = []
    for i in range(N):        # 0..3 planes an agent, through its current velocity
        nrm = rng.normal(size=(i % 4, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) if len(nrm) else 1.0
        user.append(np.concatenate([np.tile(x[i, 3:6], (i % 4, 1)) - 0.2 * nrm, nrm], 1).astype(np.float32))
    f, faces = au.fence_planes(x, lo, hi, tau)
    head = [np.concatenate([f[i], user[i]]) for i in range(N)]
    on = ar.ids(a)
    xc, vc = ar.compact(a, x, vg)
    # the oracle's compacted records, walked with each active row's own head
    want_c, nv_c, carry = walk(lqro_mod, oracle, ref[0][1], xc, vc, len(on), 1.0, np.zeros(3),
                               head=[head[i] for i in on])
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_active(a)
    ctx.set_fence(lo, hi, tau)
    ctx.set_user_planes(user)
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, a, nv, (nv_c, want_c, carry), N, what="fence+user")
    assert (_bits(nv_c) != _bits(ref[0][0])).any()           # the head shows in a row
    ctx.close()


@pytest.mark.parametrize("world,mode,name", [(2, "block", "half"), (3, "block", "mid"), (2, "cyclic", "odd"),
                                             (3, "cyclic", "mod3")])
def test_row_shards(lqro_mod, orc, gains, world, mode, name):
    """Every shard takes the same global mask; one shard owns only inactive
    rows.  begin / the N x 4 row-normal table / end, two steps."""
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    a = ar.mask(name, N) if name != "mid" else ((np.arange(N) < 8) | (np.arange(N) >= 16)).astype(np.uint8)
    assert any(not a[lqro_mod.shard_row_ids(N, g, world, mode)].any() for g in range(world))
    xc, vc = ar.compact(a, x, vg)
    ref = orc.steps(xc, vc, len(xc), "qhull", steps=2)
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    ctxs = []
    for g in range(world):
        c = _ctx(lqro_mod, gains, N, "qhull", **lqro_mod.shard_rows(N, g, world, mode))
        c.set_active(a)
        ctxs.append(c)
    for t in range(2):
        tabs = [torch.full((N, 4), float("nan"), dtype=torch.float64, device="cuda") for _ in range(world)]
        newv = [torch.full((N, 3), float("nan"), dtype=torch.float64, device="cuda") for _ in range(world)]
        for g, c in enumerate(ctxs):
            c.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), tabs[g].data_ptr(), 0)
        torch.cuda.synchronize()
        whole = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        for g in range(world):   # the all-gather: each rank's own rows
            ids = torch.from_numpy(lqro_mod.shard_row_ids(N, g, world, mode).astype(np.int64)).cuda()
            whole[ids] = tabs[g][ids]
        torch.cuda.synchronize()
        tab = whole.cpu().numpy()
        assert np.array_equal(_bits(tab[a == 0]), _bits(np.zeros((int((a == 0).sum()), 4))))   # a row without a plane
        for g, c in enumerate(ctxs):
            c.step_device_end(whole.data_ptr(), newv[g].data_ptr(), 0)
        torch.cuda.synchronize()
        for g, c in enumerate(ctxs):
            ids = lqro_mod.shard_row_ids(N, g, world, mode)
            check(lqro_mod, c, a, newv[g].cpu().numpy(), ref[t], N, rows=ids, what=(t, g))
    for c in ctxs:
        c.close()


def clearance_want(a, x, n, lo=None, hi=None, rows=None):
    """tests/clearance_ref.py over the compacted arrays, the columns mapped
    back, the cleared record for an inactive row; the total over the active
    own rows."""
    on = ar.ids(a)
    rc, _ = cr.measure(x[on], len(on), RXY, RZ, lo=lo, hi=hi)
    for f in ("j_s2", "j_d2"):
        rc[f] = np.where(rc[f] >= 0, on[np.maximum(rc[f], 0)], -1)
    rc["hit"] = np.where(rc["hit"] >= 0, on[np.maximum(rc["hit"], 0)], -1)
    full = np.zeros(n, cr.ROW_DTYPE)
    full["s2_min"] = full["d2_min"] = full["fence_min"] = cr.INF
    full["j_s2"] = full["j_d2"] = full["fence_face"] = -1
    full["hit"] = -1
    full[on] = rc
    rows = np.arange(n) if rows is None else np.asarray(rows)
    own_on = np.array([i for i in rows if a[i]], np.int64)
    tot = cr.total(full[own_on], own_on) if len(own_on) else dict(cr.empty_total(), n_measured=1)
    return full[rows], tot


def audit_want(a, want_recs, nv, vg, tol, n, level=0):
    """tests/lp_audit_ref.py over the active rows' lists (the expected records'
    planes, the columns' global ids), the cleared record for an inactive row;
    the total over the active rows."""
    on = ar.ids(a)
    lists = au.assemble(want_recs[on], on, n, level=level)
    rows_on = au.rows(lists, nv, vg, tol, row_ids=on)
    full = np.zeros(n, au.ROW_DTYPE)
    full["viol_max"] = full["hard_viol_max"] = au.NINF
    full["i"] = np.arange(n)
    for f in ("k_viol", "kind_viol", "id_viol", "k_hard", "kind_hard", "id_hard"):
        full[f] = -1
    full[on] = rows_on
    return full, au.total(rows_on)


def test_monitor_and_audit(lqro_mod, orc, gains):
    tol = 1e-5
    x, vg, a, ref = want_for(lqro_mod, orc, 11, "mod3", "qhull")
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_monitor(1)
    ctx.set_lp_audit(1, tol)
    ctx.set_active(a)                                          # (after them: it keeps both settings)
    since_c, since_a = cr.empty_total(), au.empty_total()
    for t in range(2):
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, a, nv, ref[t], N, what=(t,))
        rows_w, tot_w = clearance_want(a, x, N)
        since_c = cr.fold(since_c, tot_w)
        last, acc = ctx.monitor()
        assert cc.same_rows(ctx.monitor_rows(), rows_w), t
        assert cc.same_total(last, tot_w) and cc.same_total(acc, since_c), (t, last, tot_w)
        assert tot_w["n_hit"] > 0
        want, _ = ar.expand_records(a, ref[t][1], N)
        arows_w, atot_w = audit_want(a, want, nv, vg, tol, N)
        since_a = au.fold(since_a, atot_w)
        alast, aacc = ctx.lp_audit()
        assert au.same_rows(ctx.lp_audit_rows(), arows_w), t
        assert au.same_total(alast, atot_w) and au.same_total(aacc, since_a), (t, alast, atot_w)
    # the explicit measurement reads the mask too; unmasked it sees the inactive agents again
    rows, tot = ctx.clearance(x)
    rows_w, tot_w = clearance_want(a, x, N)
    assert cc.same_rows(rows, rows_w) and cc.same_total(tot, tot_w)
    ctx.set_active(None)
    rows, tot = ctx.clearance(x)
    r_all, t_all = cr.measure(x, N, RXY, RZ)
    assert cc.same_rows(rows, r_all) and cc.same_total(tot, t_all) and t_all["n_hit"] > tot_w["n_hit"]
    ctx.close()


def hard_newv(a, want, vg, n):
    """tests/lp_hard_ref.py over each active row's list at LQRO_HARD_OBSTACLES:
    its obstacle columns' planes first, in column order, all of them hard, then
    its agent planes; an inactive row's newV is +0.0."""
    out = np.zeros((n, 3))
    both = 0
    for i in ar.ids(a):
        row = want[i]
        k = (row["flags"] & 1) != 0
        pl = np.concatenate([row["plane_point"], row["plane_normal"]], 1).astype(np.float32)
        ob = row["j"] >= n
        out[i] = hr.new_v(np.concatenate([pl[k & ob], pl[k & ~ob]]), vg[i], n_hard=int((k & ob).sum()))
        both += int((k & ob).any() and (k & ~ob).any())
    return out, both


@pytest.mark.parametrize("cull", [0, 6], ids=["all_pairs", "culling"])
def test_with_hard_obstacles(lqro_mod, oracle, orc, gains, cull):
    """LQRO_HARD_OBSTACLES under a mask: the LP takes a row's obstacle slots
    ahead of its agent slots (with culling: the list entries >= n_agents - 1),
    which relies on a skipped agent slot holding flag 0 and on the obstacle
    columns not being masked.  Records, carry and pairs against the oracle over
    the compacted agents + M bodies (agents' radii, responsibility 0.5); newV
    against tests/lp_hard_ref.py over the lists with the obstacle planes
    first; the audit's n_hard and records against tests/lp_audit_ref.py."""
    from test_gpu_hard_planes import obstacles_on_paths
    tol, dist = 1e-5, 2.0
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    obs = obstacles_on_paths(lqro_mod, x, M)       # ahead of agents 1, 6, 11, 16: two of them inactive below
    a = ar.mask("mod3", N)
    on = ar.ids(a)
    na = len(on)
    xc = np.concatenate([x[on], obs])
    vc = np.concatenate([vg[on], np.zeros((M, 3))])
    if cull:
        oracle.set_neighbors(dist, cull)
    try:
        nv_o, recs_o, carry_o = orc.steps(xc, vc, na, "qhull")[0]
    finally:
        oracle.set_neighbors(0.0, 0)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_lp_audit(1, tol)
    ctx.set_active(a)
    ctx.set_obstacles(obs, responsibility=0.5)
    ctx.set_hard_planes(lqro_mod.LQRO_HARD_OBSTACLES)
    if cull:
        ctx.set_neighbors(dist, cull)
    nv = step_nan(lqro_mod, ctx, x, vg)
    if not cull:
        want, _ = ar.expand_records(a, recs_o, N, M)
        nv_w, both = hard_newv(a, want, vg, N)
        check(lqro_mod, ctx, a, nv, (nv_o, recs_o, carry_o), N, m=M, nv_full=nv_w, what="hard obstacles")
    else:
        got = ctx.records().reshape(N, cull)
        want = np.zeros((N, cull), dtype=got.dtype)
        want["i"], want["j"], want["n_reach"] = np.arange(N)[:, None], -1, -1
        kept = 0
        for ic, i in enumerate(on):                # the compact row's kept neighbours, columns mapped back
            ref_row = recs_o[ic][recs_o[ic]["n_reach"] >= 0].copy()
            ref_row["i"] = i
            ref_row["j"] = [ar.global_column(a, int(jc), N) for jc in ref_row["j"]]
            want[i, :len(ref_row)] = ref_row
            kept += len(ref_row)
        assert_records(lqro_mod, got, want, what="hard obstacles, culled")
        assert (want["j"][on] >= N).any(), "no obstacle among the kept neighbours"
        assert ctx.stats()["pairs"] == kept
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_o))
        nv_w, both = hard_newv(a, want, vg, N)
        assert np.array_equal(_bits(nv), _bits(nv_w)), np.nonzero((_bits(nv) != _bits(nv_w)).any(1))[0]
    assert both >= 2, "no active row has obstacle and agent planes"
    soft = ar.expand_newv(a, nv_o, N)
    assert (_bits(nv_w) != _bits(soft)).any(), "the obstacle planes' place and hardness show in no row"
    arows_w, atot_w = audit_want(a, want, nv, vg, tol, N, level=3)
    assert arows_w["n_hard"][on].max() > 0 and not arows_w["n_hard"][a == 0].any()
    alast, _ = ctx.lp_audit()
    assert au.same_rows(ctx.lp_audit_rows(), arows_w)
    assert au.same_total(alast, atot_w), (alast, atot_w)
    ctx.close()


def test_culling_fallback_scan(lqro_mod, oracle, gains):
    """k_nbr past its 1,024 candidates in LDS: 1,700 agents all within range of
    one another, every third inactive, so an active row has 1,132 candidates
    and takes both of its global-memory scans under the mask."""
    n, h, npts, k, dist = 1700, 8, 16, 3, 50.0
    x, vg = lqro_mod.synthetic_swarm(n, box=6.0, seed=5)
    a = ar.mask("mod3", n)
    on = ar.ids(a)
    assert len(on) - 1 > 1024
    xc, vc = ar.compact(a, x, vg)
    o = Oracle(oracle, gains, h=h, npts=npts)          # (one thread: its carried normal in row order)
    oracle.set_neighbors(dist, k)
    try:
        nv_o, recs_o, carry_o = o.steps(xc, vc, len(on), "qhull")[0]
    finally:
        oracle.set_neighbors(0.0, 0)
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=h, npts=npts)
    ctx.set_active(a)
    ctx.set_neighbors(dist, k)
    nv = step_nan(lqro_mod, ctx, x, vg)
    got = ctx.records().reshape(n, k)
    want = np.zeros((n, k), dtype=got.dtype)
    want["i"], want["j"], want["n_reach"] = np.arange(n)[:, None], -1, -1
    for ic, i in enumerate(on):
        ref_row = recs_o[ic][recs_o[ic]["n_reach"] >= 0].copy()
        ref_row["i"], ref_row["j"] = i, on[ref_row["j"]]
        want[i, :len(ref_row)] = ref_row
    assert_records(lqro_mod, got, want, what="fallback scan")
    assert ctx.stats()["pairs"] == len(on) * k
    assert np.array_equal(_bits(nv), _bits(ar.expand_newv(a, nv_o, n)))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_o))
    ctx.close()


# 8 ------------------------------------------------------------------------
def test_python_hosts(lqro_mod, orc, gains):
    x, vg, a, ref = want_for(lqro_mod, orc, 11, "mod3", "qhull")
    full = ar.expand_newv(a, ref[0][0], N)
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x[i], vGoal=vg[i]) for i in range(N)], horizon=H, n_points=NP)
    sim.findMatrices()
    sim.set_active(a.astype(bool))
    try:
        sim.step()
    except lqro_mod.QhullMergeSuspect:
        pass
    got = np.stack([q.newV for q in sim.qlist])
    assert np.array_equal(_bits(got), _bits(full)) and not got[a == 0].any()
    sim.ctx.close()
    g = lqro_mod.synthesize_gains()
    loop = lqro_mod.DeviceLoop(x, vg, g, H, NP)
    d_a = torch.from_numpy(a.copy()).cuda()
    loop.set_active(d_a)
    assert loop.ctx._act_keep is d_a                           # the tensor is kept alive
    nv = loop.step()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(nv.cpu().numpy()), _bits(full))
    loop.close()


def test_cpp_host(lqro_mod, orc, tmp_path):
    """lqro::Simulator::setActive: mod3, cleared, half; the pair loop alone, so
    x stays and the carry chains."""
    if not os.path.exists(ACTIVE_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_active()
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=11)
    names = ("mod3", "all", "half")
    masks = np.stack([ar.mask(k, N) if k != "all" else np.full(N, 255, np.uint8) for k in names])
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([N, H, NP, len(names)], np.int32).tofile(f)
        x.tofile(f)
        vg.tofile(f)
        masks.tofile(f)
    r = subprocess.run([ACTIVE_MAIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(names), N, 3)
    carry = np.zeros(3)
    for t, k in enumerate(names):
        a = ar.mask(k, N)
        xc, vc = ar.compact(a, x, vg)
        nv_c, _, carry = orc.steps(xc, vc, len(xc), "qhull", carry=carry)[0]
        assert np.array_equal(_bits(out[t]), _bits(ar.expand_newv(a, nv_c, N))), t


# 9 ------------------------------------------------------------------------
def test_c3_size_masked_equals_parked(lqro_mod, gains):
    """N = 1024, H = 100, Qhull order, i % 4 == 3 inactive, GPU against GPU:
    the masked step equals the unmasked step over the parked swarm in the
    active rows' newV and the carry.  Four steps: the last two run the hot
    schedule (the work of the step two before is known)."""
    n, h = 1024, 100
    x, vg = lqro_mod.synthetic_swarm(n)
    a = (np.arange(n) % 4 != 3).astype(np.uint8)
    on = ar.ids(a)
    cfg = dict(flags=lqro_mod.LQRO_FLAG_QHULL_ORDER)
    masked = lqro_mod.Context(lqro_mod.config(n, h, NP, **cfg))
    parked = lqro_mod.Context(lqro_mod.config(n, h, NP, **cfg))
    for c in (masked, parked):
        c.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    masked.set_active(a)
    xp = ar.park(a, x)
    for t in range(4):
        nv_m = step_nan(lqro_mod, masked, x, vg)
        nv_p = _step(lqro_mod, parked, xp, vg)
        assert np.array_equal(_bits(nv_m[on]), _bits(nv_p[on])), (t, np.nonzero((_bits(nv_m) != _bits(nv_p)).any(1))[0][:8])
        assert np.array_equal(_bits(nv_m[a == 0]), _bits(np.zeros((n - len(on), 3)))), t
        assert np.array_equal(_bits(masked.carry_normal()), _bits(parked.carry_normal())), t
        sm, sp = masked.stats(), parked.stats()
        assert sm["pairs"] == len(on) * (len(on) - 1) and sm["inside"] == sp["inside"] > 0, (t, sm, sp)
    masked.close()
    parked.close()


# 10 -----------------------------------------------------------------------
def test_recycled_memory_and_setters(lqro_mod, orc, gains):
    """A mask set, cleared and set again between steps (the buffers come and
    go); lqro_set_obstacles with a mask in place renumbers the slots and keeps
    the mask; a failed call leaves the mask as it was."""
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    x, vgn = x_all[:N], vg[:N]
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    carry = np.zeros(3)
    L = lqro_mod.lib()
    for t, (name, obs) in enumerate((("mod3", 0), ("all", 0), ("half", 0), ("half", M), ("odd", M), ("odd", 0))):
        a = ar.mask(name, N)
        if t == 4:
            assert L.lqro_set_active(None, lqro_mod._p(a)) == -1       # LQRO_E_ARG: nothing changes
            with pytest.raises(ValueError):
                ctx.set_active(np.ones(N + 1, bool))
        ctx.set_active(None if name == "all" else a)
        if t in (3, 5):
            ctx.set_obstacles(x_all[N:] if obs else None, responsibility=0.5)
        bodies = x_all if obs else x
        xc, vc = ar.compact(a, bodies, vg if obs else vgn)
        ref = orc.steps(xc, vc, int(a.sum()), "qhull", carry=carry)[0]
        nv = step_nan(lqro_mod, ctx, x, vgn)
        check(lqro_mod, ctx, a, nv, ref, N, m=obs, what=(t, name, obs))
        carry = ref[2]
    ctx.close()
