"""Interaction classes (lqro_set_interaction, lqro_set_interaction_device; DESIGN
§6.18), bit for bit against tests/interaction_ref.py: the pair-local record
fields from one oracle step without a table, the factor-dependent fields, the
carried normal and each row's LP redone by its walk over the live slots.
Records (every field), newV, the pairs statistic and the carried normal, over
two consecutive steps.  tests/test_interaction_cpu.py pins the walk against the
oracle and states what the seeds must show; the same conditions are asserted
here, so a seed that does not meet them fails."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import active_ref as ar
import clearance_cases as cc
import clearance_ref as cr
import interaction_ref as ir
import lp_audit_ref as au
import lp_hard_ref as hr
from conftest import ROOT
from test_active_cpu import HOT
from test_gpu_obstacles import Oracle, _bits, _ctx, _flags, assert_records, obstacle_swarm
from test_interaction_cpu import SEEDS, assert_seed, expectation, local_for

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "lqr-obstacles_amd")
INTERACTION_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_interaction_main")
RULES = ("qhull", "canonical")
N, BOX, H, NP = 24, 3.0, 50, 100
RXY, RZ = 0.26, 0.75
E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def orc(oracle, gains):
    return Oracle(oracle, gains, h=H, npts=NP)


def step_nan(lqro, ctx, x, vg):
    """lqro_step into a newV prefilled with NaN."""
    nv = np.full((x.shape[0], 3), np.nan)
    x, vg = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(vg, np.float64)
    rc = lqro.lib().lqro_step(ctx._h, lqro._p(x), lqro._p(vg), lqro._p(nv))
    assert rc in (0, -9), rc   # (LQRO_E_QHMERGE: the step completed; the records say which pair)
    return nv


def snapshot(ctx, nv):
    return nv.tobytes(), ctx.records().tobytes(), ctx.carry_normal().tobytes(), ctx.stats()


def check(lqro, ctx, want, nv, pairs, rows=None, what=""):
    """One step's records, newV, carry and pairs counter against one entry of
    `expectation` (rows: the context's own, default all)."""
    recs_w, nv_w, carry_w, _ = want
    n = recs_w.shape[0]
    ids = np.arange(n) if rows is None else np.asarray(rows)
    got = ctx.records().reshape(len(ids), -1)
    assert_records(lqro, got, recs_w[ids], what=what)          # (a dead slot: i, j and zeros)
    assert np.array_equal(_bits(nv[ids]), _bits(nv_w[ids])), (what, np.nonzero((_bits(nv) != _bits(nv_w)).any(1))[0])
    if ctx.cfg.flags & lqro.LQRO_FLAG_QHULL_ORDER:              # (the canonical rule carries no normal)
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_w)), what
    assert ctx.stats()["pairs"] == pairs, (what, ctx.stats()["pairs"], pairs)


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_uniform_and_cleared_equal_no_table(lqro_mod, gains, rule):
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=16)
    c, share = ir.table("uniform")
    runs = {}
    for kind in ("never", "uniform", "cleared", "cleared_share"):
        ctx = _ctx(lqro_mod, gains, N, rule)
        if kind == "uniform":
            ctx.set_interaction(ir.classes(N, c), share)
        if kind.startswith("cleared"):
            ctx.set_interaction(ir.classes(N, 3), ir.table("weights")[1])
            if kind == "cleared":
                ctx.set_interaction(None, None)
            else:                                                # (share == NULL clears as cls == NULL does)
                assert lqro_mod.lib().lqro_set_interaction(ctx._h, lqro_mod._p(ir.classes(N, 3)), 3, None) == 0
        runs[kind] = [snapshot(ctx, step_nan(lqro_mod, ctx, x, vg)) for t in range(2)]
        ctx.close()
    for kind in ("uniform", "cleared", "cleared_share"):
        assert runs[kind] == runs["never"], kind
    assert runs["never"][0][3]["pairs"] == N * (N - 1)


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_ghost(lqro_mod, gains, rule):
    """Class 1 is avoided by nobody and avoids nobody: the class-0 rows are the
    same context's under lqro_set_active(cls == 0); a class-1 row's LP runs over
    no plane."""
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=16)
    c, share = ir.table("ghost")
    cls = ir.classes(N, c)
    tab, msk = _ctx(lqro_mod, gains, N, rule), _ctx(lqro_mod, gains, N, rule)
    tab.set_interaction(cls, share)
    msk.set_active(cls == 0)
    free = lqro_mod.calculate_new_v([np.zeros((0, 6), np.float32)] * N, vg)
    for t in range(2):
        nv_t, nv_m = step_nan(lqro_mod, tab, x, vg), step_nan(lqro_mod, msk, x, vg)
        rt, rm = tab.records().reshape(N, N - 1), msk.records().reshape(N, N - 1)
        assert rt[cls == 0].tobytes() == rm[cls == 0].tobytes() and (rt["flags"][cls == 0] != 0).any(), t
        assert rt[cls == 1].tobytes() == rm[cls == 1].tobytes() and not rt["flags"][cls == 1].any(), t
        assert np.array_equal(_bits(nv_t[cls == 0]), _bits(nv_m[cls == 0])), t
        assert np.array_equal(_bits(nv_t[cls == 1]), _bits(free[cls == 1])) and free[cls == 1].any(), t
        assert np.array_equal(_bits(tab.carry_normal()), _bits(msk.carry_normal())), t
        assert tab.stats() == msk.stats() and tab.stats()["pairs"] == 12 * 11, t
    tab.close()
    msk.close()


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(SEEDS))
def test_tables_against_the_reference(lqro_mod, oracle, orc, gains, name, rule):
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], rule)
    assert_seed(lqro_mod, local, fac, live, rule, share, what=(name, rule))
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_interaction(cls, share)
    for t in range(2):          # (the second step enters with the first's carry)
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want[t], nv, ir.pairs(cls, share, N), what=(name, rule, t))
        b = ctx.hull_builds()
        if len(b):               # no hull is built for a dead slot
            assert live[b["i"], b["j"] - (b["j"] > b["i"])].all(), (name, rule, t)
        assert len(ctx.hull_failures()) == 0 and len(ctx.qhmerge_pairs()) == 0
    ctx.close()


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [61, 63, 66])
def test_odd_sizes(lqro_mod, oracle, gains, n):
    """The class bytes are no whole number of words (61, 63, 66) and a row's
    columns cross the wave width (63 / 64 / 65 slots); `weights`."""
    o = Oracle(oracle, gains, h=H, npts=NP, threads=8)      # (only the pair-local fields are read)
    x, vg = lqro_mod.synthetic_swarm(n, box=4.5, seed=16)
    local = o.steps(x, vg, n, "qhull")[0][1]
    c, share = ir.table("weights")
    cls = ir.classes(n, c)
    fac, live = ir.factors(cls, share, n)
    inside = (local["flags"] & lqro_mod.REC_INSIDE) != 0
    assert (inside & live).any() and (inside & ~live).any()
    ctx = _ctx(lqro_mod, gains, n, "qhull")
    ctx.set_interaction(cls, share)
    carry = np.zeros(3)
    for t in range(2):
        want = ir.walk(lqro_mod, oracle, local, x, vg, n, fac, live, carry)
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want, nv, ir.pairs(cls, share, n), what=(n, t))
        carry = want[2]
    assert (local["flags"] & lqro_mod.REC_PLANE).any()
    ctx.close()


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_sixteen_classes(lqro_mod, oracle, orc, gains, rule):
    """C = LQRO_CLASSES_MAX, every class used; a quarter of the entries 0, the
    others drawn from (0, 1]."""
    c = ir.CLASSES_MAX
    rng = np.random.default_rng(16)
    share = rng.uniform(0.0, 1.0, (c, c))
    share[rng.uniform(size=(c, c)) < 0.25] = 0.0
    share[3, 5], share[5, 3] = 1.0, np.nextafter(0.0, 1.0)      # the ends of the range: both live
    cls = rng.permutation(np.arange(N) % c).astype(np.uint8)
    assert len(np.unique(cls)) == c
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, "c16", 16, rule, cls=cls,
                                                              table=(c, share))
    assert 0 < live.sum() < live.size
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_interaction(cls, share)
    for t in range(2):
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want[t], nv, ir.pairs(cls, share, N), what=(rule, t))
    ctx.close()


# 6 ------------------------------------------------------------------------
def test_row_with_nothing_to_avoid_keeps_its_fence(lqro_mod, oracle, orc, gains):
    """Agent 5 is alone in class 1, which ignores everybody (and everybody
    avoids it with share 1.0): its row is all dead, it still gets its fence
    planes and its LP runs."""
    lo, hi, tau = (-1.2, -1.2, -1.4), (1.2, 1.2, 1.4), 2.0
    cls = np.zeros(N, np.uint8)
    cls[5] = 1
    share = np.array([[0.5, 1.0], [0.0, 0.0]])
    x, vg, (_, local, _) = local_for(lqro_mod, orc, 16, "qhull")
    f, faces = au.fence_planes(x, lo, hi, tau)
    fac, live = ir.factors(cls, share, N)
    recs_w, nv_w, carry_w, cnt = ir.walk(lqro_mod, oracle, local, x, vg, N, fac, live, np.zeros(3), head=f)
    assert cnt[5] == 0 and not live[5].any() and len(f[5]) > 0
    free = oracle.newv(np.zeros((0, 6), np.float32), vg[5], 100.0)
    assert (_bits(nv_w[5]) != _bits(free)).any()              # the fence shows in the row
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_fence(lo, hi, tau)
    ctx.set_interaction(cls, share)                             # (it keeps the fence)
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, (recs_w, nv_w, carry_w, cnt), nv, ir.pairs(cls, share, N), what="lone")
    assert ir.pairs(cls, share, N) == (N - 1) * (N - 1)
    # no live pair at all: the carry stays as it entered, every row's LP over no pair plane
    ctx.set_fence(None, None, 0.0)
    ctx.set_interaction(np.zeros(N, np.uint8), np.zeros((1, 1)))
    carry = np.array([0.6, 0.0, -0.8])
    ctx.carry_normal(carry)
    nv = step_nan(lqro_mod, ctx, x, vg)
    free = lqro_mod.calculate_new_v([np.zeros((0, 6), np.float32)] * N, vg)
    assert np.array_equal(_bits(nv), _bits(free))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry))
    st = ctx.stats()
    assert (st["pairs"], st["planes"], st["inside"], st["sum_n_reach"]) == (0, 0, 0, 0) and len(ctx.hull_builds()) == 0
    assert not ctx.records()["flags"].any()
    ctx.close()


# 7 ------------------------------------------------------------------------
def test_errors_and_a_failed_call_changes_nothing(lqro_mod, oracle, orc, gains):
    name = "weights"
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], "qhull")
    L, p = lqro_mod.lib(), lqro_mod._p
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_interaction(cls, share)
    d_cls = torch.from_numpy(cls.copy()).cuda()
    bad = []
    for c in (0, -1, 17):
        sh = np.full((max(c, 1), max(c, 1)), 0.5)
        bad.append((L.lqro_set_interaction(ctx._h, p(cls), c, p(sh)), L.lqro_set_interaction_device(ctx._h, d_cls.data_ptr(), c, p(sh))))
    for v in (1.0000000000000002, -1e-300, np.nan, np.inf, -np.inf, -0.5):
        sh = share.copy()
        sh[2, 1] = v
        bad.append((L.lqro_set_interaction(ctx._h, p(cls), 3, p(sh)), L.lqro_set_interaction_device(ctx._h, d_cls.data_ptr(), 3, p(sh))))
    over = cls.copy()
    over[N - 1] = 3
    bad.append((L.lqro_set_interaction(ctx._h, p(over), 3, p(share)), E_ARG))
    assert all(b == (E_ARG, E_ARG) for b in bad), bad
    with pytest.raises(ValueError):
        ctx.set_interaction(np.zeros(N + 1, np.uint8), share)
    for t in range(2):          # the table set before the failed calls is still the one in force
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want[t], nv, ir.pairs(cls, share, N), what=("after failed calls", t))
    # a pending half-step was enqueued under the old table: LQRO_E_STATE, then the step ends as it began
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_tab = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
    d_nv = torch.full((N, 3), float("nan"), dtype=torch.float64, device="cuda")
    ctx.carry_normal(np.zeros(3))
    ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), 0)
    assert L.lqro_set_interaction(ctx._h, None, 0, None) == E_STATE
    assert L.lqro_set_interaction(ctx._h, p(cls), 3, p(share)) == E_STATE
    assert L.lqro_set_interaction_device(ctx._h, d_cls.data_ptr(), 3, p(share)) == E_STATE
    ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), 0)
    torch.cuda.synchronize()
    check(lqro_mod, ctx, want[0], d_nv.cpu().numpy(), ir.pairs(cls, share, N), what="after E_STATE")
    ctx.close()


# 8 ------------------------------------------------------------------------
def test_python_hosts(lqro_mod, oracle, orc, gains):
    name = "priority"
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], "qhull")
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x[i], vGoal=vg[i]) for i in range(N)], horizon=H, n_points=NP)
    sim.findMatrices()
    sim.set_interaction(cls, share)
    try:
        sim.step()
    except lqro_mod.QhullMergeSuspect:
        pass
    got = np.stack([q.newV for q in sim.qlist])
    assert np.array_equal(_bits(got), _bits(want[0][1]))
    sim.ctx.close()
    g = lqro_mod.synthesize_gains()
    loop = lqro_mod.DeviceLoop(x, vg, g, H, NP)
    d_cls = torch.from_numpy(cls.copy()).cuda()
    loop.set_interaction(d_cls, share, device=True)
    assert loop.ctx._ix_keep is d_cls                          # the tensor is kept alive
    nv = loop.step()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(nv.cpu().numpy()), _bits(want[0][1]))
    loop.close()


def test_cpp_host(lqro_mod, oracle, orc, tmp_path):
    """lqro::Simulator::setInteraction: weights, cleared, weights with the
    classes shifted by one; the pair loop alone, so x stays and the carry chains."""
    if not os.path.exists(INTERACTION_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_interaction()
    seed = SEEDS["weights"]
    x, vg, (_, local, _) = local_for(lqro_mod, orc, seed, "qhull")
    c, share = ir.table("weights")
    steps = [ir.classes(N, c), np.full(N, 255, np.uint8), ((np.arange(N) + 1) % c).astype(np.uint8)]
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([N, H, NP, len(steps), c], np.int32).tofile(f)
        x.tofile(f)
        vg.tofile(f)
        share.tofile(f)
        np.stack(steps).tofile(f)
    r = subprocess.run([INTERACTION_MAIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(steps), N, 3)
    carry = np.zeros(3)
    for t, k in enumerate(steps):
        if k[0] == 255:
            fac, live = ir.factors(np.zeros(N, np.uint8), np.full((1, 1), 0.5), N)
        else:
            fac, live = ir.factors(k, share, N)
        _, nv_w, carry, _ = ir.walk(lqro_mod, oracle, local, x, vg, N, fac, live, carry)
        assert np.array_equal(_bits(out[t]), _bits(nv_w)), t


# 9 ------------------------------------------------------------------------
HOT_STEPS = 4
HOT_TABLE = "weights"


def hot_classes(t, n):
    """Steps 0-1: i % 3; steps 2-3: (i + 1) % 3."""
    return ((np.arange(n) + (1 if t >= 2 else 0)) % 3).astype(np.uint8)


@pytest.fixture(scope="module")
def hot(lqro_mod, oracle, gains):
    """The 257-agent hot swarm of tests/test_active_cpu.py under `weights`; the
    class bytes change between step 1 and step 2.  Per step (classes, walk)."""
    n = HOT["n"]
    x, vg = lqro_mod.synthetic_swarm(n, box=HOT["box"], seed=HOT["seed"])
    o = Oracle(oracle, gains, h=HOT["H"], npts=HOT["NP"], threads=8)
    local = o.steps(x, vg, n, "qhull")[0][1]
    c, share = ir.table(HOT_TABLE)
    inside = (local["flags"] & lqro_mod.REC_INSIDE) != 0
    steps, carry, lives = [], np.zeros(3), {}
    for t in range(HOT_STEPS):
        cls = hot_classes(t, n)
        key = int(t >= 2)
        if key not in lives:
            lives[key] = ir.factors(cls, share, n)
        fac, live = lives[key]
        want = ir.walk(lqro_mod, oracle, local, x, vg, n, fac, live, carry)
        carry = want[2]
        steps.append((cls, want, ir.pairs(cls, share, n), live))
    l0, l1 = lives[0][1], lives[1][1]
    assert (inside & l0 & ~l1).any(), "no pair inside-hull in step 1 is dead in step 2"
    assert (inside & ~l0 & l1).any(), "no dead pair of step 1 comes alive (inside-hull) in step 2"
    return x, vg, share, steps


@pytest.mark.parametrize("hot_split", ["1", "0"])
@pytest.mark.parametrize("halves", [False, True], ids=["step_device", "begin_end"])
def test_hot_schedule_device_classes(lqro_mod, gains, hot, monkeypatch, halves, hot_split):
    """257 x 256 slots: the hot schedule from the third step, which is the
    first with the rewritten classes.  The class bytes are a torch tensor given
    once and rewritten in place on the stream between the steps."""
    monkeypatch.setenv("LQRO_HOT_SPLIT", hot_split)
    x, vg, share, steps = hot
    n = HOT["n"]
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=HOT["H"], npts=HOT["NP"])
    d_cls = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ctx.set_interaction(d_cls, share, device=True)
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    L = lqro_mod.lib()
    for t, (cls, want, pairs, live) in enumerate(steps):
        over = cls.copy()
        over[cls == 2] = 2 + 7 * t                       # (a device byte >= n_classes reads as n_classes - 1)
        d_cls.copy_(torch.from_numpy(over))
        d_nv.fill_(float("nan"))
        if halves:
            ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
            if t in (0, 2):   # the pending half-step was enqueued under the old table: LQRO_E_STATE
                assert L.lqro_set_interaction(ctx._h, None, 0, None) == E_STATE
            ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
        else:
            ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
        torch.cuda.synchronize()
        check(lqro_mod, ctx, want, d_nv.cpu().numpy(), pairs, what=(t,))
        b = ctx.hull_builds()
        assert len(b) > 0 and live[b["i"], b["j"] - (b["j"] > b["i"])].all(), t
    ctx.close()


HOT_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import lqro
a = np.load(sys.argv[2])
x, vg, classes, share = a["x"], a["vg"], a["classes"], a["share"]
n = x.shape[0]
g = lqro.synthesize_gains()
c = lqro.Context(lqro.config(n, int(a["H"]), int(a["NP"]), flags=lqro.LQRO_FLAG_RECORDS | lqro.LQRO_FLAG_QHULL_ORDER))
c.set_gains(g["A"], g["B"], g["L"], g["E"])
d_cls = torch.zeros(n, dtype=torch.uint8, device="cuda")
c.set_interaction(d_cls, share, device=True)
d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
sid = torch.cuda.current_stream().cuda_stream
nv, recs, carry, pairs = [], [], [], []
for t in range(len(classes)):
    d_cls.copy_(torch.from_numpy(classes[t]))
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
    """The same four steps with LQRO_EARLY_LP=0, in a child process."""
    x, vg, share, steps = hot
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "hot.npz")
    np.savez(inp, x=x, vg=vg, classes=np.stack([k for k, *_ in steps]), share=share, H=HOT["H"], NP=HOT["NP"])
    env = dict(os.environ, LQRO_EARLY_LP="0")
    r = subprocess.run([sys.executable, "-c", HOT_CHILD, PKG, inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    for t, (cls, (recs_w, nv_w, carry_w, _), pairs, live) in enumerate(steps):
        assert_records(lqro_mod, d["recs"][t], recs_w, what=(t,))
        assert np.array_equal(_bits(d["nv"][t]), _bits(nv_w)), t
        assert np.array_equal(_bits(d["carry"][t]), _bits(carry_w)), t
        assert d["pairs"][t] == pairs, t


# 10 -----------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_with_the_mask(lqro_mod, oracle, orc, gains, rule):
    """The composition rule: live = row active, column active, share > 0.  An
    inactive row's newV is +0.0, an all-dead active row's the LP's."""
    name = "weights"
    a = ar.mask("mod3", N)
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], rule, active=a)
    plain, _ = expectation(lqro_mod, oracle, orc, name, SEEDS[name], rule)
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_interaction(cls, share)
    ctx.set_active(a)                                           # (each setter keeps the other's arrays)
    for t in range(2):
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want[t], nv, ir.pairs(cls, share, N, active=a), what=(rule, t))
        assert not np.signbit(nv[a == 0]).any() and (nv[a == 0] == 0.0).all()
    ctx.set_active(None)                                        # the table stays
    ctx.carry_normal(np.zeros(3))
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, plain[0], nv, ir.pairs(cls, share, N), what=(rule, "mask cleared"))
    ctx.close()


M = 4


def hard_newv(recs, vg, n):
    """tests/lp_hard_ref.py over each row's list at LQRO_HARD_OBSTACLES: its
    obstacle columns' planes first, in column order, all of them hard, then its
    agent planes."""
    out = np.zeros((n, 3))
    for i in range(n):
        row = recs[i]
        k = (row["flags"] & 1) != 0
        pl = np.concatenate([row["plane_point"], row["plane_normal"]], 1).astype(np.float32)
        ob = row["j"] >= n
        out[i] = hr.new_v(np.concatenate([pl[k & ob], pl[k & ~ob]]), vg[i], n_hard=int((k & ob).sum()))
    return out


def test_with_hard_obstacles(lqro_mod, oracle, orc, gains):
    """Obstacle columns keep their own responsibility and are never ignored.
    Class-0 rows see 0.5 everywhere, class-1 rows ignore class 0: against the
    reference (the oracle over agents + M bodies, walked), and the obstacle
    columns and the class-0 rows bit-identical to a context without the table
    (the canonical rule: no carried normal crosses the rows)."""
    from test_gpu_hard_planes import obstacles_on_paths
    rule = "canonical"
    x, vg, _ = local_for(lqro_mod, orc, 16, rule)
    obs = obstacles_on_paths(lqro_mod, x, M)
    x_all = np.concatenate([x, obs])
    vg_all = np.concatenate([vg, np.zeros((M, 3))])
    local = orc.steps(x_all, vg_all, N, rule)[0][1]
    share = np.array([[0.5, 0.5], [0.0, 0.5]])
    cls = ir.classes(N, 2)
    fac, live = ir.factors(cls, share, N, m=M, resp=0.75)
    recs_w, _, carry_w, cnt = ir.walk(lqro_mod, oracle, local, x_all, vg_all, N, fac, live, np.zeros(3))
    assert ((recs_w["flags"][:, N - 1:] & lqro_mod.REC_PLANE) != 0).any()
    nv_w = hard_newv(recs_w, vg, N)
    out = {}
    for kind in ("table", "plain"):
        ctx = _ctx(lqro_mod, gains, N, rule)
        ctx.set_lp_audit(1, 1e-5)
        if kind == "table":
            ctx.set_interaction(cls, share)
        ctx.set_obstacles(obs, responsibility=0.75)               # (the obstacle setter keeps the table)
        ctx.set_hard_planes(lqro_mod.LQRO_HARD_OBSTACLES)
        nv = step_nan(lqro_mod, ctx, x, vg)
        out[kind] = (nv, ctx.records().reshape(N, -1).copy(), ctx.lp_audit_rows().copy())
        if kind == "table":
            check(lqro_mod, ctx, (recs_w, nv_w, carry_w, cnt), nv, ir.pairs(cls, share, N, m=M), what="hard obstacles")
            assert np.array_equal(out[kind][2]["m"], cnt) and out[kind][2]["n_hard"].max() > 0
        ctx.close()
    (nv_t, r_t, _), (nv_p, r_p, _) = out["table"], out["plain"]
    assert r_t[:, N - 1:].tobytes() == r_p[:, N - 1:].tobytes()
    assert r_t[cls == 0].tobytes() == r_p[cls == 0].tobytes()
    assert np.array_equal(_bits(nv_t[cls == 0]), _bits(nv_p[cls == 0]))
    assert (_bits(nv_t[cls == 1]) != _bits(nv_p[cls == 1])).any()


def culled(lqro, oracle, local, x, vg, n, cls, share, dist, k, carry, active=None):
    """The culled step's expectation: row i keeps orc_neighbors' choice among
    its non-ignored active agents (slot q: its q-th kept neighbour, ascending;
    an empty slot: j = -1, n_reach = -1), the pair-local fields are the
    uncalled pair's, the rest is the walk's.  Also the kept count."""
    fac_f, live_f = ir.factors(cls, share, n, active=active)
    K = min(k, n - 1)
    loc = np.zeros((n, K), local.dtype)
    fac, live = np.zeros((n, K)), np.zeros((n, K), bool)
    loc["i"], loc["j"] = np.arange(n)[:, None], -1
    for i in range(n):
        cand = np.array([ir.column(i, q) for q in range(n - 1) if live_f[i, q]], int)
        if not len(cand):
            continue
        sel = oracle.neighbors(np.concatenate([x[i:i + 1], x[cand]]), 0, dist, k)[1:]
        for q, j in enumerate(cand[sel != 0]):
            loc[i, q] = local[i, j - (j > i)]
            fac[i, q], live[i, q] = fac_f[i, j - (j > i)], True
    recs, nv, carry, cnt = ir.walk(lqro, oracle, loc, x, vg, n, fac, live, carry, active=active)
    recs["n_reach"][~live] = -1
    return (recs, nv, carry, cnt), int(live.sum()), live_f


def test_with_culling(lqro_mod, oracle, orc, gains):
    """K = 6: a column the row ignores is no candidate and uses up no slot."""
    dist, k = 2.0, 6
    name = "weights"
    _, (x, vg, cls, share, _, _, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], "qhull")
    want0, kept, live_f = culled(lqro_mod, oracle, local, x, vg, N, cls, share, dist, k, np.zeros(3))
    # an ignored agent would have been among some row's nearest k
    d2 = ((x[:, None, :3] - x[None, :, :3]) ** 2).sum(2) + 1e9 * np.eye(N)
    near = np.argsort(d2, axis=1, kind="stable")[:, :k]
    assert any((d2[i, near[i]] < dist * dist).all() and not all(live_f[i, j - (j > i)] for j in near[i]) for i in range(N))
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_interaction(cls, share)
    ctx.set_neighbors(dist, k)                                  # (the neighbour setter keeps the table)
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, want0, nv, kept, what="culling")
    want1, kept, _ = culled(lqro_mod, oracle, local, x, vg, N, cls, share, dist, k, want0[2])
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, want1, nv, kept, what="culling, step 2")
    assert kept > 0
    ctx.close()


def test_culling_fallback_scan(lqro_mod, oracle, gains):
    """k_nbr past its 1,024 candidates in LDS (test_gpu_active's N): class 2 is
    a ghost, classes 0 and 1 see each other with 0.25 / 0.75, so a row of theirs
    has 1,132 candidates and takes both global-memory scans under the table."""
    n, h, npts, k, dist = 1700, 8, 16, 3, 50.0
    x, vg = lqro_mod.synthetic_swarm(n, box=6.0, seed=5)
    cls = ir.classes(n, 3)
    share = np.array([[0.5, 0.25, 0.0], [0.75, 0.5, 0.0], [0.0, 0.0, 0.0]])
    a = (cls != 2).astype(np.uint8)
    on = ar.ids(a)
    assert len(on) - 1 > 1024
    xc, vc = ar.compact(a, x, vg)
    o = Oracle(oracle, gains, h=h, npts=npts)
    oracle.set_neighbors(dist, k)
    try:
        _, recs_o, _ = o.steps(xc, vc, len(on), "qhull")[0]
    finally:
        oracle.set_neighbors(0.0, 0)
    loc = np.zeros((n, k), recs_o.dtype)
    loc["i"], loc["j"] = np.arange(n)[:, None], -1
    fac, live = np.zeros((n, k)), np.zeros((n, k), bool)
    for ic, i in enumerate(on):
        row = recs_o[ic][recs_o[ic]["n_reach"] >= 0].copy()
        row["i"], row["j"] = i, on[row["j"]]
        loc[i, :len(row)] = row
        fac[i, :len(row)], live[i, :len(row)] = share[cls[i], cls[row["j"]]], True
    recs_w, nv_w, carry_w, cnt = ir.walk(lqro_mod, oracle, loc, x, vg, n, fac, live, np.zeros(3))
    recs_w["n_reach"][~live] = -1
    assert (fac[live] == 0.25).any() and (fac[live] == 0.75).any()
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=h, npts=npts)
    ctx.set_interaction(cls, share)
    ctx.set_neighbors(dist, k)
    nv = step_nan(lqro_mod, ctx, x, vg)
    check(lqro_mod, ctx, (recs_w, nv_w, carry_w, cnt), nv, len(on) * k, what="fallback scan")
    ctx.close()


def test_with_per_agent_gains(lqro_mod, oracle):
    """X = 12, per-agent gains: the hot launches' and the hulls' factor with
    the row agent's own tables."""
    n, X, h = 12, 12, 40
    models = lqro_mod.perturbed_models(n)
    g = lqro_mod.synthesize_gains_batch(models, x_dim=X)
    AB = lqro_mod.synthesize_gains(x_dim=X)
    x, vg = lqro_mod.synthetic_swarm(n, box=2.5, seed=11, x_dim=X)
    T, NCF = np.zeros((n, h, 9)), np.zeros((n, h, 3, X))
    for i in range(n):
        T[i], NCF[i] = oracle.tables(AB["A"], AB["B"], g["L"][i], g["E"][i], h, X=X)
    o = Oracle(oracle, None, h=h, npts=NP, tabs=(T, NCF), per_agent=True)
    local = o.steps(x, vg, n, "qhull")[0][1]
    c, share = ir.table("weights")
    cls = ir.classes(n, c)
    fac, live = ir.factors(cls, share, n)
    inside = (local["flags"] & lqro_mod.REC_INSIDE) != 0
    assert (inside & live & (fac != 0.5)).any()
    ctx = lqro_mod.Context(lqro_mod.config(n, h, NP, x_dim=X, flags=_flags(lqro_mod, "qhull")))
    ctx.set_gains(AB["A"], AB["B"], g["L"], g["E"], per_agent=True)
    ctx.set_interaction(cls, share)
    carry = np.zeros(3)
    for t in range(2):
        want = ir.walk(lqro_mod, oracle, local, x, vg, n, fac, live, carry)
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want, nv, ir.pairs(cls, share, n), what=(t,))
        carry = want[2]
    ctx.close()


@pytest.mark.parametrize("world,mode", [(2, "block"), (3, "cyclic")])
def test_row_shards(lqro_mod, oracle, orc, gains, world, mode):
    """Every shard takes the same class bytes and table; begin / the N x 4
    row-normal table / end, two steps, the normal exchanged between the ranks."""
    name = "priority"
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], "qhull")
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vg.copy()).cuda()
    ctxs = []
    for g in range(world):
        c = _ctx(lqro_mod, gains, N, "qhull", **lqro_mod.shard_rows(N, g, world, mode))
        c.set_interaction(cls, share)
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
        for g, c in enumerate(ctxs):
            c.step_device_end(whole.data_ptr(), newv[g].data_ptr(), 0)
        torch.cuda.synchronize()
        for g, c in enumerate(ctxs):
            ids = lqro_mod.shard_row_ids(N, g, world, mode)
            rows = [int(i) for i in ids]
            check(lqro_mod, c, want[t], newv[g].cpu().numpy(), ir.pairs(cls, share, N, rows=rows), rows=ids, what=(t, g))
    for c in ctxs:
        c.close()


def test_monitor_and_audit(lqro_mod, oracle, orc, gains):
    """Clearance measures bodies, not intentions: its rows and totals are the
    ones without a table.  The audit follows the slots: m is the walked plane
    count."""
    tol = 1e-5
    name = "teams"
    want, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], "qhull")
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_monitor(1)
    ctx.set_lp_audit(1, tol)
    ctx.set_interaction(cls, share)                             # (after them: it keeps both settings)
    r_all, t_all = cr.measure(x, N, RXY, RZ)
    since = cr.empty_total()
    for t in range(2):
        nv = step_nan(lqro_mod, ctx, x, vg)
        check(lqro_mod, ctx, want[t], nv, ir.pairs(cls, share, N), what=(t,))
        since = cr.fold(since, t_all)
        last, acc = ctx.monitor()
        assert cc.same_rows(ctx.monitor_rows(), r_all), t
        assert cc.same_total(last, t_all) and cc.same_total(acc, since), (t, last, t_all)
        arows = ctx.lp_audit_rows()
        assert np.array_equal(arows["m"], want[t][3]) and (want[t][3] < N - 1).all(), t
        lists = au.assemble(want[t][0], np.arange(N), N)
        arows_w = au.rows(lists, nv, vg, tol, row_ids=np.arange(N))
        assert au.same_rows(arows, arows_w), t
        alast, _ = ctx.lp_audit()
        assert au.same_total(alast, au.total(arows_w)), t
    rows, tot = ctx.clearance(x)                                # the explicit measurement does not see it either
    assert cc.same_rows(rows, r_all) and cc.same_total(tot, t_all) and t_all["n_hit"] > 0
    ctx.close()
