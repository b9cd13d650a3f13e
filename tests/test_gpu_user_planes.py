"""Fence and user half-planes ahead of the pair planes in each row's LP
(lqro_set_fence, lqro_set_user_planes, lqro_set_user_planes_device), bit for
bit.

The expected newV of a row is the oracle's LP alone (pyoracle.newv) over
concat(fence_i, user_i, pair planes of row i): the pair planes are the step's
own records (their parity with the oracle is pinned by the rest of the
suite), the fence planes are restated here in numpy from lqro.h's formula.
Every comparison is on the bit patterns, over every row, rows with
inside-hull pairs included.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

import lp_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "lqr-obstacles_amd")
RULES = ("qhull", "canonical")
SWARM = dict(n=24, box=3.0, seed=11)     # dense: inside-hull pairs
H, NP = 50, 100


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _flags(lqro, rule, records=True):
    return (lqro.LQRO_FLAG_RECORDS if records else 0) | (lqro.LQRO_FLAG_QHULL_ORDER if rule == "qhull" else 0)


def fence_planes(x, lo, hi, tau, m=(0.26, 0.26, 0.75)):
    """lqro_set_fence's planes for every agent, (N, faces, 6) float32: axis x,
    y, z, lower face then upper, faces at infinity left out; the bound in
    fp64 in the header's order, rounded once."""
    out = []
    for a in range(3):
        if not np.isinf(lo[a]):
            p = np.zeros((x.shape[0], 6), np.float32)
            p[:, a] = (((lo[a] + m[a]) - x[:, a]) / tau).astype(np.float32)
            p[:, 3 + a] = 1.0
            out.append(p)
        if not np.isinf(hi[a]):
            p = np.zeros((x.shape[0], 6), np.float32)
            p[:, a] = (((hi[a] - m[a]) - x[:, a]) / tau).astype(np.float32)
            p[:, 3 + a] = -1.0
            out.append(p)
    return np.stack(out, 1) if out else np.zeros((x.shape[0], 0, 6), np.float32)


def pair_planes(recs, nrows):
    """Per row the emitted pair planes in record order, (m, 6) float32."""
    r = recs.reshape(nrows, -1)
    out = []
    for row in r:
        k = (row["flags"] & 1) != 0
        out.append(np.concatenate([row["plane_point"][k], row["plane_normal"][k]], 1).astype(np.float32))
    return out


def expected_newv(oracle, recs, row_ids, vg, fence=None, user=None, user_first=False):
    """(len(row_ids), 3): the oracle's LP over fence_i, user_i, pair planes."""
    pp = pair_planes(recs, len(row_ids))
    out = np.zeros((len(row_ids), 3))
    for k, i in enumerate(row_ids):
        head = [fence[i] if fence is not None else np.zeros((0, 6), np.float32),
                np.asarray(user[i], np.float32).reshape(-1, 6) if user is not None else np.zeros((0, 6), np.float32)]
        if user_first:
            head.reverse()
        out[k] = oracle.newv(np.concatenate(head + [pp[k]]), vg[i], 100.0)
    return out


def user_planes_for(x, seed=5):
    """0 to 5 planes per agent from lp_cases' families, moved to the agent's
    velocity; agents 0-2 have none, 3-5 have five."""
    rng = np.random.default_rng(seed)
    n = x.shape[0]
    counts = np.concatenate([[0, 0, 0, 5, 5, 5], rng.integers(0, 6, size=n - 6)])
    out = []
    for i, m in enumerate(counts):
        fam = lp_cases.FAMILIES[i % len(lp_cases.FAMILIES)]
        c = lp_cases._FAMILY_FN[fam](rng, int(m), i).astype(np.float32).reshape(-1, 6)
        if fam != "sphere":   # (the sphere family's planes sit at the LP's speed limit around the origin)
            c[:, :3] += x[i, 3:6].astype(np.float32)
        out.append(c)
    return out


def box_for(x):
    """A box with two agents outside (beyond the lower x face), the agent of
    largest x within m of the upper x face, the rest inside."""
    xs = np.sort(x[:, 0])
    lo = np.array([0.5 * (xs[1] + xs[2]), -2.0, -2.5])
    hi = np.array([xs[-1] + 0.1, 2.0, 2.5])
    return lo, hi


@pytest.fixture(scope="module")
def swarm(lqro_mod):
    x, vg = lqro_mod.synthetic_swarm(SWARM["n"], box=SWARM["box"], seed=SWARM["seed"])
    return x, vg, user_planes_for(x)


def _ctx(lqro, gains, n, flags, h=H, npts=NP, **kw):
    c = lqro.Context(lqro.config(n, h, npts, flags=flags, **kw))
    c.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    return c


def _step(lqro, ctx, x, vg):
    """ctx.step's newV, also when it reports a merge-suspect pair (the step
    completed; the LP saw the planes the records hold)."""
    try:
        return ctx.step(x, vg)
    except lqro.QhullMergeSuspect as e:
        return e.newv


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_user_planes_small_step(lqro_mod, oracle, gains, swarm, rule):
    x, vg, user = swarm
    n = x.shape[0]
    assert sum(len(u) == 0 for u in user) >= 3 and sum(len(u) == 5 for u in user) >= 3
    assert max(len(u) for u in user) == 5
    plain = _ctx(lqro_mod, gains, n, _flags(lqro_mod, rule))
    p1 = _step(lqro_mod, plain, x, vg)
    prec = plain.records()
    assert plain.stats()["inside"] > 0
    p2 = _step(lqro_mod, plain, x, vg)
    plain.close()
    ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, rule))
    ctx.set_user_planes(user)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    assert len(recs) == n * (n - 1) and recs.tobytes() == prec.tobytes()   # the pair path does not see them
    want = expected_newv(oracle, recs, range(n), vg, user=user)
    assert np.array_equal(_bits(nv), _bits(want)), np.nonzero((_bits(nv) != _bits(want)).any(1))[0]
    assert (_bits(nv) != _bits(p1)).any(), "no user plane changed any row"
    none = [i for i in range(n) if len(user[i]) == 0]
    assert np.array_equal(_bits(nv[none]), _bits(p1[none]))
    ctx.set_user_planes(None)
    assert np.array_equal(_bits(_step(lqro_mod, ctx, x, vg)), _bits(p2))   # a fresh context's second step
    ctx.close()


# 2 ------------------------------------------------------------------------
def test_fence(lqro_mod, oracle, gains, swarm):
    x, vg, user = swarm
    n = x.shape[0]
    m = np.array([0.26, 0.26, 0.75])
    inf = np.inf
    lo, hi = box_for(x)
    p = x[:, :3]
    outside = ((p < lo) | (p > hi)).any(1)
    near = ~outside & ((p - lo < m) | (hi - p < m)).any(1)
    assert outside.sum() == 2 and near.sum() >= 1 and (~outside & ~near).sum() >= 1
    ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "qhull"))
    # a floor alone
    flo, fhi = np.array([-inf, -inf, -1.0]), np.array([inf, inf, inf])
    ctx.set_fence(flo, fhi, 2.0)
    nv = _step(lqro_mod, ctx, x, vg)
    f = fence_planes(x, flo, fhi, 2.0)
    assert f.shape == (n, 1, 6)
    want = expected_newv(oracle, ctx.records(), range(n), vg, fence=f)
    assert np.array_equal(_bits(nv), _bits(want))
    # the whole box
    ctx.set_fence(lo, hi, 2.0)
    nv = _step(lqro_mod, ctx, x, vg)
    f = fence_planes(x, lo, hi, 2.0)
    assert f.shape == (n, 6, 6)
    recs = ctx.records()
    want = expected_newv(oracle, recs, range(n), vg, fence=f)
    assert np.array_equal(_bits(nv), _bits(want))
    free = expected_newv(oracle, recs, range(n), vg)
    assert (_bits(want) != _bits(free)).any(1).sum() >= 2, "the box changed fewer than two rows"
    # fence, then user planes, then the pairs: the stated order, and no other
    ctx.set_user_planes(user)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    want = expected_newv(oracle, recs, range(n), vg, fence=f, user=user)
    swapped = expected_newv(oracle, recs, range(n), vg, fence=f, user=user, user_first=True)
    assert (_bits(want) != _bits(swapped)).any(), "the order of fence and user planes shows in no row"
    assert np.array_equal(_bits(nv), _bits(want))
    # off again
    ctx.set_fence(None, None, 0.0)
    ctx.set_user_planes(None)
    nv = _step(lqro_mod, ctx, x, vg)
    assert np.array_equal(_bits(nv), _bits(expected_newv(oracle, ctx.records(), range(n), vg)))
    # a box narrower than the ellipsoid, bad plane counts
    L = lqro_mod.lib()
    bad_lo, bad_hi = np.array([0.0, 0.0, 0.0]), np.array([0.5, 5.0, 5.0])
    assert L.lqro_set_fence(ctx._h, bad_lo.ctypes.data, bad_hi.ctypes.data, 2.0) == -1
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = 8193
    big = np.zeros((8193, 6), np.float32)
    assert L.lqro_set_user_planes(ctx._h, big.ctypes.data, offs.ctypes.data) == -1
    offs[1:] = np.arange(n)[::-1]
    assert L.lqro_set_user_planes(ctx._h, big.ctypes.data, offs.ctypes.data) == -1
    assert L.lqro_set_user_planes_device(ctx._h, big.ctypes.data, 8193, None) == -1
    ctx.close()


# 3 ------------------------------------------------------------------------
LONG_SEED = 3


def long_user_planes(total, x, seed=LONG_SEED):
    """Agent 0: total - 5 planes in the manner of lp_cases.long_row (far
    feasible planes, then a 129-plane parallel family); agents 1-5: 0 to 3."""
    c, _ = lp_cases.long_row(total - 5, seed)
    rng = np.random.default_rng([seed, total])
    out = [c.astype(np.float32)]
    for i in range(1, x.shape[0]):
        p = lp_cases._FAMILY_FN["parallel"](rng, (i - 1) % 4, i).astype(np.float32).reshape(-1, 6)
        p[:, :3] += x[i, 3:6].astype(np.float32)
        out.append(p)
    return out


@pytest.mark.parametrize("total", lp_cases.LONG_SIZES)
def test_layout_borders(lqro_mod, oracle, gains, total):
    """5 + U planes on agent 0's row: the last row of each launch_lp layout
    and the first of the next, with linearProgram4 running under each;
    through lqro_set_user_planes_device from a torch tensor, live counts
    below the pitch and NaN in the unused slots."""
    n, h, npts = 6, 20, 50
    x, vg = lqro_mod.synthetic_swarm(n, box=2.0, seed=3)
    user = long_user_planes(total, x)
    U = total - 5
    assert len(user[0]) == U and [len(u) for u in user[1:]] == [0, 1, 2, 3, 0]
    flat = np.full((n, U, 6), np.nan, np.float32)
    for i, u in enumerate(user):
        flat[i, :len(u)] = u
    counts = np.array([len(u) for u in user], np.int32)
    d_planes = torch.from_numpy(flat).cuda()
    d_counts = torch.from_numpy(counts).cuda()
    torch.cuda.synchronize()
    ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "qhull"), h=h, npts=npts)
    ctx.set_user_planes_device(d_planes.data_ptr(), U, d_counts.data_ptr())
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    row0 = np.concatenate([user[0], pair_planes(recs, n)[0]])
    assert oracle.lp_chain(row0, vg[0], 100.0) > 0, "linearProgram4 does not run on agent 0's row"
    want = expected_newv(oracle, recs, range(n), vg, user=user)
    assert np.array_equal(_bits(nv), _bits(want)), (total, nv, want)
    # no counts: every slot is live (each agent's own planes repeated to the
    # pitch; the agents that have none take agent 0's)
    full = np.stack([np.resize(u if len(u) else user[0], (U, 6)) for u in user])
    d_full = torch.from_numpy(full).cuda()
    torch.cuda.synchronize()
    ctx.set_user_planes_device(d_full.data_ptr(), U, 0)
    nv = _step(lqro_mod, ctx, x, vg)
    want = expected_newv(oracle, ctx.records(), range(n), vg, user=list(full))
    assert np.array_equal(_bits(nv), _bits(want))
    ctx.set_user_planes_device(0, 0, 0)
    nv = _step(lqro_mod, ctx, x, vg)
    assert np.array_equal(_bits(nv), _bits(expected_newv(oracle, ctx.records(), range(n), vg)))
    ctx.close()


# 4 ------------------------------------------------------------------------
HOT = dict(n=257, box=14.0, seed=7, H=50, NP=50, steps=4)
HOT_LO, HOT_HI, HOT_TAU = (-6.0, -6.0, -6.5), (6.0, 6.0, 6.5), 2.0


def hot_user_planes(x):
    """Two planes per agent: keep 0.5 m/s around a direction of the agent's own."""
    rng = np.random.default_rng(17)
    nrm = rng.normal(size=(x.shape[0], 2, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    pts = x[:, None, 3:6] - 0.5 * nrm
    return np.concatenate([pts, nrm], 2).astype(np.float32)


HOT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import lqro
a = np.load(sys.argv[2])
x, vg = a["x"], a["vg"]
g = lqro.synthesize_gains()
c = lqro.Context(lqro.config(x.shape[0], int(a["H"]), int(a["NP"]),
                             flags=lqro.LQRO_FLAG_RECORDS | lqro.LQRO_FLAG_QHULL_ORDER))
c.set_gains(g["A"], g["B"], g["L"], g["E"])
c.set_fence(a["lo"], a["hi"], float(a["tau"]))
c.set_user_planes(list(a["user"]))
nv, recs = [], []
for t in range(int(a["steps"])):
    try:
        nv.append(c.step(x, vg))
    except lqro.QhullMergeSuspect as e:
        nv.append(e.newv)
    recs.append(c.records())
np.savez(sys.argv[3], nv=np.stack(nv), recs=np.stack(recs))
"""


@pytest.fixture(scope="module")
def hot_swarm(lqro_mod):
    x, vg = lqro_mod.synthetic_swarm(HOT["n"], box=HOT["box"], seed=HOT["seed"])
    return x, vg, hot_user_planes(x)


def _hot_expected(oracle, hot_swarm, recs):
    x, vg, user = hot_swarm
    f = fence_planes(x, np.array(HOT_LO), np.array(HOT_HI), HOT_TAU)
    return expected_newv(oracle, recs, range(x.shape[0]), vg, fence=f, user=user)


@pytest.mark.parametrize("split", [False, True])
def test_early_lp_sees_the_extras(lqro_mod, oracle, gains, hot_swarm, split):
    """257 x 256 slots: the hot schedule with the early LP from the third
    step.  lqro_step_device, and lqro_step_device_begin / _end on one context
    owning every row (the early rows run in _begin)."""
    x, vg, user = hot_swarm
    n = x.shape[0]
    ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "qhull"), h=HOT["H"], npts=HOT["NP"])
    ctx.set_fence(HOT_LO, HOT_HI, HOT_TAU)
    ctx.set_user_planes(list(user))
    d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
    d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_tab = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sid = torch.cuda.current_stream().cuda_stream
    for t in range(HOT["steps"]):
        d_nv.zero_()
        if split:
            ctx.step_device_begin(d_x.data_ptr(), d_vg.data_ptr(), d_tab.data_ptr(), sid)
            if t == 0:   # the pending half-step's LP still reads the planes: LQRO_E_STATE
                L = lqro_mod.lib()
                assert L.lqro_set_fence(ctx._h, None, None, 0.0) == -4
                assert L.lqro_set_user_planes(ctx._h, None, None) == -4
                assert L.lqro_set_user_planes_device(ctx._h, None, 0, None) == -4
            ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
        else:
            ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
        torch.cuda.synchronize()
        recs = ctx.records()
        if t == 2:
            assert ctx.stats()["inside"] > 0
        want = _hot_expected(oracle, hot_swarm, recs)
        got = d_nv.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (t, np.nonzero((_bits(got) != _bits(want)).any(1))[0])
    ctx.close()


def test_early_lp_off_sees_the_extras(lqro_mod, oracle, hot_swarm, tmp_path):
    """The same four steps with LQRO_EARLY_LP=0 (read from the environment
    when the context is created: a child process)."""
    x, vg, user = hot_swarm
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "hot.npz")
    np.savez(inp, x=x, vg=vg, user=user, lo=HOT_LO, hi=HOT_HI, tau=HOT_TAU, H=HOT["H"], NP=HOT["NP"],
             steps=HOT["steps"])
    env = dict(os.environ, LQRO_EARLY_LP="0")
    r = subprocess.run([sys.executable, "-c", HOT_CHILD, PKG, inp, out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    for t in range(HOT["steps"]):
        want = _hot_expected(oracle, hot_swarm, d["recs"][t])
        assert np.array_equal(_bits(d["nv"][t]), _bits(want)), t


# 5 ------------------------------------------------------------------------
def test_culling_with_extras(lqro_mod, oracle, gains, swarm):
    x, vg, user = swarm
    n, K = x.shape[0], 4
    lo, hi = box_for(x)
    ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "qhull"))
    ctx.set_neighbors(6.0, K)
    ctx.set_fence(lo, hi, 2.0)
    ctx.set_user_planes(user)
    nv = _step(lqro_mod, ctx, x, vg)
    recs = ctx.records()
    assert len(recs) == n * K
    want = expected_newv(oracle, recs, range(n), vg, fence=fence_planes(x, lo, hi, 2.0), user=user)
    assert np.array_equal(_bits(nv), _bits(want))
    ctx.close()


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["block", "cyclic"])
@pytest.mark.parametrize("world", [2, 3])
def test_shards_read_the_global_arrays(lqro_mod, gains, swarm, world, mode):
    x, vg, user = swarm
    n = x.shape[0]
    lo, hi = box_for(x)

    def run(**kw):
        ctx = _ctx(lqro_mod, gains, n, _flags(lqro_mod, "canonical"), **kw)
        ctx.set_fence(lo, hi, 2.0)
        ctx.set_user_planes(user)
        nv = ctx.step(x, vg)
        ids = ctx.row_ids
        ctx.close()
        return nv, ids

    full, _ = run()
    seen = []
    for r in range(world):
        nv, ids = run(**lqro_mod.shard_rows(n, r, world, mode))
        assert np.array_equal(ids, lqro_mod.shard_row_ids(n, r, world, mode))
        assert np.array_equal(_bits(nv[ids]), _bits(full[ids])), (r, mode)
        seen.extend(ids)
    assert sorted(seen) == list(range(n))


# 7 ------------------------------------------------------------------------
def _context_two_steps(lqro_mod, gains, x, vg, lo, hi, user):
    ctx = _ctx(lqro_mod, gains, x.shape[0], _flags(lqro_mod, "qhull", records=False))
    ctx.set_fence(lo, hi, 2.0)
    if user is not None:
        ctx.set_user_planes(user)
    out = [_step(lqro_mod, ctx, x, vg) for _ in range(2)]
    ctx.close()
    return out


def test_python_hosts_pass_them_through(lqro_mod, gains, swarm):
    x, vg, user = swarm
    n = x.shape[0]
    lo, hi = box_for(x)
    want = _context_two_steps(lqro_mod, gains, x, vg, lo, hi, None)
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x[i], vGoal=vg[i]) for i in range(n)], horizon=H, n_points=NP,
                             fence=(lo, hi, 2.0))
    sim.findMatrices()
    for t in range(2):
        try:
            sim.step()
        except lqro_mod.QhullMergeSuspect:
            pass                             # (newV is stored before the raise)
        got = np.stack([q.newV for q in sim.qlist])
        assert np.array_equal(_bits(got), _bits(want[t])), t
    sim.ctx.close()
    want = _context_two_steps(lqro_mod, gains, x, vg, lo, hi, user)
    g = dict(gains, l=np.zeros(4))
    loop = lqro_mod.DeviceLoop(x, vg, g, H, NP, fence=(lo, hi, 2.0), user_planes=user)
    for t in range(2):
        nv = loop.step()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(nv.cpu().numpy()), _bits(want[t])), t
    loop.close()


def test_cpp_host_passes_them_through(lqro_mod, gains, swarm, tmp_path):
    from test_user_planes_cpu import build_fence_main, write_fence_input
    x, vg, user = swarm
    n = x.shape[0]
    lo, hi = box_for(x)
    want = _context_two_steps(lqro_mod, gains, x, vg, lo, hi, user)
    exe = build_fence_main(tmp_path)
    write_fence_input(tmp_path / "in.bin", x, vg, H, NP, 2, lo, hi, 2.0, user)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    # (a merge-suspect step ends the program with status 1 after storing newV; this swarm has none)
    assert r.returncode == 0, r.stderr
    got = np.zeros((2, n, 3))
    for line in r.stdout.splitlines():
        t, i, a, b, c = line.split()
        got[int(t), int(i)] = [float.fromhex(a), float.fromhex(b), float.fromhex(c)]
    for t in range(2):
        assert np.array_equal(_bits(got[t]), _bits(want[t])), t


RAISE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import lqro
lqro.LIB_PATH = sys.argv[2]
x, vg = lqro.synthetic_swarm(24, box=3.0, seed=11)
sim = lqro.Simulator([lqro.Quadrotor(x[i], vGoal=vg[i]) for i in range(24)], horizon=45)
sim.findMatrices()
try:
    sim.step()
    print("no raise")
except lqro.HullFailure as e:
    got = np.stack([q.newV for q in sim.qlist])
    print("stored" if np.array_equal(got, e.newv) and e.newv.any() else "not stored")
"""


def test_simulator_stores_newv_of_a_raising_step(lqro_mod):
    """A step that raises (here LQRO_E_HULL from the tiny-cap library of
    tests/test_gpu_hull_caps.py) has written newV: Simulator.step stores it
    in qlist before re-raising."""
    lib = os.path.join(PKG, "liblqro_tinycap.so")
    assert os.path.exists(lib), "liblqro_tinycap.so not built (__graft_entry__.build)"
    r = subprocess.run([sys.executable, "-c", RAISE_CHILD, PKG, lib], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "stored", r.stdout
