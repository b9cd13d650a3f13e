"""Obstacles as extra columns of the pair loop (lqro_set_obstacles,
lqro_set_obstacles_device), bit for bit against the oracle as it stands.

`pyoracle.step(..., rows=(0, N))` over an (N + M)-body array is the pair loop
the feature asks for: rows 0..N-1 sweep the columns 0..N+M-1.  With obstacle
radii equal to the agents' and responsibility 0.5 an obstacle column IS an
agent column, and the whole step (records, LP, carried normal) is the
oracle's.  With another shape or responsibility the pair-local fields come
from two oracle steps (the agents' sphere S for the agent columns, the
obstacles' sphere S_o for the obstacle columns) and the three fields that
depend on the factor of LQRO:1416 and on the loop-carried normal are redone
in (i, j) order by `walk` below:

    for every record with REC_PLANE and without HULLFAIL:
        n = carry if REC_STALE else rec.normal;  carry = n
        d = rec.dist * (responsibility if j >= N else 0.5)
        mult = +1 if REC_INSIDE else -1
        point[k] = float32(x[i, 3 + k] + mult * d * n[k]);  plane_normal = float32(n)

and each row's newV is the oracle's LP (pyoracle.newv) over the walked planes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before liblqro.so is loaded: the process then runs on the one HIP runtime torch brings

from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "lqr-obstacles_amd")
RULES = ("qhull", "canonical")
H, NP = 50, 100
N, M = 24, 4
RXY, RZ = 0.26, 0.75            # the agents' radii (lqro_config_default)
PAIR_LOCAL = ("i", "j", "n_reach", "reach_hash", "flags", "gjk_iters", "simplex_n", "simplex", "dist", "wpt_vrel",
              "wpt_hull", "facet", "n_facets")
WALKED = ("normal", "plane_point", "plane_normal")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _flags(lqro, rule):
    return lqro.LQRO_FLAG_RECORDS | (lqro.LQRO_FLAG_QHULL_ORDER if rule == "qhull" else 0)


def obstacle_swarm(lqro, n, m, seed, box=3.0, x_dim=16):
    """synthetic_swarm(n + m): rows n.. are the obstacles, at rest except the
    last, which keeps its velocity (a moving obstacle)."""
    x_all, vg = lqro.synthetic_swarm(n + m, box=box, seed=seed, x_dim=x_dim)
    x_all[n:n + m - 1, 3:6] = 0.0
    return x_all, vg


def _ctx(lqro, gains, n, rule, h=H, npts=NP, **kw):
    c = lqro.Context(lqro.config(n, h, npts, flags=_flags(lqro, rule), **kw))
    c.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    return c


def _step(lqro, ctx, x, vg):
    try:
        return ctx.step(x, vg)
    except lqro.QhullMergeSuspect as e:   # (the step completed; the records say which pair)
        return e.newv


class Oracle:
    """The oracle's steps over the (n + m) bodies, rows (0, n)."""

    def __init__(self, oracle, gains, h=H, npts=NP, tabs=None, per_agent=False, threads=1):
        self.o, self.npts, self.per_agent, self.threads = oracle, npts, per_agent, threads
        self.T, self.NCF = tabs if tabs is not None else oracle.tables(gains["A"], gains["B"], gains["L"], gains["E"], h)
        self.S = oracle.sphere(npts)

    def steps(self, x_all, vg, n, rule, steps=1, S=None, carry=None):
        """[(newV rows [0, n), records (n, n + m - 1), carry out)] of `steps`
        consecutive steps, the first entered with `carry` (default 0)."""
        o = self.o
        out = []
        o.set_hull_rule(1 if rule == "qhull" else 0, round16=True)
        o.carry_normal(np.zeros(3) if carry is None else carry)
        try:
            for _ in range(steps):
                nv, recs = o.step(self.T, self.NCF, self.S if S is None else S, x_all, vg, rows=(0, n),
                                  per_agent=self.per_agent, threads=self.threads)
                out.append((nv[:n], recs.reshape(n, -1), o.carry_normal()))
        finally:
            o.set_hull_rule(0)
        return out

    def obstacle_sphere(self, oxy, oz):
        """S_o: createSpheres over the summed radii (lqro.h), asserted equal to
        the header's formula bit for bit."""
        So = self.o.sphere(self.npts, (RXY + oxy) / 2, (RZ + oz) / 2)
        dlong, dz = np.pi * (3.0 - np.sqrt(5.0)), 2.0 / self.npts
        lon, z = 0.0, 1.0 - dz / 2.0
        want = np.zeros((self.npts, 3))
        for p in range(self.npts):
            want[p] = [(RXY + oxy) * np.cos(lon) * np.sqrt(1 - z * z), (RXY + oxy) * np.sin(lon) * np.sqrt(1 - z * z),
                       (RZ + oz) * z]
            z -= dz
            lon += dlong
        assert np.array_equal(_bits(So), _bits(want))
        return So

    def pair_local(self, x_all, vg, n, rule, oxy, oz):
        """Records (n, n + m - 1) whose agent columns come from the step with S
        and whose obstacle columns from the step with S_o; the walked fields
        are not yet valid."""
        ra = self.steps(x_all, vg, n, rule)[0][1]
        ro = self.steps(x_all, vg, n, rule, S=self.obstacle_sphere(oxy, oz))[0][1]
        exp = ra.copy()
        exp[:, n - 1:] = ro[:, n - 1:]
        return exp


def walk(lqro, oracle, local, x_all, vg, n, resp, carry, head=None, rows=None):
    """The module docstring's walk over `local` (rows x slots, in (i, j)
    order): (records with the walked fields, newV per row, carry out).
    head[i]: planes ahead of row i's pair planes."""
    exp = local.copy()
    carry = np.array(carry, np.float64)
    rows = range(n) if rows is None else rows
    nv = np.zeros((len(rows), 3))
    for r, i in enumerate(rows):
        planes = [] if head is None else [np.asarray(head[i], np.float32).reshape(-1, 6)]
        for q in range(exp.shape[1]):
            rec = exp[r, q]
            fl = int(rec["flags"])
            if not (fl & lqro.REC_PLANE) or (fl & lqro.REC_HULLFAIL):
                continue
            nrm = carry.copy() if fl & lqro.REC_STALE else rec["normal"].copy()
            carry = nrm
            d = rec["dist"] * (resp if rec["j"] >= n else 0.5)
            mult = 1.0 if fl & lqro.REC_INSIDE else -1.0
            pt = np.array([x_all[i, 3 + k] + mult * d * nrm[k] for k in range(3)]).astype(np.float32)
            exp[r, q]["normal"] = nrm
            exp[r, q]["plane_point"] = pt
            exp[r, q]["plane_normal"] = nrm.astype(np.float32)
            planes.append(np.concatenate([pt, nrm.astype(np.float32)])[None])
        nv[r] = oracle.newv(np.concatenate(planes) if planes else np.zeros((0, 6), np.float32), vg[i], 100.0)
    return exp, nv, carry


def assert_records(lqro, got, want, fields=PAIR_LOCAL + WALKED, what=""):
    got, want = got.reshape(want.shape), want
    for f in fields:
        a, b = got[f], want[f]
        if f == "flags":
            a = a & ~lqro.REC_LOCAL   # the oracle has no local hull
        if f == "n_facets":           # (... whose count is of the facets it certified: lqro.h)
            a = np.where((got["flags"] & lqro.REC_LOCAL) != 0, b, a)
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, f, [(int(want["i"][k[0], k[1]]), int(want["j"][k[0], k[1]])) for k in bad[:5]])


def counts(lqro, recs, n):
    """(obstacle planes, obstacle inside-hull pairs, stale obstacle pairs, stale agent pairs)."""
    ob = recs["j"] >= n
    fl = recs["flags"]
    return (int(((fl & lqro.REC_PLANE) != 0)[ob].sum()), int(((fl & lqro.REC_INSIDE) != 0)[ob].sum()),
            int(((fl & lqro.REC_STALE) != 0)[ob].sum()), int(((fl & lqro.REC_STALE) != 0)[~ob].sum()))


@pytest.fixture(scope="module")
def orc(oracle, gains):
    return Oracle(oracle, gains)


_LOCAL = {}


def local_for(orc, lqro, seed, rule, radii, n=N, m=M):
    """The pair-local expectation of obstacle_swarm(n, m, seed), computed once."""
    key = (seed, rule, radii, n, m)
    if key not in _LOCAL:
        x_all, vg = obstacle_swarm(lqro, n, m, seed)
        _LOCAL[key] = (x_all, vg, orc.pair_local(x_all, vg, n, rule, *radii))
    return _LOCAL[key]


_EQUAL = {}


def equal_for(orc, lqro, seed, rule):
    """Two consecutive oracle steps of the all-agents (N + M) loop, once."""
    key = (seed, rule)
    if key not in _EQUAL:
        x_all, vg = obstacle_swarm(lqro, N, M, seed)
        _EQUAL[key] = (x_all, vg, orc.steps(x_all, vg, N, rule, steps=2))
    return _EQUAL[key]


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("rule", RULES)
def test_equals_an_all_agents_step(lqro_mod, orc, gains, rule, seed):
    """Obstacle radii = the agents', responsibility 0.5: records, newV and
    the carried normal are pyoracle.step's over the (N + M) bodies, rows
    (0, N), over two steps (the second enters with the first's carry)."""
    x_all, vg, ref = equal_for(orc, lqro_mod, seed, rule)
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_obstacles(x_all[N:], responsibility=0.5)
    ctx.carry_normal(np.zeros(3))
    for t, (nv_o, recs_o, carry_o) in enumerate(ref):
        nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
        recs = ctx.records()
        assert len(recs) == N * (N - 1 + M)
        assert_records(lqro_mod, recs, recs_o, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_o)), t
        if rule == "qhull":
            assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_o)), t
        assert ctx.stats()["pairs"] == N * (N - 1 + M)
    planes, inside, stale_obs, stale_ag = counts(lqro_mod, ref[0][1], N)
    assert planes > 0 and inside > 0, (planes, inside)
    if rule == "qhull":   # (the swarm exercises the carried normal on both kinds of column)
        assert (stale_ag if seed == 11 else stale_obs) > 0, (seed, stale_obs, stale_ag)
    ctx.close()


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("radii", [(0.0, 0.0), (0.5, 0.25), (1.0, 1.0)])
@pytest.mark.parametrize("rule", RULES)
def test_responsibility_and_shape(lqro_mod, oracle, orc, gains, rule, radii):
    x_all, vg, local = local_for(orc, lqro_mod, 11, rule, radii)
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_obstacles(x_all[N:], radii[0], radii[1], responsibility=1.0)
    ctx.carry_normal(np.zeros(3))
    carry = np.zeros(3)
    for t in range(2):
        want, nv_w, carry = walk(lqro_mod, oracle, local, x_all, vg, N, 1.0, carry)
        nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
        assert_records(lqro_mod, ctx.records(), want, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_w)), (t, np.nonzero((_bits(nv) != _bits(nv_w)).any(1))[0])
        if rule == "qhull":
            assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
        if t == 0:
            first = nv_w
    ctx.close()
    planes, inside, stale_obs, _ = counts(lqro_mod, local, N)
    assert planes > 0 and inside > 0
    equal = equal_for(orc, lqro_mod, 11, rule)[2][0][0]
    assert (_bits(first) != _bits(equal)).any(1).sum() >= 1, "no row's newV differs from the all-agents step"
    if rule == "qhull" and radii == (1.0, 1.0):
        assert stale_obs >= 1, "no stale obstacle pair"


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_columns_that_emit_nothing(lqro_mod, gains, rule):
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    x, vgn = x_all[:N], vg[:N]
    far = x_all[N:].copy()
    far[:, 0] += 1000.0
    plain = _ctx(lqro_mod, gains, N, rule)
    p = []
    for t in range(3):
        nv = _step(lqro_mod, plain, x, vgn)
        p.append((nv, plain.records().reshape(N, N - 1), plain.carry_normal()))
    plain.close()
    ctx = _ctx(lqro_mod, gains, N, rule)
    ctx.set_obstacles(far, 0.5, 0.25)
    for t in range(2):
        nv = _step(lqro_mod, ctx, x, vgn)
        recs = ctx.records().reshape(N, N - 1 + M)
        assert np.array_equal(recs["j"][:, N - 1:], np.tile(np.arange(N, N + M), (N, 1)))
        assert not (recs["flags"][:, N - 1:] & lqro_mod.REC_PLANE).any()
        assert recs[:, :N - 1].tobytes() == p[t][1].tobytes(), t
        assert np.array_equal(_bits(nv), _bits(p[t][0])), t
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(p[t][2])), t
    ctx.set_obstacles(None)
    nv = _step(lqro_mod, ctx, x, vgn)
    recs = ctx.records()
    assert len(recs) == N * (N - 1) and recs.reshape(N, N - 1).tobytes() == p[2][1].tobytes()
    assert np.array_equal(_bits(nv), _bits(p[2][0]))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(p[2][2]))
    ctx.close()


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 40, 41, 42])
def test_chunk_borders(lqro_mod, oracle, orc, gains, m):
    """24, 63, 64 and 65 slots a row: the LP's and the ballots' 64-wide chunks."""
    assert N - 1 + m in (24, 63, 64, 65)
    radii = (0.5, 0.25)
    x_all, vg, local = local_for(orc, lqro_mod, 11, "qhull", radii, m=m)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_obstacles(x_all[N:], *radii)
    want, nv_w, carry = walk(lqro_mod, oracle, local, x_all, vg, N, 1.0, np.zeros(3))
    nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert_records(lqro_mod, ctx.records(), want)
    assert np.array_equal(_bits(nv), _bits(nv_w))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry))
    assert counts(lqro_mod, local, N)[0] > 0
    ctx.close()


# 5 ------------------------------------------------------------------------
HOT = dict(n=257, m=8, box=14.0, seed=7, H=50, NP=50, steps=4)
HOT_RADII = (1.0, 1.0)
HOT_LO, HOT_HI, HOT_TAU = (-6.0, -6.0, -6.5), (6.0, 6.0, 6.5), 2.0


def hot_obstacles(lqro, x_all, which):
    """The 8 obstacle states of the hot swarm's two halves.  synthetic_swarm(265)
    scatters its last 8 bodies through a 14 m box, where none comes inside an
    agent's LQR-obstacle: the obstacles are moved onto agents' paths instead —
    obstacle o sits 0.6 m (first half: steps 0-1) or 0.9 m (second half: steps
    2-3) ahead of agent 16 o + 3 along its velocity, at rest except the last,
    which keeps the velocity synthetic_swarm drew for it."""
    n, m = HOT["n"], HOT["m"]
    obs = x_all[n:].copy()
    for o in range(m):
        a = x_all[16 * o + 3]
        v = a[3:6] / np.linalg.norm(a[3:6])
        obs[o, 0:3] = a[0:3] + (0.6 if which == 0 else 0.9) * v
    return obs


@pytest.fixture(scope="module")
def hot(lqro_mod, oracle, gains):
    """The 257-agent hot swarm of tests/test_gpu_user_planes.py (its
    construction: synthetic_swarm is a prefix of the 265-body draw) with 8
    obstacles; the pair-local expectation of both halves."""
    n, m = HOT["n"], HOT["m"]
    x_all, vg = obstacle_swarm(lqro_mod, n, m, HOT["seed"], box=HOT["box"])
    x257, _ = lqro_mod.synthetic_swarm(n, box=HOT["box"], seed=HOT["seed"])
    assert np.array_equal(x_all[:n], x257)
    orc = Oracle(oracle, gains, h=HOT["H"], npts=HOT["NP"], threads=8)   # (67,848 pairs a step)
    halves = []
    for which in (0, 1):
        xa = x_all.copy()
        xa[n:] = hot_obstacles(lqro_mod, x_all, which)
        halves.append((xa, orc.pair_local(xa, vg, n, "qhull", *HOT_RADII)))
    assert all(counts(lqro_mod, loc, n)[1] >= 1 for _, loc in halves), "no obstacle inside-hull pair"
    return x_all, vg, halves


def hot_expected(lqro, oracle, hot, head=None):
    """Per step (records, newV, carry out) of the four hot steps."""
    _, vg, halves = hot
    carry = np.zeros(3)
    out = []
    for t in range(HOT["steps"]):
        xa, local = halves[t // 2]
        want, nv, carry = walk(lqro, oracle, local, xa, vg, HOT["n"], 1.0, carry, head=head)
        out.append((want, nv, carry))
    return out


@pytest.fixture(scope="module")
def hot_want(lqro_mod, oracle, hot):
    return hot_expected(lqro_mod, oracle, hot)


@pytest.mark.parametrize("hot_split", ["1", "0"])
@pytest.mark.parametrize("halves", [False, True], ids=["step_device", "begin_end"])
def test_device_path_and_schedules(lqro_mod, gains, hot, hot_want, monkeypatch, halves, hot_split):
    """257 x 264 slots: the hot schedule from the third step.  The obstacle
    states are a torch tensor rewritten between the second and the third step
    (lqro_set_obstacles_device reads it when the step runs)."""
    monkeypatch.setenv("LQRO_HOT_SPLIT", hot_split)
    x_all, vg, hv = hot
    n = HOT["n"]
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=HOT["H"], npts=HOT["NP"])
    d_obs = torch.from_numpy(hv[0][0][n:].copy()).cuda()
    ctx.set_obstacles(d_obs, *HOT_RADII)
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
                L = lqro_mod.lib()
                assert L.lqro_set_obstacles(ctx._h, None, 0, 0.0, 0.0, 1.0) == -4
                assert L.lqro_set_obstacles_device(ctx._h, d_obs.data_ptr(), 8, 1.0, 1.0, 1.0) == -4
            ctx.step_device_end(d_tab.data_ptr(), d_nv.data_ptr(), sid)
        else:
            ctx.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
        torch.cuda.synchronize()
        want, nv_w, carry = hot_want[t]
        assert_records(lqro_mod, ctx.records(), want, what=(t,))
        got = d_nv.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(nv_w)), (t, np.nonzero((_bits(got) != _bits(nv_w)).any(1))[0])
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
    ctx.close()


HOT_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import lqro
a = np.load(sys.argv[2])
x, vg = a["x"], a["vg"]
n = x.shape[0]
g = lqro.synthesize_gains()
c = lqro.Context(lqro.config(n, int(a["H"]), int(a["NP"]), flags=lqro.LQRO_FLAG_RECORDS | lqro.LQRO_FLAG_QHULL_ORDER))
c.set_gains(g["A"], g["B"], g["L"], g["E"])
d_obs = torch.from_numpy(a["obs0"]).cuda()
c.set_obstacles(d_obs, float(a["oxy"]), float(a["oz"]))
d_x, d_vg = torch.from_numpy(x).cuda(), torch.from_numpy(vg).cuda()
d_nv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
sid = torch.cuda.current_stream().cuda_stream
nv, recs = [], []
for t in range(int(a["steps"])):
    if t == 2:
        d_obs.copy_(torch.from_numpy(a["obs1"]))
    c.step_device(d_x.data_ptr(), d_vg.data_ptr(), d_nv.data_ptr(), sid)
    torch.cuda.synchronize()
    nv.append(d_nv.cpu().numpy())
    recs.append(c.records())
np.savez(sys.argv[3], nv=np.stack(nv), recs=np.stack(recs))
"""


def test_device_path_early_lp_off(lqro_mod, hot, hot_want, tmp_path):
    """The same four steps with LQRO_EARLY_LP=0, in a child process."""
    x_all, vg, hv = hot
    n = HOT["n"]
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "hot.npz")
    np.savez(inp, x=x_all[:n], vg=vg[:n], obs0=hv[0][0][n:], obs1=hv[1][0][n:], oxy=HOT_RADII[0], oz=HOT_RADII[1],
             H=HOT["H"], NP=HOT["NP"], steps=HOT["steps"])
    env = dict(os.environ, LQRO_EARLY_LP="0")
    r = subprocess.run([sys.executable, "-c", HOT_CHILD, PKG, inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    for t in range(HOT["steps"]):
        want, nv_w, _ = hot_want[t]
        assert_records(lqro_mod, d["recs"][t], want, what=(t,))
        assert np.array_equal(_bits(d["nv"][t]), _bits(nv_w)), t


def test_order_fence_user_agents_obstacles(lqro_mod, oracle, gains, hot):
    """A 6-face fence and two user planes per agent with the obstacles: the
    row's LP sees fence, user, agent and obstacle planes in that order."""
    from test_gpu_user_planes import fence_planes, hot_user_planes
    x_all, vg, hv = hot
    n = HOT["n"]
    x = x_all[:n]
    user = hot_user_planes(x)
    f = fence_planes(x, np.array(HOT_LO), np.array(HOT_HI), HOT_TAU)
    head = [np.concatenate([f[i], user[i]]) for i in range(n)]
    ctx = _ctx(lqro_mod, gains, n, "qhull", h=HOT["H"], npts=HOT["NP"])
    ctx.set_fence(HOT_LO, HOT_HI, HOT_TAU)
    ctx.set_user_planes(list(user))
    ctx.set_obstacles(hv[0][0][n:], *HOT_RADII)
    nv = _step(lqro_mod, ctx, x, vg[:n])
    want, nv_w, _ = walk(lqro_mod, oracle, hv[0][1], hv[0][0], vg, n, 1.0, np.zeros(3), head=head)
    assert_records(lqro_mod, ctx.records(), want)
    assert np.array_equal(_bits(nv), _bits(nv_w)), np.nonzero((_bits(nv) != _bits(nv_w)).any(1))[0]
    # no other order gives this: the obstacle planes first, per row
    differs = 0
    for i in range(n):
        row = want[i]
        k = (row["flags"] & lqro_mod.REC_PLANE) != 0
        if not (k & (row["j"] >= n)).any():
            continue
        pl = np.concatenate([row["plane_point"], row["plane_normal"]], 1).astype(np.float32)
        ob = row["j"] >= n
        other = np.concatenate([pl[k & ob], head[i], pl[k & ~ob]])
        differs += int((_bits(oracle.newv(other, vg[i], 100.0)) != _bits(nv_w[i])).any())
    assert differs >= 1, "the plane order shows in no row"
    ctx.close()


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["neighbors_first", "obstacles_first"])
@pytest.mark.parametrize("k", [2, 12])
def test_culling(lqro_mod, oracle, orc, gains, k, order):
    """Obstacles are candidates like agents: K = min(k, N + M - 1) slots a row,
    (d2, column) order; k = 2 is below the number of obstacles in range of some
    row, k = 12 above it for every row.  Equal radii, responsibility 0.5: the
    oracle's culled step over the (N + M) bodies."""
    dist = 2.0
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    d2 = ((x_all[:N, None, :3] - x_all[None, N:, :3]) ** 2).sum(2)
    in_range = (d2 < dist * dist).sum(1)
    assert in_range.max() > 2 and in_range.max() < 12, in_range
    oracle.set_neighbors(dist, k)
    try:
        nv_o, recs_o, carry_o = orc.steps(x_all, vg, N, "qhull")[0]
    finally:
        oracle.set_neighbors(0.0, 0)
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    if order == "neighbors_first":
        ctx.set_neighbors(dist, k)
        ctx.set_obstacles(x_all[N:], responsibility=0.5)
    else:
        ctx.set_obstacles(x_all[N:], responsibility=0.5)
        ctx.set_neighbors(dist, k)
    nv = _step(lqro_mod, ctx, x_all[:N], vg[:N])
    K = min(k, N + M - 1)
    recs = ctx.records().reshape(N, K)
    kept = kept_obs = 0
    for i in range(N):
        ref_row = recs_o[i][recs_o[i]["n_reach"] >= 0]
        c = len(ref_row)
        kept += c
        kept_obs += int((ref_row["j"] >= N).sum())
        assert c <= K and np.all(recs[i][c:]["n_reach"] == -1) and np.all(recs[i][c:]["j"] == -1)
        assert_records(lqro_mod, recs[i][:c][None], ref_row[None], what=(i,))
    assert kept_obs > 0 and ctx.stats()["pairs"] == kept
    assert np.array_equal(_bits(nv), _bits(nv_o))
    assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_o))
    ctx.close()


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize("radii", [None, (0.5, 0.25)], ids=["agents_shape", "own_shape"])
def test_per_agent_gains(lqro_mod, oracle, radii):
    """X = 12, N = 12, M = 3, per-agent gains: the row agent's own tables
    (and, with a shape of the obstacles' own, its own slice bound).  Equal
    radii and 0.5: the all-agents oracle step; (0.5, 0.25) and 1.0: the walk."""
    n, m, X, h = 12, 3, 12, 40
    models = lqro_mod.perturbed_models(n)
    g = lqro_mod.synthesize_gains_batch(models, x_dim=X)
    AB = lqro_mod.synthesize_gains(x_dim=X)
    x_all, vg = obstacle_swarm(lqro_mod, n, m, 11, box=2.5, x_dim=X)
    T, NCF = np.zeros((n + m, h, 9)), np.zeros((n + m, h, 3, X))
    for r in range(n):   # (the obstacles have no tables: a row's pair reads the row agent's)
        T[r], NCF[r] = oracle.tables(AB["A"], AB["B"], g["L"][r], g["E"][r], h, X=X)
    orc = Oracle(oracle, None, h=h, npts=NP, tabs=(T, NCF), per_agent=True)
    ctx = lqro_mod.Context(lqro_mod.config(n, h, NP, x_dim=X, flags=_flags(lqro_mod, "qhull")))
    ctx.set_gains(AB["A"], AB["B"], g["L"], g["E"], per_agent=True)
    if radii is None:
        ctx.set_obstacles(x_all[n:], responsibility=0.5)
        ref = orc.steps(x_all, vg, n, "qhull", steps=2)
    else:
        ctx.set_obstacles(x_all[n:], *radii)
        local = orc.pair_local(x_all, vg, n, "qhull", *radii)
        ref, carry = [], np.zeros(3)
        for t in range(2):
            want, nv_w, carry = walk(lqro_mod, oracle, local, x_all, vg, n, 1.0, carry)
            ref.append((nv_w, want, carry))
    for t, (nv_o, recs_o, carry_o) in enumerate(ref):
        nv = _step(lqro_mod, ctx, x_all[:n], vg[:n])
        assert_records(lqro_mod, ctx.records(), recs_o, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_o)), t
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry_o)), t
    assert counts(lqro_mod, ref[0][1], n)[0] > 0
    ctx.close()


def test_per_agent_gains_hot_launch(lqro_mod, oracle, hot):
    """Per-agent gains on the hot swarm (257 x 264 slots): from the third step
    the hot launch computes its pairs with the row agent's tables read in
    place (kHotPerAgent), the obstacle columns' slice bound among them."""
    x_all, vg, hv = hot
    n, m, h, npts = HOT["n"], HOT["m"], HOT["H"], HOT["NP"]
    xa = hv[0][0]
    g = lqro_mod.synthesize_gains_batch(lqro_mod.perturbed_models(n))
    AB = lqro_mod.synthesize_gains()
    T, NCF = np.zeros((n + m, h, 9)), np.zeros((n + m, h, 3, 16))
    for r in range(n):
        T[r], NCF[r] = oracle.tables(AB["A"], AB["B"], g["L"][r], g["E"][r], h)
    orc = Oracle(oracle, None, h=h, npts=npts, tabs=(T, NCF), per_agent=True, threads=8)
    local = orc.pair_local(xa, vg, n, "qhull", *HOT_RADII)
    assert counts(lqro_mod, local, n)[1] >= 1
    ctx = lqro_mod.Context(lqro_mod.config(n, h, npts, flags=_flags(lqro_mod, "qhull")))
    ctx.set_gains(AB["A"], AB["B"], g["L"], g["E"], per_agent=True)
    ctx.set_obstacles(xa[n:], *HOT_RADII)
    carry = np.zeros(3)
    for t in range(3):
        want, nv_w, carry = walk(lqro_mod, oracle, local, xa, vg, n, 1.0, carry)
        nv = _step(lqro_mod, ctx, xa[:n], vg[:n])
        assert_records(lqro_mod, ctx.records(), want, what=(t,))
        assert np.array_equal(_bits(nv), _bits(nv_w)), t
        assert np.array_equal(_bits(ctx.carry_normal()), _bits(carry)), t
    ctx.close()


# 8 ------------------------------------------------------------------------
@pytest.mark.parametrize("world,mode", [(2, "block"), (3, "block"), (2, "cyclic"), (3, "cyclic")])
def test_row_shards(lqro_mod, gains, world, mode):
    """Every shard takes the same obstacles; begin / the N x 4 row-normal
    table / end.  Every rank's records, newV and carried normal equal one
    context's over two steps (a row's last normal may be an obstacle column's)."""
    radii = (1.0, 1.0)
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    x, vgn = x_all[:N], vg[:N]
    one = _ctx(lqro_mod, gains, N, "qhull")
    one.set_obstacles(x_all[N:], *radii)
    ref = []
    for t in range(2):
        nv = _step(lqro_mod, one, x, vgn)
        ref.append((nv, one.records().reshape(N, N - 1 + M), one.carry_normal()))
    one.close()
    assert counts(lqro_mod, ref[0][1], N)[2] >= 1, "no stale obstacle pair"
    d_x, d_vg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(vgn.copy()).cuda()
    ctxs = []
    for g in range(world):
        c = _ctx(lqro_mod, gains, N, "qhull", **lqro_mod.shard_rows(N, g, world, mode))
        c.set_obstacles(x_all[N:], *radii)
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


# 9 ------------------------------------------------------------------------
def _context_two_steps(lqro_mod, gains, x_all, vg, radii, resp):
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    ctx.set_obstacles(x_all[N:], radii[0], radii[1], resp)
    out = [_step(lqro_mod, ctx, x_all[:N], vg[:N]) for _ in range(2)]
    ctx.close()
    return out


def test_python_hosts_pass_them_through(lqro_mod, gains):
    radii, resp = (0.5, 0.25), 0.75
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    want = _context_two_steps(lqro_mod, gains, x_all, vg, radii, resp)
    plain = _ctx(lqro_mod, gains, N, "qhull")
    assert (_bits(_step(lqro_mod, plain, x_all[:N], vg[:N])) != _bits(want[0])).any()
    plain.close()
    sim = lqro_mod.Simulator([lqro_mod.Quadrotor(x_all[i], vGoal=vg[i]) for i in range(N)], horizon=H, n_points=NP,
                             records=True)
    sim.findMatrices()
    sim.set_obstacles(lqro_mod.obstacle_states(x_all[N:, 0:3], x_all[N:, 3:6]), radii[0], radii[1], resp)
    for t in range(2):
        try:
            sim.step()
        except lqro_mod.QhullMergeSuspect:
            pass                             # (newV is stored before the raise)
        got = np.stack([q.newV for q in sim.qlist])
        assert np.array_equal(_bits(got), _bits(want[t])), t
    sim.ctx.close()
    g = dict(gains, l=np.zeros(4))
    loop = lqro_mod.DeviceLoop(x_all[:N], vg[:N], g, H, NP, flags=_flags(lqro_mod, "qhull"),
                               obstacles=(torch.from_numpy(x_all[N:].copy()).cuda(), radii[0], radii[1], resp))
    for t in range(2):
        nv = loop.step()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(nv.cpu().numpy()), _bits(want[t])), t
    loop.close()


def test_cpp_host_passes_them_through(lqro_mod, gains, tmp_path):
    from test_obstacles_cpu import build_obstacles_main, write_obstacles_input
    radii, resp = (0.5, 0.25), 1.0
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    want = _context_two_steps(lqro_mod, gains, x_all, vg, radii, resp)
    exe = build_obstacles_main(tmp_path)
    write_obstacles_input(tmp_path / "in.bin", x_all[:N], vg[:N], H, NP, 2, x_all[N:], radii, resp)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    # (a merge-suspect step ends the program with status 1 after storing newV; this swarm has none)
    assert r.returncode == 0, r.stderr
    got = np.zeros((2, N, 3))
    for line in r.stdout.splitlines():
        t, i, a, b, c = line.split()
        got[int(t), int(i)] = [float.fromhex(a), float.fromhex(b), float.fromhex(c)]
    for t in range(2):
        assert np.array_equal(_bits(got[t]), _bits(want[t])), t


# 10 -----------------------------------------------------------------------
def test_argument_and_state_errors(lqro_mod, gains):
    from test_gpu_dyn import _Hip
    E_ARG, E_STATE = -1, -4
    x_all, vg = obstacle_swarm(lqro_mod, N, M, 11)
    obs = np.ascontiguousarray(x_all[N:])
    ctx = _ctx(lqro_mod, gains, N, "qhull")
    L = lqro_mod.lib()
    p = obs.ctypes.data
    inf, nan = np.inf, np.nan
    for oxy, oz, resp in ((-0.1, 0.5, 1.0), (0.5, -0.1, 1.0), (inf, 0.5, 1.0), (0.5, inf, 1.0), (nan, 0.5, 1.0),
                          (0.5, nan, 1.0), (0.5, 0.5, 0.0), (0.5, 0.5, -0.5), (0.5, 0.5, 1.0000001), (0.5, 0.5, nan),
                          (0.5, 0.5, inf)):
        assert L.lqro_set_obstacles(ctx._h, p, M, oxy, oz, resp) == E_ARG, (oxy, oz, resp)
        assert L.lqro_set_obstacles_device(ctx._h, p, M, oxy, oz, resp) == E_ARG, (oxy, oz, resp)
    assert L.lqro_set_obstacles(None, p, M, 0.5, 0.5, 1.0) == E_ARG
    assert ctx.n_obstacles == 0 and len(_step(lqro_mod, ctx, x_all[:N], vg[:N])) == N   # (a refused call changes nothing)
    assert len(ctx.records()) == N * (N - 1)
    # n_obstacles <= 0 or a null pointer clears, whatever the rest
    ctx.set_obstacles(obs)
    assert L.lqro_set_obstacles(ctx._h, p, 0, -1.0, -1.0, 7.0) == 0
    _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert len(ctx.records()) == N * (N - 1)
    ctx.set_obstacles(obs)
    assert L.lqro_set_obstacles_device(ctx._h, None, M, 0.5, 0.5, 1.0) == 0
    ctx.n_obstacles = 0
    _step(lqro_mod, ctx, x_all[:N], vg[:N])
    assert len(ctx.records()) == N * (N - 1)
    # LQRO_E_STATE between _begin and _end
    hip = _Hip()
    d_x, d_vg = hip.put(x_all[:N]), hip.put(vg[:N])
    tab, nv = hip.put(np.zeros((N, 4))), hip.put(np.zeros((N, 3)))
    try:
        ctx.step_device_begin(d_x, d_vg, tab, 0)
        assert L.lqro_set_obstacles(ctx._h, p, M, 0.5, 0.5, 1.0) == E_STATE
        assert L.lqro_set_obstacles(ctx._h, None, 0, 0.5, 0.5, 1.0) == E_STATE
        assert L.lqro_set_obstacles_device(ctx._h, p, M, 0.5, 0.5, 1.0) == E_STATE
        ctx.step_device_end(tab, nv, 0)
        hip.sync()
        assert L.lqro_set_obstacles(ctx._h, p, M, 0.5, 0.5, 1.0) == 0
    finally:
        ctx.close()
        hip.free()
