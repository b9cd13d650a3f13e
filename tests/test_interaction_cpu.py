"""The interaction classes' CPU side (lqro_set_interaction): the
exports, the wrappers' argument checks, and the reference walk of
tests/interaction_ref.py pinned against the oracle as it stands: with `uniform`
it IS the oracle's step, with `ghost` its class-0 rows are the oracle's step
over the compacted class-0 swarm.  Also here, measured on the CPU oracle and
asserted exactly, what the seeds of tests/test_gpu_interaction.py must show."""
import os
import subprocess

import numpy as np
import pytest

import active_ref as ar
import interaction_ref as ir
from test_gpu_obstacles import PAIR_LOCAL, WALKED, Oracle, _bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERACTION_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_interaction_main")
RULES = ("qhull", "canonical")
N, BOX, H, NP = 24, 3.0, 50, 100
# table: seed.  Chosen on the CPU (the oracle's Qhull-order step of seeds 11..30
# at these shapes): seed 30 has its one facet-0 pair at (21, 1), the first live
# slot of row 21 under `priority` and `teams`; seed 16 at (15, 0), live under
# `weights`.  seed_conditions() states what each must show.
SEEDS = {"priority": 30, "teams": 30, "weights": 16}


@pytest.fixture(scope="module")
def orc(oracle, gains):
    return Oracle(oracle, gains, h=H, npts=NP)


_LOCAL = {}


def local_for(lqro, orc, seed, rule, n=N, box=BOX, oracle_obj=None):
    """(x, vg, the oracle's own first step (newV, records, carry out)) of the
    dense swarm without a table: the pair-local fields of every later walk."""
    key = (seed, rule, n, box)
    if key not in _LOCAL:
        x, vg = lqro.synthetic_swarm(n, box=box, seed=seed)
        _LOCAL[key] = (x, vg, (oracle_obj or orc).steps(x, vg, n, rule)[0])
    return _LOCAL[key]


def expectation(lqro, oracle, orc, name, seed, rule, steps=2, n=N, cls=None, table=None, active=None):
    """[(records, newV, carry out, planes per row)] of `steps` consecutive
    steps under the named table (the same x and vGoal every step: only the
    carry moves on), and (x, vg, cls, share, fac, live, local records)."""
    x, vg, (_, local, _) = local_for(lqro, orc, seed, rule, n=n)
    c, share = ir.table(name) if table is None else table
    cls = ir.classes(n, c) if cls is None else np.asarray(cls, np.uint8)
    fac, live = ir.factors(cls, share, n, active=active)
    out, carry = [], np.zeros(3)
    for _ in range(steps):
        recs, nv, carry, cnt = ir.walk(lqro, oracle, local, x, vg, n, fac, live, carry, active=active)
        out.append((recs, nv, carry, cnt))
    return out, (x, vg, cls, share, fac, live, local)


def seed_conditions(lqro, local, fac, live, rule):
    """What a seed must show (asserted, never skipped): (live inside-hull
    pairs whose share is neither 0 nor 0.5, dead slots that are inside-hull
    without the table, in Qhull order the REC_STALE pairs whose carry comes
    from another row)."""
    fl = local["flags"]
    inside = (fl & lqro.REC_INSIDE) != 0
    agent = local["j"] < local.shape[0]
    odd = int((inside & live & agent & (fac != 0.5) & (fac != 0.0)).sum())
    dead = int((inside & ~live).sum())
    far = [rq for rq in ir.stale_from_another_row(lqro, local, live) if rq[0] > 0] if rule == "qhull" else None
    return odd, dead, far


def assert_seed(lqro, local, fac, live, rule, share, what=""):
    """(`teams` holds no share other than 0 and 0.5, so no seed can show it a
    live pair with one: that condition is asserted for the tables that have
    such a share, and for `teams` that it has none.)"""
    odd, dead, far = seed_conditions(lqro, local, fac, live, rule)
    has_odd = bool(((share != 0.0) & (share != 0.5)).any())
    assert (odd >= 1) == has_odd and dead >= 1, (what, odd, dead)
    assert not (local["flags"] & (lqro.REC_HULLFAIL | lqro.REC_QHMERGE_WIN)).any(), what
    if rule == "qhull":
        assert len(far) >= 1, (what, "no facet-0 pair takes its carry from another row")


def test_symbols_and_version(lqro_mod):
    lib = lqro_mod.lib()
    for sym in ("lqro_set_interaction", "lqro_set_interaction_device"):
        assert hasattr(lib, sym) and sym in lqro_mod.EXPORTS
    assert lib.lqro_version() == 5          # callers detect the feature by the symbol
    sh = np.full((2, 2), 0.5)
    k = np.zeros(4, np.uint8)
    for f in (lib.lqro_set_interaction, lib.lqro_set_interaction_device):   # a null context: LQRO_E_ARG
        assert f(None, None, 0, None) == -1
        assert f(None, lqro_mod._p(k), 2, lqro_mod._p(sh)) == -1
    text = open(os.path.join(ROOT, "include", "lqro.h")).read()
    assert "#define LQRO_CLASSES_MAX 16" in text and lqro_mod.LQRO_CLASSES_MAX == 16 == ir.CLASSES_MAX
    assert "int lqro_set_interaction(lqro_ctx* ctx, const uint8_t* cls" in text
    assert "int lqro_set_interaction_device(lqro_ctx* ctx, const uint8_t* d_cls" in text


def test_wrappers_reject_bad_arguments(lqro_mod):
    ctx = object.__new__(lqro_mod.Context)   # (no device here: the checks come before any library call)
    ctx.cfg, ctx._h = lqro_mod.config(8, 10, 20), None
    ok_sh, ok_k = np.full((2, 2), 0.5), np.zeros(8, np.uint8)
    bad_share = (np.full((2, 3), 0.5), np.full(4, 0.5), np.full((17, 17), 0.5), np.zeros((0, 0)),
                 np.array([[0.5, 1.5], [0.5, 0.5]]), np.array([[0.5, -1e-300], [0.5, 0.5]]),
                 np.array([[0.5, np.nan], [0.5, 0.5]]), np.array([[0.5, np.inf], [0.5, 0.5]]))
    for sh in bad_share:
        with pytest.raises(ValueError):
            ctx.set_interaction(ok_k, sh)
    bad_cls = (np.zeros(7, np.uint8), np.zeros(9, np.uint8), np.zeros((8, 1), np.uint8), np.zeros(0, np.uint8),
               np.full(8, 2, np.uint8), np.full(8, -1), np.zeros(8, np.float64))
    for k in bad_cls:
        with pytest.raises(ValueError):
            ctx.set_interaction(k, ok_sh)
    with pytest.raises(ValueError):
        ctx.set_interaction(ok_k, ok_sh, device=True)      # (a host array is no device array)
    for cls in (lqro_mod.Simulator, lqro_mod.DeviceLoop):
        host = object.__new__(cls)
        host.ctx = ctx
        with pytest.raises(ValueError):
            host.set_interaction(np.zeros(5, np.uint8), ok_sh)


def test_tables_and_pairs_formula():
    assert sorted(ir.TABLES) == ["ghost", "priority", "teams", "uniform", "weights"]
    c, sh = ir.table("teams")
    assert c == 3 and (np.diag(sh) == 0).all() and (sh[~np.eye(3, dtype=bool)] == 0.5).all()
    c, sh = ir.table("ghost")
    assert sh[0, 0] == 0.5 and sh.sum() == 0.5
    c, sh = ir.table("weights")
    assert sh[1, 2] == 1e-300 and sh[2, 0] == 0.0 and sh[0, 1] + sh[1, 0] == 1.0
    cls = ir.classes(7, 3)                                  # 0 1 2 0 1 2 0: 3, 2, 2 agents
    assert ir.pairs(cls, np.full((3, 3), 0.5), 7) == 7 * 6 and ir.pairs(cls, np.full((3, 3), 0.5), 7, m=2) == 7 * 8
    assert ir.pairs(cls, ir.table("teams")[1], 7) == 3 * 4 + 2 * 5 + 2 * 5
    assert ir.pairs(cls, ir.table("weights")[1], 7) == 3 * 6 + 2 * 6 + 2 * 3
    assert ir.pairs(cls, ir.table("weights")[1], 7, m=1, rows=[2, 3]) == (3 + 1) + (6 + 1)
    a = np.array([1, 1, 0, 0, 1, 1, 1])                    # active: classes 0 1 . . 1 2 0
    assert ir.pairs(cls, ir.table("teams")[1], 7, active=a) == 3 + 3 + 3 + 4 + 3
    fac, live = ir.factors(cls, ir.table("weights")[1], 7, m=1, resp=0.75, active=a)
    assert fac.shape == (7, 7) and live.sum() == ir.pairs(cls, ir.table("weights")[1], 7, m=1, active=a)
    assert fac[1, 1] == 1e-300 and live[1, 4] and fac[5, 0] == 0.0 and not live[5, 0] and fac[5, 6] == 0.75
    assert not live[2].any() and not live[:, 2][[0, 1]].any()


@pytest.mark.parametrize("rule", RULES)
def test_uniform_walk_is_the_oracles_step(lqro_mod, oracle, orc, rule):
    x, vg = lqro_mod.synthetic_swarm(N, box=BOX, seed=16)
    ref = orc.steps(x, vg, N, rule, steps=2)
    got, _ = expectation(lqro_mod, oracle, orc, "uniform", 16, rule)
    for t in range(2):
        recs, nv, carry, cnt = got[t]
        for f in PAIR_LOCAL + WALKED:
            a, b = recs[f], ref[t][1][f]
            assert np.array_equal(_bits(a) if a.dtype.kind == "f" else a, _bits(b) if b.dtype.kind == "f" else b), (t, f)
        assert np.array_equal(_bits(nv), _bits(ref[t][0])), t
        if rule == "qhull":
            assert np.array_equal(_bits(carry), _bits(ref[t][2])), t
    if rule == "qhull":                                     # (the walk's carry branch is taken)
        assert ((ref[0][1]["flags"] & lqro_mod.REC_STALE) != 0).sum() == 1


@pytest.mark.parametrize("rule", RULES)
def test_ghost_rows_are_the_compacted_swarm(lqro_mod, oracle, orc, rule):
    got, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, "ghost", 16, rule)
    a = (cls == 0).astype(np.uint8)
    xc, vc = ar.compact(a, x, vg)
    ref = orc.steps(xc, vc, len(xc), rule, steps=2)
    rows0 = ar.ids(a)
    for t in range(2):
        recs, nv, carry, cnt = got[t]
        want, wl = ar.expand_records(a, ref[t][1], N)
        assert np.array_equal(wl[rows0], live[rows0]) and not live[cls == 1].any()
        for f in PAIR_LOCAL + WALKED:
            u, v = recs[f][rows0], want[f][rows0]
            assert np.array_equal(_bits(u) if u.dtype.kind == "f" else u, _bits(v) if v.dtype.kind == "f" else v), (t, f)
        assert not recs["flags"][cls == 1].any()
        assert np.array_equal(_bits(nv[rows0]), _bits(ref[t][0]))
        for i in np.nonzero(cls == 1)[0]:               # nothing to avoid: the LP over no plane
            assert np.array_equal(_bits(nv[i]), _bits(oracle.newv(np.zeros((0, 6), np.float32), vg[i], 100.0)))
        if rule == "qhull":
            assert np.array_equal(_bits(carry), _bits(ref[t][2])), t
    assert ir.pairs(cls, share, N) == ar.pairs(a)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(SEEDS))
def test_seeds_show_what_the_gpu_tests_need(lqro_mod, oracle, orc, name, rule):
    got, (x, vg, cls, share, fac, live, local) = expectation(lqro_mod, oracle, orc, name, SEEDS[name], rule)
    assert_seed(lqro_mod, local, fac, live, rule, share, what=(name, rule))
    plain = orc.steps(x, vg, N, rule)[0]
    assert (_bits(got[0][1]) != _bits(plain[0])).any()       # the table shows in newV
    assert int(live.sum()) == ir.pairs(cls, share, N)


def test_cpp_consumer_links_and_fails_loudly_without_gpu(lqro_mod, tmp_path):
    import torch
    if not os.path.exists(INTERACTION_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_interaction()
    n = 4
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([n, 10, 20, 1, 2], np.int32).tofile(f)
        np.zeros(n * 16 + n * 3).tofile(f)
        np.full(4, 0.5).tofile(f)
        np.zeros(n, np.uint8).tofile(f)
    r = subprocess.run([INTERACTION_MAIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=60)
    if torch.cuda.device_count() > 0:        # (with a device the program runs: tests/test_gpu_interaction.py reads it)
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr
