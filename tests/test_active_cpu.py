"""The activity mask's CPU side (lqro_set_active): the exports,
the wrappers' argument checks, and the properties of the oracle's compacted
expectations that tests/test_gpu_active.py relies on, measured here on the CPU
oracle and asserted exactly: every mask of the table has planes, inside-hull
pairs and (seed 11) a facet-0 pair, none has a failed hull or a merge suspect,
every mask changes the carried normal; the hot swarm's mask D drops 94 of its
119 inside-hull pairs; and parking an agent far away equals removing it."""
import os
import subprocess

import numpy as np
import pytest

import active_ref as ar
from test_gpu_obstacles import Oracle, _bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIVE_MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_active_main")
N, BOX, H, NP = 24, 3.0, 50, 100
HOT = dict(n=257, box=14.0, seed=7, H=50, NP=50)

# seed, mask: active, planes, inside-hull, stale
TABLE = {
    (11, "ends"): (22, 462, 38, 1),
    (11, "half"): (12, 132, 11, 1),
    (11, "mod3"): (16, 240, 22, 0),
    (11, "odd"): (12, 132, 10, 0),
    (12, "ends"): (22, 462, 38, 0),
    (12, "half"): (12, 132, 10, 0),
    (12, "mod3"): (16, 240, 18, 0),
    (12, "odd"): (12, 132, 16, 0),
}


def test_symbols_and_version(lqro_mod):
    lib = lqro_mod.lib()
    for sym in ("lqro_set_active", "lqro_set_active_device"):
        assert hasattr(lib, sym) and sym in lqro_mod.EXPORTS
    assert lib.lqro_version() == 5          # callers detect the feature by the symbol
    assert lib.lqro_set_active(None, None) == -1 and lib.lqro_set_active_device(None, None) == -1   # LQRO_E_ARG
    text = open(os.path.join(ROOT, "include", "lqro.h")).read()
    assert "int lqro_set_active(lqro_ctx* ctx, const uint8_t* active" in text
    assert "int lqro_set_active_device(lqro_ctx* ctx, const uint8_t* d_active" in text


def test_wrappers_reject_a_wrong_length(lqro_mod):
    ctx = object.__new__(lqro_mod.Context)   # (no device here: the checks come before any library call)
    ctx.cfg, ctx._h = lqro_mod.config(8, 10, 20), None
    for bad in (np.ones(7, bool), np.ones(9, np.uint8), np.ones((8, 1), bool), np.ones(0, bool)):
        with pytest.raises(ValueError):
            ctx.set_active(bad)
    with pytest.raises(ValueError):
        ctx.set_active(np.ones(8, np.float64))
    for cls in (lqro_mod.Simulator, lqro_mod.DeviceLoop):
        host = object.__new__(cls)
        host.ctx = ctx
        with pytest.raises(ValueError):
            host.set_active(np.ones(5, bool))


def test_compaction_helper_numbering():
    a = ar.mask("mod3", 7)                   # 1 and 4 inactive
    assert list(ar.ids(a)) == [0, 2, 3, 5, 6]
    assert ar.slot(3, 5) == 4 and ar.slot(3, 2) == 2 and ar.column(3, 4) == 5 and ar.column(3, 2) == 2
    assert ar.global_column(a, 4, 7) == 6 and ar.global_column(a, 5, 7) == 7 and ar.global_column(a, 6, 7) == 8
    assert ar.pairs(a) == 5 * 4 and ar.pairs(a, m=2) == 5 * 6 and ar.pairs(a, rows=[1, 4]) == 0
    assert ar.pairs(a, m=1, rows=[0, 1, 2]) == 2 * 5
    dt = np.dtype([("i", np.int32), ("j", np.int32), ("flags", np.int32)])
    rc = np.zeros((5, 4 + 1), dt)
    for ic in range(5):
        for qc in range(5):
            rc[ic, qc] = (ic, ar.column(ic, qc), 1)
    out, live = ar.expand_records(a, rc, 7, m=1)
    assert out.shape == (7, 7) and live.sum() == 25
    for i in range(7):
        for q in range(7):
            j = ar.column(i, q)
            assert (out[i, q]["i"], out[i, q]["j"]) == (i, j)
            on = a[i] and (j >= 7 or a[j])
            assert live[i, q] == on and out[i, q]["flags"] == int(on)
    x = ar.park(a, np.zeros((7, 16)))
    assert list(x[4, :6]) == [5e6, -1e7, 3e6, 0, 0, 0] and not x[[0, 2, 3, 5, 6]].any()


_STEP = {}


def compact_step(lqro, orc, seed, name, carry=None):
    """(x, vg, a, newV, records, carry out) of the oracle's Qhull-order step over
    the compacted dense swarm, once."""
    key = (seed, name)
    if key not in _STEP:
        x, vg = lqro.synthetic_swarm(N, box=BOX, seed=seed)
        a = ar.mask(name, N)
        xc, vc = ar.compact(a, x, vg)
        nv, recs, cout = orc.steps(xc, vc, len(xc), "qhull", carry=carry)[0]
        _STEP[key] = (x, vg, a, nv, recs, cout)
    return _STEP[key]


@pytest.fixture(scope="module")
def orc(oracle, gains):
    return Oracle(oracle, gains, h=H, npts=NP)


@pytest.mark.parametrize("seed,name", sorted(TABLE))
def test_compacted_expectations(lqro_mod, orc, seed, name):
    lq = lqro_mod
    x, vg, a, nv, recs, cout = compact_step(lq, orc, seed, name)
    fl = recs["flags"]
    got = (int(a.sum()), int(((fl & lq.REC_PLANE) != 0).sum()), int(((fl & lq.REC_INSIDE) != 0).sum()),
           int(((fl & lq.REC_STALE) != 0).sum()))
    assert got == TABLE[(seed, name)]
    assert not (fl & (lq.REC_HULLFAIL | lq.REC_QHMERGE_WIN)).any()
    *_, call = compact_step(lq, orc, seed, "all")
    assert not np.array_equal(_bits(cout), _bits(call))      # every mask leaves with another carry


@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("name", ["ends", "half", "mod3"])
def test_parking_equals_removal(lqro_mod, orc, seed, name):
    x, vg, a, nv, recs, cout = compact_step(lqro_mod, orc, seed, name)
    pv, _, pc = orc.steps(ar.park(a, x), vg, N, "qhull")[0]
    assert np.array_equal(_bits(pv[ar.ids(a)]), _bits(nv))
    assert np.array_equal(_bits(pc), _bits(cout))


@pytest.fixture(scope="module")
def hot(lqro_mod, oracle, gains):
    x, vg = lqro_mod.synthetic_swarm(HOT["n"], box=HOT["box"], seed=HOT["seed"])
    o = Oracle(oracle, gains, h=HOT["H"], npts=HOT["NP"], threads=8)
    return x, vg, o


def hot_dropped(lqro, recs):
    """D: the even-numbered agents among the rows of the inside-hull pairs."""
    inside = (recs["flags"] & lqro.REC_INSIDE) != 0
    rows = np.unique(recs["i"][inside])
    return rows[rows % 2 == 0]


def test_hot_swarm_mask(lqro_mod, hot):
    lq = lqro_mod
    x, vg, o = hot
    n = HOT["n"]
    _, recs, _ = o.steps(x, vg, n, "qhull")[0]
    fl = recs["flags"]
    assert int(((fl & lq.REC_INSIDE) != 0).sum()) == 119 and int(((fl & lq.REC_PLANE) != 0).sum()) == 65792
    assert not (fl & (lq.REC_STALE | lq.REC_HULLFAIL | lq.REC_QHMERGE_WIN)).any()
    D = hot_dropped(lq, recs)
    assert len(D) == 45
    a = np.ones(n, np.uint8)
    a[D] = 0
    xc, vc = ar.compact(a, x, vg)
    _, rc, _ = o.steps(xc, vc, len(xc), "qhull")[0]
    assert int(((rc["flags"] & lq.REC_INSIDE) != 0).sum()) == 25
    assert int(((rc["flags"] & lq.REC_PLANE) != 0).sum()) == 44732


def test_cpp_consumer_links_and_fails_loudly_without_gpu(lqro_mod, tmp_path):
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is present (tests/test_gpu_active.py covers the run)")
    if not os.path.exists(ACTIVE_MAIN):
        import __graft_entry__ as ge
        ge.build_cpp_active()
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([4, 10, 20, 1], np.int32).tofile(f)
        np.zeros(4 * 16 + 4 * 3).tofile(f)
        np.ones(4, np.uint8).tofile(f)
    r = subprocess.run([ACTIVE_MAIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr
