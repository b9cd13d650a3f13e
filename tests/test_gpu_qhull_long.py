"""k_qhull's long partition sequences (insertions that re-partition more than
one 64-point chunk) on the C3 swarm's slowest builds, in every setting of the
switches that change how a sequence is located (LQRO_QHULL_FLAGS):

- 32: without sharp new facets the findbest_notsharp trigger is no event;
- 64: with sharp new facets the helper waves are posted under findbestnew = 1,
  the state the trigger leads to, and their chunks stand once it has fired;
- 1: the helper waves themselves.

Inputs: the reachable sets of the C3 pairs (904, 106), (106, 904) and
(531, 376) from the CPU oracle, rounded as qconvex's input is (round6), every
fourth point of each (about 2,200 points) and the full set of (904, 106)
(8,856 points, one partition of 4,214), injected through Context.debug_qhull.
Counted with the oracle's build: the thinned sets hold 45 / 57 / 48 long
sequences, 28 / 35 / 31 of them with sharp new facets and a trigger (4 / 8 /
10 after the sequence's first chunk) and 3 / 6 / 7 with a trigger but no sharp
facets; the full set 132, 61 (4) and 48, with not-sharp triggers in one-chunk
insertions too.

Expected: the oracle's restatement of Qhull's build (pyoracle.qhull) and its
selection (hull_branch_ref): the facet list in Fv order, the facet count, the
distance, the normal and the stale flag, bit for bit, whatever the setting."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [((904, 106), 4), ((106, 904), 4), ((531, 376), 4), ((904, 106), 1)]

# LQRO_QHULL_FLAGS: the default (None: 119), each new bit cleared alone, both
# cleared, and the helper waves off
SETTINGS = {"default": None, "no32": "87", "no64": "55", "no32_no64": "23", "helpers_off": "118"}


@pytest.fixture(scope="module")
def long_inputs(lqro_mod, oracle, gains):
    N, H, NP = 1024, 100, 100
    x, _ = lqro_mod.synthetic_swarm(N)
    T, NCF = oracle.tables(gains["A"], gains["B"], gains["L"], gains["E"], H)
    S = oracle.sphere(NP)
    r6 = np.vectorize(oracle.round6)
    out = []
    oracle.set_hull_rule(1, round16=True)
    try:
        for (i, j), every in PAIRS:
            rec, _, full = oracle.pair(T, NCF, S, x[i], x[j], i, j, want_points=True)
            assert rec["flags"] & lqro_mod.REC_INSIDE, (i, j)
            full = np.ascontiguousarray(full[::every])
            rounded = np.ascontiguousarray(r6(full))
            vrel = x[i, 3:6] - x[j, 3:6]
            st, fv, _, _ = oracle.qhull(rounded)
            assert st == 0, (i, j, every, st)
            nf, dist, nrm, fac, _ = oracle.hull_branch_ref(full, vrel)
            assert nf == len(fv)
            out.append(((i, j, every), rounded, full, vrel, fv, dist, nrm, np.array(fac)))
    finally:
        oracle.set_hull_rule(0)
    assert len(out[3][1]) > 8000 and all(2000 < len(o[1]) < 2400 for o in out[:3])
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_long_sequences_every_setting(lqro_mod, gains, monkeypatch, long_inputs, setting):
    monkeypatch.delenv("LQRO_QHULL_FLAGS", raising=False)
    monkeypatch.delenv("LQRO_QHULL_BIG", raising=False)
    if SETTINGS[setting] is not None:
        monkeypatch.setenv("LQRO_QHULL_FLAGS", SETTINGS[setting])
    ctx = lqro_mod.Context(lqro_mod.config(2, 100, 100))   # (the knob is read here)
    ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
    try:
        for name, rounded, full, vrel, fv, dist, nrm, fac in long_inputs:
            rec, st, fl = ctx.debug_qhull(rounded, full, vrel, max_facets=8192)
            assert st == 0, (setting, name, st)
            same = 0
            while same < min(len(fl), len(fv)) and np.array_equal(fl[same], fv[same]):
                same += 1
            assert len(fl) == len(fv) and same == len(fv), \
                f"{setting} {name}: {len(fl)} facets ({len(fv)} in Qhull's build), first difference at {same}"
            assert rec["n_facets"] == len(fv), (setting, name)
            assert list(rec["facet"]) == list(fac), (setting, name)
            assert np.float64(rec["dist"]).view(np.uint64) == np.float64(dist).view(np.uint64), (setting, name)
            assert bool(rec["flags"] & lqro_mod.REC_STALE) == (nrm is None), (setting, name)
            if nrm is not None:
                assert np.array_equal(np.asarray(rec["normal"], np.float64).view(np.uint64), nrm.view(np.uint64)), \
                    (setting, name)
    finally:
        ctx.close()
