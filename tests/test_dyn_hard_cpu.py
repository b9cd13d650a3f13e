"""The hard cases of the dynamics step (dyn_cases.HARD_FAMILIES) on the CPU.

1. Condition.  Every family's oracle result is finite and moves by at most
   1e-10 (tests/test_gpu_dyn.py's metric) when every input element is moved
   by a random +-1 ulp: ten times inside the GPU tests' 1e-9, so a GPU result
   outside 1e-9 is an error of the kernel and not the case's own sensitivity.
   A family that misses this gets another seed or size, not another bound.
2. The kernel's source, compiled for the host with the library's
   floating-point flags (tests/cpp/lqro_dyn_host.cpp, built by
   __graft_entry__.build()), against the oracle: equal bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest

import dyn_hard
from conftest import ROOT
from dyn_cases import HARD_FAMILIES, hard_case

HOST_LIB = os.path.join(ROOT, "tests", "cpp", "liblqro_dyn_host.so")
OUT = dyn_hard.STATE + ("u",)
N_AGENTS = 16

# Inputs whose exact values are what the family is about; every other input
# of the family is perturbed.  Moving them removes the family's subject and
# is answered by a jump, not by rounding error:
# - ties: N's equal off-diagonals.  One ulp decides which pivot the Jacobi
#   takes first, so the eigenvectors V turn inside N's five-fold eigenspace
#   and V sqrt(D) g is another (equally valid) draw: x moves by 7e-3.  The
#   GPU reads the same bits, and the equal entries stay equal through the
#   rotations (the same operations on the same values), so the tie rule is
#   decided identically whatever hypot's last bit.
# - exact: rotations with entries 0 and +-1.  At a quarter turn sinangle is
#   exactly 1, where asin has no derivative: 1 - 2^-53 gives pi/2 - 1.5e-8
#   and 1 + 2^-52 gives NaN.  With the exact entries sinangle is computed
#   without rounding on the host and on the device alike.
# - M or N with one value on the whole diagonal (the reference's 1e-9 I, and
#   ties again): at hover (Rot = I, agent 0 of every family) MM then has
#   exactly equal diagonal pairs with a non-zero entry between them, theta is
#   exactly 0 and the rotation is +45 degrees; an ulp on one diagonal entry
#   makes theta -1e-12 and the rotation -45 degrees, so two eigenvectors swap
#   and x_true moves by the whole noise draw (3e-6).  The equal entries come
#   from the same operations on the same values, on the device too.
EXACT_INPUTS = {"ties": ("M", "N"), "exact": ("rot", "rot_true")}


def _exact(name, key, value):
    if key in ("M", "N") and len(np.unique(np.diag(value))) == 1:
        return True
    return key in EXACT_INPUTS.get(name.partition("@")[0], ())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def results(oracle):
    """name -> (case, gains, per_agent, the oracle's outputs), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cs = hard_case(name, N_AGENTS)
            g, per = dyn_hard.gains(oracle, cs)
            st = dyn_hard.states(cs)
            u = dyn_hard.oracle_step(oracle, cs, st, g, per)
            cache[name] = (cs, g, per, dict(st, u=u))
        return cache[name]
    return get


def _ulp(a, rng):
    a = np.asarray(a, np.float64)
    return np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))


@pytest.mark.parametrize("name", HARD_FAMILIES)
def test_condition(oracle, results, name):
    cs, g, per, ref = results(name)
    for k in OUT:
        assert np.all(np.isfinite(ref[k])), k
    errs = dict.fromkeys(OUT, 0.0)
    for draw in range(4):
        rng = np.random.default_rng([0x554C50, HARD_FAMILIES.index(name), draw])
        cp = dict(cs)
        for k in dyn_hard.AGENT + ("M", "N", "nrm"):
            if not _exact(name, k, cs[k]):
                cp[k] = _ulp(cs[k], rng)
        gp = {k: _ulp(g[k], rng) for k in dyn_hard.GAINS}
        st = dyn_hard.states(cp)
        u = dyn_hard.oracle_step(oracle, cp, st, gp, per)
        got = dict(st, u=u)
        errs = {k: max(errs[k], dyn_hard.rel_err(got[k], ref[k])) for k in OUT}
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    for k in OUT:
        assert errs[k] <= 1e-10, f"{name} {k}: moves by {errs[k]:.3e} under +-1 ulp"


@pytest.mark.parametrize("name", HARD_FAMILIES)
def test_host_build_bit_for_bit(oracle, results, name):
    if not os.path.exists(HOST_LIB):
        pytest.skip("tests/cpp/liblqro_dyn_host.so not built (__graft_entry__.build())")
    h = C.CDLL(HOST_LIB)
    vp = C.c_void_p
    h.lqro_dyn_host_agent_step.argtypes = [vp] * 11 + [C.c_double] + [vp] * 8
    h.lqro_dyn_host_agent_step.restype = None
    cs, g, per, ref = results(name)
    st = dyn_hard.states(cs)
    n = st["x"].shape[0]
    u = np.zeros((n, 4))
    kf = np.zeros((n, 8), np.float32)
    ms = dyn_hard.models(oracle, cs)
    m0 = oracle.Model()
    oracle.lib().orc_model_default(C.byref(m0))
    M, N = np.ascontiguousarray(cs["M"]), np.ascontiguousarray(cs["N"])
    nrm = np.ascontiguousarray(cs["nrm"])
    for a in range(n):
        ga = {k: np.ascontiguousarray(g[k][a] if per else g[k], np.float64) for k in dyn_hard.GAINS}
        h.lqro_dyn_host_agent_step(C.byref(ms[a] if ms else m0), *[_p(ga[k]) for k in dyn_hard.GAINS],
                                   _p(st["u_goal"][a]), _p(st["p_goal"][a]), _p(M), _p(N), _p(nrm[a]), 1.25,
                                   *[_p(st[k][a]) for k in dyn_hard.STATE], _p(u[a]), _p(kf[a]))
    got = dict(st, u=u)
    for k in OUT:
        assert np.array_equal(got[k].view(np.uint64), ref[k].view(np.uint64)), \
            f"{name} {k}: max rel err {dyn_hard.rel_err(got[k], ref[k]):.3e}"
    assert np.array_equal(kf.view(np.uint32),
                          oracle.keyframes(1.25, ref["x_true"], ref["rot_true"]).view(np.uint32))


@pytest.mark.parametrize("what", ["n models, shared gains", "1 model, per-agent gains"])
def test_condition_mixed_switches(oracle, what):
    """The same condition for the two mixed (n_models, per_agent_gains) cases
    of tests/test_gpu_dyn_edges.py::test_model_and_gain_switches."""
    cs = hard_case("models", N_AGENTS)
    gb, _ = dyn_hard.gains(oracle, cs)
    g0, _ = dyn_hard.gains(oracle, dict(cs, model_ix=None))
    m0 = oracle.Model()
    oracle.lib().orc_model_default(C.byref(m0))
    ms, g, per = (dyn_hard.models(oracle, cs), g0, False) if what.startswith("n") else ([m0], gb, True)

    def run(c, gg):
        st = dyn_hard.states(c)
        u = oracle.agent_step(st, gg, c["nrm"], models=ms, M=c["M"], N=c["N"], per_agent=per)
        return dict(st, u=u)
    ref = run(cs, g)
    for k in OUT:
        assert np.all(np.isfinite(ref[k])), k
    for draw in range(4):
        rng = np.random.default_rng([0x4D4958, draw])
        cp = dict(cs)
        for k in dyn_hard.AGENT + ("M", "N", "nrm"):
            if not _exact("models", k, cs[k]):
                cp[k] = _ulp(cs[k], rng)
        got = run(cp, {k: _ulp(g[k], rng) for k in dyn_hard.GAINS})
        for k in OUT:
            err = dyn_hard.rel_err(got[k], ref[k])
            assert err <= 1e-10, f"{what} {k}: moves by {err:.3e} under +-1 ulp"
