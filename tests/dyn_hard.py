"""Helpers shared by the hard-case tests of the dynamics step
(test_dyn_hard_cpu.py, test_gpu_dyn_edges.py, golden/make_golden_dyn.py):
dyn_cases.hard_case's arrays as the state dict, gains and models that
lqro.dynamics_step and pyoracle.agent_step take."""
from __future__ import annotations

import ctypes as C

import numpy as np

from dyn_cases import HARD_FAMILIES, MODEL_FIELDS, model_variants

STATE = ("x", "rot", "x_true", "rot_true", "P", "vgoal")
AGENT = STATE + ("u_goal", "p_goal")
GAINS = ("L", "E", "l", "Lh", "Eh")
L_TERM = (0.01, -0.02, 0.03, -0.04)   # exercises the + l term, as tests/test_gpu_dyn.py does


def states(cs: dict) -> dict:
    return {k: np.ascontiguousarray(cs[k], np.float64).copy() for k in AGENT}


def _default_fields(oracle) -> dict:
    m = oracle.Model()
    oracle.lib().orc_model_default(C.byref(m))
    return {f: getattr(m, f) for f in MODEL_FIELDS}


def models(oracle, cs: dict, cls=None):
    """None (the default model) or one model per agent, as `cls` structures
    (pyoracle.Model by default; lqro.Model has the same fields)."""
    if cs["model_ix"] is None:
        return None
    cls = cls or oracle.Model
    var = model_variants(_default_fields(oracle))
    return [cls(*[var[i][f] for f in MODEL_FIELDS]) for i in cs["model_ix"]]


def gains(oracle, cs: dict):
    """(gains, per_agent): the default model's gains with l = L_TERM, or, for
    per-agent models, each model's own controlMatrices stacked (the oracle's
    synthesis, which lqro_synthesize_gains_batch equals bit for bit,
    tests/test_gpu_synth.py)."""
    ms = models(oracle, cs)
    if ms is None:
        g = oracle.synthesize()
        g["l"] = np.array(L_TERM)
        return g, False
    distinct = {}
    for i, m in zip(cs["model_ix"], ms):
        if int(i) not in distinct:
            distinct[int(i)] = oracle.synthesize(m)
    g = {k: np.stack([distinct[int(i)][k] for i in cs["model_ix"]]) for k in GAINS}
    g["l"] = g["l"] + np.array(L_TERM)
    return g, True


def oracle_step(oracle, cs: dict, st: dict, g: dict, per_agent: bool) -> np.ndarray:
    return oracle.agent_step(st, g, cs["nrm"], models=models(oracle, cs), M=cs["M"], N=cs["N"],
                             per_agent=per_agent)


def rel_err(a: np.ndarray, b: np.ndarray) -> float:
    """tests/test_gpu_dyn.py's _close metric: relative to max(|b|, 1e-3 max|b|)."""
    scale = np.maximum(np.abs(b), 1e-3 * np.abs(b).max() + 1e-300)
    return float((np.abs(a - b) / scale).max())


# ---- the noise path and the filters, function by function -----------------
# (tests/test_oracle_dyn.py, tests/golden/make_golden_dyn.py: the oracle
# against the reference's own code, live and from tests/golden/dyn_hard.npz)
REF_FAMILIES = tuple(f for f in HARD_FAMILIES if not f.startswith("models"))
REF_INPUTS = ("x", "rot", "x_true", "rot_true", "P", "vgoal", "u_goal", "p_goal", "nrm", "M", "N")


def ref_agents(name: str) -> int:
    """Agents per family in the fixture: 4, or 8 where the family is a list of rotations."""
    return 8 if name.partition("@")[0] in ("exact", "quat") else 4


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleFns:
    """The oracle's functions in the call shapes of RefFns."""

    def __init__(self, oracle):
        self.o = oracle.lib()
        self.o.orc_sample_gaussian.argtypes = [C.c_int] + [C.c_void_p] * 4
        self.m = oracle.Model()
        self.o.orc_model_default(C.byref(self.m))

    def control_velocity(self, *a): self.o.orc_control_velocity(*a)
    def control_position(self, *a): self.o.orc_control_position(*a)
    def jacobi(self, n, m, V, D): self.o.orc_jacobi(n, m, V, D)
    def sample(self, n, mean, var, nrm, out): self.o.orc_sample_gaussian(n, mean, var, nrm, out)
    def propagate(self, x, R, u, M, nrm): self.o.orc_propagate(C.byref(self.m), x, R, u, M, nrm)
    def kalman1(self, x, R, u, M, P): self.o.orc_kalman1(C.byref(self.m), x, R, u, M, P)
    def kalman2(self, x, R, z, N, P): self.o.orc_kalman2(C.byref(self.m), x, R, z, N, P)


class RefFns:
    """oracle/_ref/libref.so: the reference's own functions."""

    def __init__(self, r):
        self.r = r

    def control_velocity(self, *a): self.r.ref_control_velocity(*a)
    def control_position(self, *a): self.r.ref_control_position(*a)
    def jacobi(self, n, m, V, D): assert self.r.ref_jacobi(n, m, V, D) == 0
    def sample(self, n, mean, var, nrm, out):
        {6: self.r.ref_sample_gaussian6, 16: self.r.ref_sample_gaussian16}[n](mean, var, nrm, out)
    def propagate(self, *a): self.r.ref_propagate(*a)
    def kalman1(self, *a): self.r.ref_kalman1_m(*a)
    def kalman2(self, *a): self.r.ref_kalman2_n(*a)


def by_function(fn, cs: dict, g: dict) -> dict:
    """One agent step (LQRO:1438-1445) as a chain of `fn`'s functions, every
    link's result kept: findU, propagate, kalmanFilter1, the observation draw,
    kalmanFilter2, findVGoal; then sampleGaussian<16> on M itself and jacobi
    of M and N."""
    c = {k: np.ascontiguousarray(cs[k], np.float64) for k in REF_INPUTS}
    n = c["x"].shape[0]
    gg = {k: np.ascontiguousarray(g[k], np.float64) for k in GAINS}
    out = dict(u=np.zeros((n, 4)), pr_x=c["x_true"].copy(), pr_rot=c["rot_true"].copy(),
               k1_x=c["x"].copy(), k1_rot=c["rot"].copy(), k1_P=c["P"].copy(), z=np.zeros((n, 6)),
               v=np.zeros((n, 3)), sg16=np.zeros((n, 16)))
    zero16 = np.zeros(16)
    for a in range(n):
        fn.control_velocity(_p(c["x"][a]), _p(c["rot"][a]), _p(c["vgoal"][a]), _p(c["u_goal"][a]),
                            _p(gg["L"]), _p(gg["E"]), _p(gg["l"]), _p(out["u"][a]))
        fn.propagate(_p(out["pr_x"][a]), _p(out["pr_rot"][a]), _p(out["u"][a]), _p(c["M"]), _p(c["nrm"][a]))
        fn.kalman1(_p(out["k1_x"][a]), _p(out["k1_rot"][a]), _p(out["u"][a]), _p(c["M"]), _p(out["k1_P"][a]))
        hx = np.concatenate([out["pr_x"][a, 9:12], out["pr_x"][a, 0:3]])     # h (LQRO:399-419)
        fn.sample(6, _p(hx), _p(c["N"]), _p(c["nrm"][a, 16:]), _p(out["z"][a]))
        fn.sample(16, _p(zero16), _p(c["M"]), _p(c["nrm"][a]), _p(out["sg16"][a]))
    for k in ("x", "rot", "P"):
        out["k2_" + k] = out["k1_" + k].copy()
    for a in range(n):
        fn.kalman2(_p(out["k2_x"][a]), _p(out["k2_rot"][a]), _p(out["z"][a]), _p(c["N"]), _p(out["k2_P"][a]))
        fn.control_position(_p(out["k2_x"][a]), _p(out["k2_rot"][a]), _p(c["p_goal"][a]), _p(c["u_goal"][a]),
                            _p(gg["Lh"]), _p(gg["Eh"]), _p(out["v"][a]))
    for key, m in (("jM", c["M"]), ("jN", c["N"])):
        k = m.shape[0]
        V, D = np.zeros((k, k)), np.zeros((k, k))
        fn.jacobi(k, _p(m), _p(V), _p(D))
        assert np.array_equal(D, np.diag(np.diag(D)))
        out[key + "_V"], out[key + "_d"] = V, np.diag(D).copy()
    return out
