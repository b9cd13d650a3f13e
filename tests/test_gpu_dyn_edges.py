"""The per-agent step after the pair loop (lqro_dynamics_step[_device], k_dynw
and k_dyn) on the inputs tests/test_gpu_dyn.py does not reach:

- the hard families of dyn_cases.py: dense, tied, block and asymmetric noise
  covariances (k_dynw's 6x6 and 16x16 Jacobi rotations run), tilts past 90
  degrees, exact quarter and half turns, rotation errors, high body rates,
  per-agent models.  k_dynw and k_dyn agree bit for bit, both match the oracle
  to test_gpu_dyn.py's 1e-9 (every family's own sensitivity is below 1e-10,
  tests/test_dyn_hard_cpu.py), the keyframes bit for bit;
- proof from k_dynw's own counters that the rotations and other squaring
  counts were executed;
- launch edges (n = 1, 63, 64, 65), the four (n_models, per_agent_gains)
  combinations, memory past agent n and the read-only inputs, null u and
  keyframes, and the LQRO_E_ARG returns."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-9   # tests/test_gpu_dyn.py's one-step tolerance
LQRO_E_ARG = -1


if __name__ == "__main__":   # the coverage child (below): no conftest has set the path
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "lqr-obstacles_amd"),
                    os.path.join(os.path.dirname(HERE), "oracle"), HERE]

import dyn_hard  # noqa: E402
from dyn_cases import HARD_FAMILIES, hard_case  # noqa: E402

OUT = dyn_hard.STATE + ("u",)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _gains(lqro_mod, oracle, cs):
    """(gains, models, per_agent): per-agent models take their gains from
    lqro_synthesize_gains_batch."""
    if cs["model_ix"] is None:
        g, _ = dyn_hard.gains(oracle, cs)
        return g, None, False
    ms = dyn_hard.models(oracle, cs, cls=lqro_mod.Model)
    gb = lqro_mod.synthesize_gains_batch(ms)
    gb["l"] = gb["l"] + np.array(dyn_hard.L_TERM)
    return gb, ms, True


@contextlib.contextmanager
def _kernel(lane):
    """LQRO_DYN_LANE (read at every call): 0 k_dynw, 1 k_dyn."""
    old = os.environ.get("LQRO_DYN_LANE")
    os.environ["LQRO_DYN_LANE"] = str(lane)
    try:
        yield
    finally:
        if old is None:
            del os.environ["LQRO_DYN_LANE"]
        else:
            os.environ["LQRO_DYN_LANE"] = old


def _step(lqro_mod, lane, cs, g, ms, per, keyframes=None, time=0.0):
    """One lqro_dynamics_step through k_dynw (lane 0) or k_dyn (lane 1)."""
    st = dyn_hard.states(cs)
    with _kernel(lane):
        u = lqro_mod.dynamics_step(st, g, cs["nrm"], models=ms, M=cs["M"], N=cs["N"], per_agent=per,
                                   keyframes=keyframes, time=time)
    return dict(st, u=u)


def _same(a, b, what):
    for k in OUT:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _errors(got, ref):
    return {k: dyn_hard.rel_err(got[k], ref[k]) for k in OUT}


def _oracle(oracle, cs, g, ms, per):
    st = dyn_hard.states(cs)
    u = oracle.agent_step(st, g, cs["nrm"], models=ms, M=cs["M"], N=cs["N"], per_agent=per)
    return dict(st, u=u)


def _head(cs, n):
    """The first n agents of a case."""
    return {k: (v[:n] if isinstance(v, np.ndarray) and k not in ("M", "N") else v) for k, v in cs.items()}


# ---- hard cases ------------------------------------------------------------
@pytest.mark.parametrize("name", HARD_FAMILIES)
def test_hard_cases(lqro_mod, oracle, name):
    n = 16
    cs = hard_case(name, n)
    g, ms, per = _gains(lqro_mod, oracle, cs)
    kf = [np.zeros((n, 8), np.float32) for _ in range(2)]
    wave = _step(lqro_mod, 0, cs, g, ms, per, keyframes=kf[0], time=1.25)
    lane = _step(lqro_mod, 1, cs, g, ms, per, keyframes=kf[1], time=1.25)
    ref = _oracle(oracle, cs, g, ms, per)
    ew, el = _errors(wave, ref), _errors(lane, ref)
    print(f"\nDYNERR {name} k_dynw " + " ".join(f"{k}={v:.2e}" for k, v in ew.items()))
    print(f"DYNERR {name} k_dyn  " + " ".join(f"{k}={v:.2e}" for k, v in el.items()))
    _same(wave, lane, f"{name}: k_dynw against k_dyn")
    assert np.array_equal(_bits(kf[0]), _bits(kf[1]))
    for k in OUT:
        assert np.all(np.isfinite(wave[k])), k
        assert ew[k] <= RTOL, f"{name} k_dynw {k}: max rel err {ew[k]:.3e}"
        assert el[k] <= RTOL, f"{name} k_dyn {k}: max rel err {el[k]:.3e}"
    # visualize's keyframe from the step's own xTrue / RotTrue, bit for bit
    want = oracle.keyframes(1.25, wave["x_true"], wave["rot_true"])
    assert np.array_equal(_bits(kf[0]), _bits(want))


# ---- coverage proof --------------------------------------------------------
COVERAGE_RUNS = ("tilt_1.4", "dense_N", "dense_unit", "models")   # tilt_1.4: the default model and covariances


def _coverage_child():
    """LQRO_DYN_PROFILE is read once per process: this runs in a fresh one,
    started with it set.  One k_dynw step per family, then the 32 counters."""
    import lqro
    import pyoracle
    L = lqro.lib()
    L.lqro_debug_dyn_profile.argtypes = [C.c_void_p, C.c_int]
    res = {}
    for name in COVERAGE_RUNS:
        cs = hard_case(name, 16)
        g, ms, per = _gains(lqro, pyoracle, cs)
        _step(lqro, 0, cs, g, ms, per)
        out = np.zeros(32, np.uint64)
        assert L.lqro_debug_dyn_profile(out.ctypes.data_as(C.c_void_p), 1) == 0
        res[name] = [int(v) for v in out]
    print("DYNPROF " + json.dumps(res))


def test_coverage_counters():
    env = dict(os.environ, LQRO_DYN_PROFILE="1", LQRO_DYN_LANE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DYNPROF ")][-1]
    prof = json.loads(line[len("DYNPROF "):])
    for name in COVERAGE_RUNS:
        assert prof[name][15] == 16, f"{name}: {prof[name][15]} agent steps counted"
    sq = {name: prof[name][23] / prof[name][15] for name in COVERAGE_RUNS}
    print(f"\nDYNCOV dense_N 6x6 rotations={prof['dense_N'][14]} dense_unit 16x16 rotations/agent="
          f"{prof['dense_unit'][12] / 16:.1f} squarings/agent models={sq['models']:.3f} default={sq['tilt_1.4']:.3f}")
    assert prof["dense_N"][14] > 0                     # jacobi<6> rotated
    assert prof["dense_unit"][12] >= 120 * 16          # jacobi<16>: a full sweep per agent
    assert sq["models"] != sq["tilt_1.4"]              # other squaring counts in expm


# ---- launch edges ----------------------------------------------------------
@pytest.fixture(scope="module")
def full65(lqro_mod, oracle):
    """65 agents on dense_mid through each kernel, once."""
    cs = hard_case("dense_mid", 65)
    g, ms, per = _gains(lqro_mod, oracle, cs)
    return cs, g, {lane: _step(lqro_mod, lane, cs, g, ms, per) for lane in (0, 1)}


@pytest.mark.parametrize("lane", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_agent_counts(lqro_mod, oracle, full65, n, lane):
    cs, g, full = full65
    got = _step(lqro_mod, lane, _head(cs, n), g, None, False)
    for k in OUT:
        assert got[k].shape[0] == n
        assert np.array_equal(_bits(got[k]), _bits(full[lane][k][:n])), f"n={n} lane={lane}: {k}"
    if n == 65:
        ref = _oracle(oracle, cs, g, None, False)
        for k, v in _errors(got, ref).items():
            assert v <= RTOL, f"n=65 lane={lane} {k}: max rel err {v:.3e}"


@pytest.mark.parametrize("lane", [0, 1])
def test_model_and_gain_switches(lqro_mod, oracle, lane):
    """n_models in {1, n} and per_agent_gains in {0, 1}, independently."""
    n = 16
    cs = hard_case("models", n)
    gb, ms, _ = _gains(lqro_mod, oracle, cs)
    g0, _ = dyn_hard.gains(oracle, dict(cs, model_ix=None))
    m0 = lqro_mod.default_model()
    shared = _step(lqro_mod, lane, cs, g0, None, False)
    runs = {"1 model, shared gains": (shared, None, g0, False)}
    runs["n models, per-agent gains"] = (_step(lqro_mod, lane, cs, gb, ms, True), ms, gb, True)
    runs["n models, shared gains"] = (_step(lqro_mod, lane, cs, g0, ms, False), ms, g0, False)
    runs["1 model, per-agent gains"] = (_step(lqro_mod, lane, cs, gb, [m0], True), [m0], gb, True)
    for what, (got, models, g, per) in runs.items():
        ref = _oracle(oracle, cs, g, models, per)
        for k, v in _errors(got, ref).items():
            assert v <= RTOL, f"{what}, lane={lane}, {k}: max rel err {v:.3e}"
    # the switches select addresses only: n copies of the one model, or of the
    # one set of gains, give the shared case's bits
    gt = {k: np.ascontiguousarray(np.broadcast_to(np.asarray(g0[k], np.float64), (n,) + np.shape(g0[k])))
          for k in dyn_hard.GAINS}
    _same(_step(lqro_mod, lane, cs, g0, [m0] * n, False), shared, "n equal models, shared gains")
    _same(_step(lqro_mod, lane, cs, gt, None, True), shared, "1 model, n equal gains")
    _same(_step(lqro_mod, lane, cs, gt, [m0] * n, True), shared, "n equal models, n equal gains")


# ---- guards: memory past agent n, read-only inputs, null outputs -------------
class _Hip:
    """Device buffers through the HIP runtime liblqro.so itself links."""

    def __init__(self):
        path = "libamdhip64.so"
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line and "/opt/rocm" in line:
                    path = line.split()[-1]
                    break
        self.h = C.CDLL(path)
        self.ptrs = []

    def put(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 8))) == 0
        self.ptrs.append(p)
        assert self.h.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    def get(self, ptr: int, like: np.ndarray) -> np.ndarray:
        out = np.empty_like(like)
        assert self.h.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    def sync(self):
        assert self.h.hipDeviceSynchronize() == 0

    def free(self):
        for p in self.ptrs:
            self.h.hipFree(p)


# Finite on purpose (about 1.07): a NaN pattern survives arithmetic, so a stray
# agent computed from a NaN tail could write the very pattern back.
SENTINEL64 = np.uint64(0x3FF123456789ABCD)
SENTINEL32 = np.uint32(0x3F8ABCDE)
TAIL = 2
WRITTEN = ("x", "rot", "x_true", "rot_true", "P", "vgoal", "u", "keyframes")


def _padded(a, n):
    """a's n agents followed by TAIL agents of the sentinel pattern."""
    dt = a.dtype
    out = np.empty((n + TAIL,) + a.shape[1:], dt)
    out.view(np.uint32 if dt == np.float32 else np.uint64)[...] = SENTINEL32 if dt == np.float32 else SENTINEL64
    out[:n] = a
    return out


def _device_step(lqro_mod, hip, lane, cs, g, n, with_outputs):
    """lqro_dynamics_step_device on buffers of n + TAIL agents; returns the
    host images before and after, by field."""
    L = lqro_mod.lib()
    st = dyn_hard.states(cs)
    host = {k: _padded(st[k], n) for k in dyn_hard.AGENT}
    host["normals"] = _padded(np.ascontiguousarray(cs["nrm"], np.float64), n)
    host["u"] = _padded(np.zeros((n, 4)), n)
    host["keyframes"] = _padded(np.zeros((n, 8), np.float32), n)
    for k in dyn_hard.GAINS:
        host[k] = np.ascontiguousarray(g[k], np.float64)
    host["M"], host["N"] = np.ascontiguousarray(cs["M"]), np.ascontiguousarray(cs["N"])
    host["model"] = np.frombuffer(bytes(lqro_mod.default_model()), dtype=np.uint8).copy()
    d = {k: hip.put(v) for k, v in host.items()}
    a = lqro_mod.Agents(*[d[k] for k in dyn_hard.STATE], d["u"] if with_outputs else None, d["u_goal"],
                        d["p_goal"], *[d[k] for k in dyn_hard.GAINS], d["M"], d["N"], d["normals"],
                        d["keyframes"] if with_outputs else None)
    a.time = 0.5
    with _kernel(lane):
        rc = L.lqro_dynamics_step_device(C.c_void_p(d["model"]), 1, n, 0, C.byref(a), None)
    assert rc == 0
    hip.sync()
    return host, {k: hip.get(d[k], host[k]) for k in host}


@pytest.mark.parametrize("lane", [0, 1])
@pytest.mark.parametrize("n", [1, 65])
def test_guards(lqro_mod, oracle, full65, n, lane):
    cs, g, full = full65
    cs = _head(cs, n)
    hip = _Hip()
    try:
        before, after = _device_step(lqro_mod, hip, lane, cs, g, n, True)
        _, quiet = _device_step(lqro_mod, hip, lane, cs, g, n, False)
    finally:
        hip.free()
    for k in WRITTEN:      # agents n, n + 1: left alone
        assert np.array_equal(_bits(after[k][n:]), _bits(before[k][n:])), f"{k}: written past agent {n}"
        assert np.array_equal(_bits(quiet[k][n:]), _bits(before[k][n:])), f"{k}: written past agent {n}"
    for k in before:       # read-only inputs: unchanged, tails included
        if k not in WRITTEN:
            assert np.array_equal(_bits(after[k]), _bits(before[k])), f"{k}: input changed"
            assert np.array_equal(_bits(quiet[k]), _bits(before[k])), f"{k}: input changed"
    for k in dyn_hard.STATE:
        # the device entry point computes what lqro_dynamics_step does ...
        assert np.array_equal(_bits(after[k][:n]), _bits(full[lane][k][:n])), k
        # ... with or without u and keyframes
        assert np.array_equal(_bits(quiet[k]), _bits(after[k])), f"{k}: differs with u = keyframes = NULL"
    assert np.array_equal(_bits(after["u"][:n]), _bits(full[lane]["u"][:n]))
    want = oracle.keyframes(0.5, after["x_true"][:n], after["rot_true"][:n])
    assert np.array_equal(_bits(after["keyframes"][:n]), _bits(want))
    for k in ("u", "keyframes"):   # null outputs: nothing written at all
        assert np.array_equal(_bits(quiet[k]), _bits(before[k])), k


# ---- arguments -------------------------------------------------------------
BAD_ARGS = {
    "n = 0": dict(n=0),
    "n_models = 2 with n = 3": dict(n_models=2),
    "models = NULL": dict(models=None),
    "agents = NULL": dict(agents=None),
    "P = NULL": dict(null="P"),
    "normals = NULL": dict(null="normals"),
    "Lh = NULL": dict(null="Lh"),
}


ORDER = ("x", "rot", "x_true", "rot_true", "P", "vgoal", "u", "u_goal", "p_goal",
         "L", "E", "l", "Lh", "Eh", "M", "N", "normals")


@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_bad_arguments(lqro_mod, oracle, what):
    """LQRO_E_ARG from both entry points (host arrays for lqro_dynamics_step,
    device buffers for lqro_dynamics_step_device), the state arrays untouched."""
    L = lqro_mod.lib()
    n = 3
    bad = BAD_ARGS[what]
    cs = hard_case("dense_mid", n)
    g, _ = dyn_hard.gains(oracle, cs)
    host = dyn_hard.states(cs)
    host.update({k: np.ascontiguousarray(v, np.float64) for k, v in
                 dict(g, M=cs["M"], N=cs["N"], normals=cs["nrm"]).items() if k in ORDER})
    host["u"] = np.zeros((n, 4))
    before = {k: v.copy() for k, v in host.items()}
    models = (lqro_mod.Model * 3)(*[lqro_mod.default_model()] * 3)   # (three, so that index 2 exists)
    n_models, n_arg = bad.get("n_models", 1), bad.get("n", n)
    hip = _Hip()
    try:
        dev = {k: hip.put(v) for k, v in host.items()}
        dev_models = hip.put(np.frombuffer(bytes(models), dtype=np.uint8))
        rcs = []
        for ptrs, marg, fn in ((({k: v.ctypes.data_as(C.c_void_p).value for k, v in host.items()}), models,
                                lambda m, a: L.lqro_dynamics_step(m, n_models, n_arg, 0, a, 0)),
                               (dev, C.c_void_p(dev_models),
                                lambda m, a: L.lqro_dynamics_step_device(m, n_models, n_arg, 0, a, None))):
            ptrs = dict(ptrs)
            if "null" in bad:
                ptrs[bad["null"]] = None
            a = lqro_mod.Agents(*[ptrs[k] for k in ORDER], None)
            rcs.append(fn(None if "models" in bad else marg, None if "agents" in bad else C.byref(a)))
        hip.sync()
        after_dev = {k: hip.get(dev[k], host[k]) for k in host}
    finally:
        hip.free()
    assert rcs == [LQRO_E_ARG, LQRO_E_ARG], rcs
    for k in host:
        assert np.array_equal(_bits(host[k]), _bits(before[k])), k
        assert np.array_equal(_bits(after_dev[k]), _bits(before[k])), k


if __name__ == "__main__":
    _coverage_child()
