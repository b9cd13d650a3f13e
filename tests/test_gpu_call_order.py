"""What each entry point of liblqro.so returns around a half-step.

lqro_step_device_begin leaves the context `pending` until lqro_step_device_end:
the half-step still reads the tables, the plane buffers and the counters, so
the setters, the getters and the steps refuse (LQRO_E_STATE) without touching
the device, argument errors still come first (LQRO_E_ARG), and the four
diagnostic hooks that never looked at `pending` still answer.  Recorded from
the library as it was before its runtime file was split; one tiny context
(N = 8, H = 20, NP = 30, default flags: Qhull order), raw C-ABI calls.

lqro_get_records needs LQRO_FLAG_RECORDS (without it: LQRO_E_STATE at any
time), so the second context, the one that first shows what a context without
gains returns, has that flag and pins lqro_get_records around a half-step of
its own.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE = 0, -1, -4
N, H, NP = 8, 20, 30


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _Calls:
    """The entry points on one context, each with arguments that succeed on an
    idle context and leave its results as they were."""

    def __init__(self, lqro_mod, ctx, gains, d_x, d_vg, d_tab, d_nv):
        self.L, self.h = lqro_mod.lib(), ctx._h
        self.g = [np.ascontiguousarray(gains[k], dtype=np.float64) for k in "ABLE"]
        self.dev = [C.c_void_p(v) for v in (d_x, d_vg, d_tab, d_nv)]
        self.x, self.vg = lqro_mod.synthetic_swarm(N)
        self.i64, self.f64 = np.zeros(4 * 16384, np.int64), np.zeros(3 * N)
        self.u64 = np.zeros(4 * 4096, np.uint64)
        self.n = C.c_int64()
        self.recs = np.zeros(N * (N - 1), dtype=lqro_mod.RECORD_DTYPE)

    def refused_while_pending(self):
        L, h, n = self.L, self.h, C.byref(self.n)
        d_x, d_vg, d_tab, d_nv = self.dev
        return {
            "lqro_set_neighbors": lambda: L.lqro_set_neighbors(h, 0.0, 0),
            "lqro_set_user_planes": lambda: L.lqro_set_user_planes(h, None, None),
            "lqro_set_user_planes_device": lambda: L.lqro_set_user_planes_device(h, None, 0, None),
            "lqro_set_fence": lambda: L.lqro_set_fence(h, None, None, 0.0),
            "lqro_set_gains": lambda: L.lqro_set_gains(h, *[_p(v) for v in self.g], 0),
            "lqro_get_carry_normal": lambda: L.lqro_get_carry_normal(h, _p(self.f64)),
            "lqro_set_carry_normal": lambda: L.lqro_set_carry_normal(h, _p(self.f64)),   # (what get just read)
            "lqro_get_stats": lambda: L.lqro_get_stats(h, _p(self.i64)),
            "lqro_get_stats_ex": lambda: L.lqro_get_stats_ex(h, _p(self.i64), 12),
            "lqro_get_hull_builds": lambda: L.lqro_get_hull_builds(h, _p(self.i64), C.c_int64(64), n),
            "lqro_get_hull_failures": lambda: L.lqro_get_hull_failures(h, _p(self.i64), 64, n),
            "lqro_get_qhmerge_pairs": lambda: L.lqro_get_qhmerge_pairs(h, _p(self.i64), 64, n),
            "lqro_step": lambda: L.lqro_step(h, _p(self.x), _p(self.vg), _p(self.f64)),
            "lqro_step_device": lambda: L.lqro_step_device(h, d_x, d_vg, d_nv, None),
        }

    def begin(self):
        d_x, d_vg, d_tab, _ = self.dev
        return self.L.lqro_step_device_begin(self.h, d_x, d_vg, d_tab, None)

    def end(self):
        return self.L.lqro_step_device_end(self.h, self.dev[2], self.dev[3], None)

    def records(self):
        return self.L.lqro_get_records(self.h, _p(self.recs), len(self.recs), C.byref(self.n))

    def null_arguments(self):
        L, h = self.L, self.h
        d_x, d_vg, d_tab, d_nv = self.dev
        return {
            "lqro_set_neighbors(NULL)": lambda: L.lqro_set_neighbors(None, 1.0, 4),
            "lqro_set_fence(NULL)": lambda: L.lqro_set_fence(None, None, None, 0.0),
            "lqro_set_gains(A = NULL)": lambda: L.lqro_set_gains(h, None, *[_p(v) for v in self.g[1:]], 0),
            "lqro_get_carry_normal(out = NULL)": lambda: L.lqro_get_carry_normal(h, None),
            "lqro_set_carry_normal(NULL)": lambda: L.lqro_set_carry_normal(None, _p(self.f64)),
            "lqro_get_stats(out = NULL)": lambda: L.lqro_get_stats(h, None),
            "lqro_get_stats_ex(NULL)": lambda: L.lqro_get_stats_ex(None, _p(self.i64), 12),
            "lqro_get_records(out = NULL)": lambda: L.lqro_get_records(h, None, 0, None),
            "lqro_get_hull_builds(n_out = NULL)": lambda: L.lqro_get_hull_builds(h, _p(self.i64), C.c_int64(4), None),
            "lqro_get_hull_failures(n_out = NULL)": lambda: L.lqro_get_hull_failures(h, _p(self.i64), 64, None),
            "lqro_step(newv = NULL)": lambda: L.lqro_step(h, _p(self.x), _p(self.vg), None),
            "lqro_step_device(d_newv = NULL)": lambda: L.lqro_step_device(h, d_x, d_vg, None, None),
            "lqro_step_device_begin(d_x = NULL)": lambda: L.lqro_step_device_begin(h, None, d_vg, d_tab, None),
            "lqro_step_device_end(d_newv = NULL)": lambda: L.lqro_step_device_end(h, d_tab, None, None),
        }

    def hooks(self):
        """Not in lqro.h, bound by name; they never look at `pending`."""
        L, h = self.L, self.h
        big = np.zeros(16384, np.uint64)
        return {
            "lqro_debug_prof_words": lambda: L.lqro_debug_prof_words(h, C.c_int64(0), C.c_int64(32), _p(self.u64)),
            "lqro_debug_local_hull": lambda: L.lqro_debug_local_hull(h, _p(self.i64)),
            "lqro_debug_local_hull_jobs": lambda: L.lqro_debug_local_hull_jobs(h, _p(self.u64)),
            "lqro_debug_hull_profile": lambda: L.lqro_debug_hull_profile(h, _p(big)),
        }


def _all(calls, want):
    got = {name: f() for name, f in calls.items()}
    assert got == {name: want for name in calls}, {k: v for k, v in got.items() if v != want}


def test_status_around_a_half_step(lqro_mod, gains):
    from test_gpu_dyn import _Hip   # device buffers through liblqro's own HIP runtime
    x, vg = lqro_mod.synthetic_swarm(N)
    ctx = lqro_mod.Context(lqro_mod.config(N, H, NP))
    assert ctx.cfg.flags == lqro_mod.LQRO_FLAG_QHULL_ORDER
    rctx = lqro_mod.Context(lqro_mod.config(N, H, NP,
                                            flags=lqro_mod.LQRO_FLAG_QHULL_ORDER | lqro_mod.LQRO_FLAG_RECORDS))
    hip = _Hip()
    zt, zv = np.zeros((N, 4)), np.zeros((N, 3))
    d_x, d_vg = hip.put(x), hip.put(vg)
    d_tab, d_nv, d_ref = hip.put(zt), hip.put(zv), hip.put(zv)
    r_tab, r_nv = hip.put(zt), hip.put(zv)
    try:
        ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
        c = _Calls(lqro_mod, ctx, gains, d_x, d_vg, d_tab, d_nv)
        r = _Calls(lqro_mod, rctx, gains, d_x, d_vg, r_tab, r_nv)
        # a fresh context: the getters that wait for the last step have nothing to wait for
        assert c.L.lqro_get_stats(c.h, _p(c.i64)) == OK
        assert c.L.lqro_get_carry_normal(c.h, _p(c.f64)) == OK
        assert c.end() == E_STATE                                   # no begin
        # no gains: no step of any kind
        assert r.L.lqro_step(r.h, _p(r.x), _p(r.vg), _p(r.f64)) == E_STATE
        assert r.L.lqro_step_device(r.h, *r.dev[:2], r.dev[3], None) == E_STATE
        assert r.begin() == E_STATE
        rctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
        # the reference: one plain step of the same inputs from the same carried normal
        ctx.carry_normal(np.zeros(3))
        ctx.step_device(d_x, d_vg, d_ref, 0)
        hip.sync()
        want = hip.get(d_ref, zv)
        ctx.carry_normal(np.zeros(3))
        # pending
        assert c.begin() == OK
        _all(c.refused_while_pending(), E_STATE)
        assert c.begin() == E_STATE                                 # a second begin
        _all(c.null_arguments(), E_ARG)
        _all(c.hooks(), OK)
        assert r.begin() == OK
        assert r.records() == E_STATE
        # after _end
        assert c.end() == OK
        hip.sync()
        got = hip.get(d_nv, zv)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert np.abs(got).max() > 0
        assert r.end() == OK
        assert r.records() == OK and r.n.value == N * (N - 1)
        assert c.records() == E_STATE                               # no LQRO_FLAG_RECORDS: never
        _all(c.refused_while_pending(), OK)
        _all(c.hooks(), OK)
        t = np.zeros(4, np.float32)
        assert c.L.lqro_get_timings(c.h, _p(t)) == OK
        assert c.begin() == OK and c.end() == OK
        hip.sync()
    finally:
        ctx.close()
        rctx.close()
        hip.free()
