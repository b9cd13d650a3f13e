"""lqro — Python host binding of liblqro.so (the MI355X LQR-Obstacle step).

This module mirrors the reference simulator's interface for the pair loop
(hihixuyang/LQR-Obstacles, QuadrotorHoverController/LQRObstacles.cpp, "LQRO"):

  * ``Quadrotor``  — the agent record the loop reads and writes (LQRO:73-165:
    ``x``, ``L``, ``E``, ``vGoal``, ``newV``);
  * ``Simulator.findMatrices()`` — controlMatrices at hover (LQRO:520-582,
    called per agent at LQRO:1370-1373);
  * ``Simulator.step()`` — the pair loop LQRO:1393-1436: every ordered pair's
    LQR-Obstacle, its half-plane, and each agent's new velocity
    (calculateNewV, LQRO:1435), computed by the HIP kernels.

All numerics run in liblqro.so (HIP for gfx950).  There is no CPU fallback:
if the library or a gfx950 device is missing, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblqro.so")

LQRO_OK = 0
LQRO_E_HULL = -8              # an inside-hull pair's hull could not be built (degenerate input or capacity; no half-plane)
LQRO_E_QHMERGE = -9           # the step ran, but a pair's winning facet may be one qconvex's pre-merge joins
LQRO_FLAG_RECORDS = 0x1
LQRO_FLAG_QHULL_ORDER = 0x2   # the reference's own hull rule over Qhull's build order (k_qhull)
REC_PLANE, REC_INSIDE, REC_BACKUP, REC_HULL, REC_HULLFAIL, REC_LOCAL = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
REC_STALE, REC_QHMERGE = 0x40, 0x80
REC_QHMERGE_WIN = 0x100       # with REC_QHMERGE: qconvex's pre-merge may have merged the winning facet
HULL_BUILD_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("n_points", np.int32), ("insertions", np.int32),
                             ("facet_slots", np.int32), ("kernel", np.int32), ("t_start", np.uint64),
                             ("t_end", np.uint64)])


class Config(C.Structure):
    _fields_ = [
        ("n_agents", C.c_int32), ("x_dim", C.c_int32), ("u_dim", C.c_int32),
        ("horizon", C.c_int32), ("n_points", C.c_int32), ("min_reach", C.c_int32),
        ("xy_radius", C.c_double), ("z_radius", C.c_double),
        ("vmax_reach", C.c_double), ("vmax_lp", C.c_double),
        ("row_begin", C.c_int32), ("row_end", C.c_int32),
        ("device", C.c_int32), ("flags", C.c_int32), ("row_stride", C.c_int32),
    ]


class Model(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "dt", "gravity", "mass", "inertia", "moment_const", "thrust_latency", "length",
        "j_step", "qv", "qp", "r", "pos_weight")]


class PairRecord(C.Structure):
    _fields_ = [
        ("i", C.c_int32), ("j", C.c_int32), ("n_reach", C.c_int32), ("flags", C.c_int32),
        ("gjk_iters", C.c_int32), ("simplex_n", C.c_int32), ("simplex", C.c_int32 * 4),
        ("facet", C.c_int32 * 3), ("n_facets", C.c_int32), ("reach_hash", C.c_uint64),
        ("dist", C.c_double), ("normal", C.c_double * 3), ("wpt_vrel", C.c_double * 3),
        ("wpt_hull", C.c_double * 3), ("plane_point", C.c_float * 3),
        ("plane_normal", C.c_float * 3),
    ]


RECORD_DTYPE = np.dtype([
    ("i", "<i4"), ("j", "<i4"), ("n_reach", "<i4"), ("flags", "<i4"), ("gjk_iters", "<i4"),
    ("simplex_n", "<i4"), ("simplex", "<i4", (4,)), ("facet", "<i4", (3,)),
    ("n_facets", "<i4"), ("reach_hash", "<u8"), ("dist", "<f8"), ("normal", "<f8", (3,)),
    ("wpt_vrel", "<f8", (3,)), ("wpt_hull", "<f8", (3,)), ("plane_point", "<f4", (3,)),
    ("plane_normal", "<f4", (3,)),
])
assert RECORD_DTYPE.itemsize == C.sizeof(PairRecord) == 168

class ClearanceRow(C.Structure):
    """lqro_clearance_row: one own row's separation from every column."""
    _fields_ = [("s2_min", C.c_double), ("d2_min", C.c_double), ("fence_min", C.c_double),
                ("j_s2", C.c_int32), ("j_d2", C.c_int32), ("n_hit", C.c_int32), ("fence_face", C.c_int32),
                ("hit", C.c_int32 * 6)]


class ClearanceTotal(C.Structure):
    """lqro_clearance_total: the minima and counts over a context's own rows."""
    _fields_ = [("s2_min", C.c_double), ("d2_min", C.c_double), ("fence_min", C.c_double),
                ("s2_i", C.c_int32), ("s2_j", C.c_int32), ("d2_i", C.c_int32), ("d2_j", C.c_int32),
                ("fence_i", C.c_int32), ("fence_face", C.c_int32),
                ("n_hit", C.c_int64), ("n_rows_hit", C.c_int64), ("n_fence_out", C.c_int64),
                ("n_measured", C.c_int64)]


CLEARANCE_ROW_DTYPE = np.dtype([("s2_min", "<f8"), ("d2_min", "<f8"), ("fence_min", "<f8"), ("j_s2", "<i4"),
                                ("j_d2", "<i4"), ("n_hit", "<i4"), ("fence_face", "<i4"), ("hit", "<i4", (6,))])
assert CLEARANCE_ROW_DTYPE.itemsize == C.sizeof(ClearanceRow) == 64 and C.sizeof(ClearanceTotal) == 80
CLEARANCE_TOTAL_FIELDS = tuple(n for n, _ in ClearanceTotal._fields_)


def _total_dict(t: ClearanceTotal) -> dict:
    return {n: getattr(t, n) for n in CLEARANCE_TOTAL_FIELDS}


def merge_clearance(totals) -> dict:
    """The ranks' totals of one measurement (or of the same measurements since
    a reset) as one: each minimum is the smallest (value, i, j) over the
    shards (a +inf minimum has indices -1), the counts are summed, n_measured
    is the shards' common count (its largest).  Row shards partition the rows,
    so the merge of a block or cyclic split equals the single context's
    total."""
    totals = list(totals)
    out = dict(s2_min=np.inf, s2_i=-1, s2_j=-1, d2_min=np.inf, d2_i=-1, d2_j=-1, fence_min=np.inf, fence_i=-1,
               fence_face=-1, n_hit=0, n_rows_hit=0, n_fence_out=0, n_measured=0)
    for v, a, b in (("s2_min", "s2_i", "s2_j"), ("d2_min", "d2_i", "d2_j"), ("fence_min", "fence_i", "fence_face")):
        keys = [(float(t[v]), int(t[a]), int(t[b])) for t in totals if float(t[v]) < np.inf]
        if keys:
            out[v], out[a], out[b] = min(keys)
    for k in ("n_hit", "n_rows_hit", "n_fence_out"):
        out[k] = sum(int(t[k]) for t in totals)
    out["n_measured"] = max([int(t["n_measured"]) for t in totals], default=0)
    return out


class PredictRow(C.Structure):
    """lqro_predict_row: one own row's predicted separation over the horizon."""
    _fields_ = [("s2_min", C.c_double), ("d2_min", C.c_double),
                ("j_s2", C.c_int32), ("k_s2", C.c_int32), ("j_d2", C.c_int32), ("k_d2", C.c_int32),
                ("k_first", C.c_int32), ("j_first", C.c_int32), ("n_conf", C.c_int32), ("reserved", C.c_int32),
                ("conf", C.c_int32 * 4)]


class PredictTotal(C.Structure):
    """lqro_predict_total: the minima, the first hit and the counts over a context's own rows."""
    _fields_ = [("s2_min", C.c_double), ("d2_min", C.c_double),
                ("s2_i", C.c_int32), ("s2_j", C.c_int32), ("s2_k", C.c_int32),
                ("d2_i", C.c_int32), ("d2_j", C.c_int32), ("d2_k", C.c_int32),
                ("first_k", C.c_int32), ("first_i", C.c_int32), ("first_j", C.c_int32), ("reserved", C.c_int32),
                ("n_conf", C.c_int64), ("n_rows_conf", C.c_int64), ("n_measured", C.c_int64)]


PREDICT_ROW_DTYPE = np.dtype([("s2_min", "<f8"), ("d2_min", "<f8"), ("j_s2", "<i4"), ("k_s2", "<i4"), ("j_d2", "<i4"),
                              ("k_d2", "<i4"), ("k_first", "<i4"), ("j_first", "<i4"), ("n_conf", "<i4"),
                              ("reserved", "<i4"), ("conf", "<i4", (4,))])
assert PREDICT_ROW_DTYPE.itemsize == C.sizeof(PredictRow) == 64 and C.sizeof(PredictTotal) == 80
PREDICT_TOTAL_FIELDS = tuple(n for n, _ in PredictTotal._fields_)
PREDICT_TILE = 8   # LQRO_PREDICT_TILE: own rows a workgroup of k_conf


def _predict_total_dict(t: PredictTotal) -> dict:
    return {n: getattr(t, n) for n in PREDICT_TOTAL_FIELDS}


def merge_prediction(totals) -> dict:
    """The ranks' totals of one prediction (or of the same predictions since a
    reset) as one: each minimum is the smallest (value, i, j, k) over the
    shards (a +inf minimum has indices -1), the first hit the smallest
    (k, i, j), the counts are summed, n_measured is the shards' common count
    (its largest).  Row shards partition the rows, so the merge of a block or
    cyclic split equals the single context's total of one prediction."""
    totals = list(totals)
    out = dict(s2_min=np.inf, d2_min=np.inf, s2_i=-1, s2_j=-1, s2_k=-1, d2_i=-1, d2_j=-1, d2_k=-1, first_k=-1,
               first_i=-1, first_j=-1, reserved=0, n_conf=0, n_rows_conf=0, n_measured=0)
    for v in ("s2", "d2"):
        keys = [(float(t[v + "_min"]), int(t[v + "_i"]), int(t[v + "_j"]), int(t[v + "_k"])) for t in totals
                if float(t[v + "_min"]) < np.inf]
        if keys:
            out[v + "_min"], out[v + "_i"], out[v + "_j"], out[v + "_k"] = min(keys)
    keys = [(int(t["first_k"]), int(t["first_i"]), int(t["first_j"])) for t in totals if int(t["first_k"]) >= 0]
    if keys:
        out["first_k"], out["first_i"], out["first_j"] = min(keys)
    for k in ("n_conf", "n_rows_conf"):
        out[k] = sum(int(t[k]) for t in totals)
    out["n_measured"] = max([int(t["n_measured"]) for t in totals], default=0)
    return out


class LpRow(C.Structure):
    """lqro_lp_row: one own row's result against the plane list its LP saw."""
    _fields_ = [("viol_max", C.c_float), ("hard_viol_max", C.c_float), ("v2", C.c_float), ("dv2", C.c_float),
                ("i", C.c_int32), ("m", C.c_int32), ("n_hard", C.c_int32), ("n_viol", C.c_int32),
                ("n_viol_tol", C.c_int32), ("n_hard_viol", C.c_int32),
                ("k_viol", C.c_int32), ("kind_viol", C.c_int32), ("id_viol", C.c_int32),
                ("k_hard", C.c_int32), ("kind_hard", C.c_int32), ("id_hard", C.c_int32)]


class LpTotal(C.Structure):
    """lqro_lp_total: the maxima and counts over a context's own rows."""
    _fields_ = [("viol_max", C.c_float), ("viol_i", C.c_int32), ("viol_k", C.c_int32), ("viol_kind", C.c_int32),
                ("viol_id", C.c_int32),
                ("hard_viol_max", C.c_float), ("hard_i", C.c_int32), ("hard_k", C.c_int32), ("hard_kind", C.c_int32),
                ("hard_id", C.c_int32),
                ("dv2_max", C.c_float), ("dv2_i", C.c_int32),
                ("n_rows_viol", C.c_int64), ("n_rows_hard_viol", C.c_int64), ("n_viol_tol", C.c_int64),
                ("n_planes", C.c_int64), ("n_measured", C.c_int64)]


LP_ROW_DTYPE = np.dtype([("viol_max", "<f4"), ("hard_viol_max", "<f4"), ("v2", "<f4"), ("dv2", "<f4"),
                         ("i", "<i4"), ("m", "<i4"), ("n_hard", "<i4"), ("n_viol", "<i4"), ("n_viol_tol", "<i4"),
                         ("n_hard_viol", "<i4"), ("k_viol", "<i4"), ("kind_viol", "<i4"), ("id_viol", "<i4"),
                         ("k_hard", "<i4"), ("kind_hard", "<i4"), ("id_hard", "<i4")])
assert LP_ROW_DTYPE.itemsize == C.sizeof(LpRow) == 64 and C.sizeof(LpTotal) == 88
LP_TOTAL_FIELDS = tuple(n for n, _ in LpTotal._fields_)
# a plane's source in an LP audit record (lqro.h)
LQRO_AUDIT_FENCE, LQRO_AUDIT_USER, LQRO_AUDIT_COLUMN = 0, 1, 2
RVO_EPSILON = 0.00001   # the tolerance the docs suggest for set_lp_audit


def _lp_total_dict(t: LpTotal) -> dict:
    return {n: getattr(t, n) for n in LP_TOTAL_FIELDS}


_LP_MAXIMA = (("viol_max", ("viol_i", "viol_k", "viol_kind", "viol_id")),
              ("hard_viol_max", ("hard_i", "hard_k", "hard_kind", "hard_id")),
              ("dv2_max", ("dv2_i",)))
_LP_COUNTS = ("n_rows_viol", "n_rows_hard_viol", "n_viol_tol", "n_planes")


def merge_lp_audit(totals) -> dict:
    """The ranks' totals of one audit (or of the same audits since a reset) as
    one: each maximum is decided by the largest value, then the smallest i,
    then the smallest k over the shards (a -inf maximum has indices -1), the
    counts are summed, n_measured is the shards' common count (its largest).
    Row shards partition the rows, so the merge of a block or cyclic split
    equals the single context's total of one audit."""
    totals = list(totals)
    out = {n: (0 if n.startswith("n_") else -1) for n in LP_TOTAL_FIELDS}
    for v, idx in _LP_MAXIMA:
        out[v] = np.float32(-np.inf)
        best = None
        for t in totals:
            val = np.float32(t[v])
            if not val > -np.inf:
                continue
            key = (int(t[idx[0]]), int(t[idx[1]]) if len(idx) > 1 else 0)
            if best is None or val > best[0] or (val == best[0] and key < best[1]):
                best = (val, key, t)
        if best is not None:
            out[v] = best[0]
            for n in idx:
                out[n] = int(best[2][n])
    for k in _LP_COUNTS:
        out[k] = sum(int(t[k]) for t in totals)
    out["n_measured"] = max([int(t["n_measured"]) for t in totals], default=0)
    return out


# every symbol include/lqro.h declares
EXPORTS = (
    "lqro_config_default", "lqro_model_default", "lqro_synthesize_gains", "lqro_sphere",
    "lqro_create", "lqro_destroy", "lqro_set_gains", "lqro_step", "lqro_step_device",
    "lqro_get_records", "lqro_get_stats", "lqro_get_timings", "lqro_status_string",
    "lqro_version", "lqro_calculate_new_v", "lqro_synthesize_gains_batch",
    "lqro_dynamics_step", "lqro_dynamics_step_device", "lqro_normals", "lqro_set_neighbors",
    "lqro_synthesize_gains_x", "lqro_synthesize_gains_batch_x",
    "lqro_set_carry_normal", "lqro_get_carry_normal",
    "lqro_step_device_begin", "lqro_step_device_end",
    "lqro_get_stats_ex", "lqro_get_hull_failures", "lqro_get_hull_builds", "lqro_get_qhmerge_pairs",
    "lqro_set_user_planes", "lqro_set_user_planes_device", "lqro_set_fence",
    "lqro_set_obstacles", "lqro_set_obstacles_device",
    "lqro_set_obstacles_ex", "lqro_set_obstacles_ex_device",
    "lqro_set_hard_planes", "lqro_calculate_new_v_hard",
    "lqro_clearance", "lqro_clearance_device", "lqro_set_monitor", "lqro_get_monitor",
    "lqro_get_monitor_rows", "lqro_get_monitor_pairs",
    "lqro_set_lp_audit", "lqro_get_lp_audit", "lqro_get_lp_audit_rows", "lqro_audit_new_v",
    "lqro_set_active", "lqro_set_active_device",
    "lqro_set_interaction", "lqro_set_interaction_device",
    "lqro_predict", "lqro_predict_device", "lqro_predict_paths", "lqro_predict_paths_device",
    "lqro_get_prediction", "lqro_get_prediction_rows", "lqro_get_paths",
)
# lqro_set_hard_planes' levels: the planes linearProgram4 does not relax
LQRO_HARD_NONE, LQRO_HARD_FENCE, LQRO_HARD_HEAD, LQRO_HARD_OBSTACLES = 0, 1, 2, 3
LQRO_CLASSES_MAX = 16   # lqro_set_interaction's classes

NORMALS_PER_AGENT = 22   # LQRO_NORMALS_PER_AGENT: 16 propagate + 6 observation


class Agents(C.Structure):
    """lqro_agents: per-agent state, gains and noise of the step after the
    pair loop (LQRO:1437-1446)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "x", "rot", "x_true", "rot_true", "P", "vgoal", "u", "u_goal", "p_goal",
        "L", "E", "l", "Lh", "Eh", "M", "N", "normals", "keyframes")] + [("time", C.c_double)]

_lib = None


def lib() -> C.CDLL:
    """Load liblqro.so (raises if it was not built: no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"liblqro.so not built at {LIB_PATH}; run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.lqro_status_string.restype = C.c_char_p
        L.lqro_config_default.argtypes = [C.POINTER(Config), i32, i32, i32]
        L.lqro_model_default.argtypes = [C.POINTER(Model)]
        L.lqro_synthesize_gains.argtypes = [C.POINTER(Model)] + [vp] * 7
        L.lqro_synthesize_gains_batch.argtypes = [C.POINTER(Model), i32] + [vp] * 7 + [i32]
        L.lqro_synthesize_gains_x.argtypes = [C.POINTER(Model), i32] + [vp] * 8
        L.lqro_synthesize_gains_batch_x.argtypes = [C.POINTER(Model), i32, i32] + [vp] * 8 + [i32]
        L.lqro_sphere.argtypes = [i32, dbl, dbl, vp]
        L.lqro_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.lqro_destroy.argtypes = [vp]
        L.lqro_destroy.restype = None
        L.lqro_set_gains.argtypes = [vp, vp, vp, vp, vp, i32]
        L.lqro_step.argtypes = [vp, vp, vp, vp]
        L.lqro_step_device.argtypes = [vp, vp, vp, vp, vp]
        L.lqro_step_device_begin.argtypes = [vp, vp, vp, vp, vp]
        L.lqro_step_device_end.argtypes = [vp, vp, vp, vp]
        L.lqro_get_records.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.lqro_get_stats.argtypes = [vp, vp]
        L.lqro_get_stats_ex.argtypes = [vp, vp, i32]
        L.lqro_get_hull_failures.argtypes = [vp, vp, i64, C.POINTER(i64)]
        if hasattr(L, "lqro_get_qhmerge_pairs"):   # (older libraries in A/B runs lack it)
            L.lqro_get_qhmerge_pairs.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.lqro_get_timings.argtypes = [vp, vp]
        L.lqro_calculate_new_v.argtypes = [vp, vp, i32, vp, dbl, vp, i32]
        L.lqro_dynamics_step.argtypes = [C.POINTER(Model), i32, i32, i32, C.POINTER(Agents), i32]
        L.lqro_dynamics_step_device.argtypes = [vp, i32, i32, i32, C.POINTER(Agents), vp]
        L.lqro_normals.argtypes = [C.POINTER(C.c_uint32), i64, vp]
        L.lqro_set_neighbors.argtypes = [vp, dbl, i32]
        L.lqro_set_user_planes.argtypes = [vp, vp, vp]
        L.lqro_set_user_planes_device.argtypes = [vp, vp, i32, vp]
        L.lqro_set_fence.argtypes = [vp, vp, vp, dbl]
        if hasattr(L, "lqro_set_obstacles"):   # (older libraries in A/B runs lack them)
            L.lqro_set_obstacles.argtypes = [vp, vp, i32, dbl, dbl, dbl]
            L.lqro_set_obstacles_device.argtypes = [vp, vp, i32, dbl, dbl, dbl]
        if hasattr(L, "lqro_set_obstacles_ex"):
            L.lqro_set_obstacles_ex.argtypes = [vp, vp, i32, vp, vp, vp]
            L.lqro_set_obstacles_ex_device.argtypes = [vp, vp, i32, vp, vp, vp]
        if hasattr(L, "lqro_set_hard_planes"):   # (older libraries in A/B runs lack them)
            L.lqro_set_hard_planes.argtypes = [vp, i32]
            L.lqro_calculate_new_v_hard.argtypes = [vp, vp, vp, i32, vp, dbl, vp, i32]
        if hasattr(L, "lqro_clearance"):   # (older libraries in A/B runs lack them)
            L.lqro_clearance.argtypes = [vp, vp, vp, C.POINTER(ClearanceTotal)]
            L.lqro_clearance_device.argtypes = [vp, vp, vp, vp]
            L.lqro_set_monitor.argtypes = [vp, i32]
            L.lqro_get_monitor.argtypes = [vp, C.POINTER(ClearanceTotal), C.POINTER(ClearanceTotal), i32]
            L.lqro_get_monitor_rows.argtypes = [vp, vp, i64, C.POINTER(i64)]
            L.lqro_get_monitor_pairs.argtypes = [vp, vp, i64, C.POINTER(i64)]
        if hasattr(L, "lqro_set_lp_audit"):   # (older libraries in A/B runs lack them)
            L.lqro_set_lp_audit.argtypes = [vp, i32, C.c_float]
            L.lqro_get_lp_audit.argtypes = [vp, C.POINTER(LpTotal), C.POINTER(LpTotal), i32]
            L.lqro_get_lp_audit_rows.argtypes = [vp, vp, i64, C.POINTER(i64)]
            L.lqro_audit_new_v.argtypes = [vp, vp, vp, i32, vp, vp, C.c_float, vp, C.POINTER(LpTotal), i32]
        if hasattr(L, "lqro_set_active"):   # (older libraries in A/B runs lack them)
            L.lqro_set_active.argtypes = [vp, vp]
            L.lqro_set_active_device.argtypes = [vp, vp]
        if hasattr(L, "lqro_set_interaction"):   # (as above)
            L.lqro_set_interaction.argtypes = [vp, vp, i32, vp]
            L.lqro_set_interaction_device.argtypes = [vp, vp, i32, vp]
        if hasattr(L, "lqro_predict"):   # (older libraries in A/B runs lack them)
            L.lqro_predict.argtypes = [vp, vp, vp, vp, C.POINTER(PredictTotal)]
            L.lqro_predict_device.argtypes = [vp, vp, vp, vp, vp]
            L.lqro_predict_paths.argtypes = [vp, vp, vp, C.POINTER(PredictTotal)]
            L.lqro_predict_paths_device.argtypes = [vp, vp, vp, vp]
            L.lqro_get_prediction.argtypes = [vp, C.POINTER(PredictTotal), C.POINTER(PredictTotal), i32]
            L.lqro_get_prediction_rows.argtypes = [vp, vp, i64, C.POINTER(i64)]
            L.lqro_get_paths.argtypes = [vp, vp]
        L.lqro_set_carry_normal.argtypes = [vp, vp]
        L.lqro_get_carry_normal.argtypes = [vp, vp]
        _lib = L
    return _lib


class LqroError(RuntimeError):
    pass


class HullFailure(LqroError):
    """lqro_step returned LQRO_E_HULL: inside-hull pairs whose hull could not
    be built (degenerate or too few points, or every hull kernel's capacity
    exceeded) got no half-plane (the reference's qconvex
    always returns a hull, LQRO:879-880).  .pairs: their (i, j); .newv: the
    step's new velocities, computed without those planes."""

    def __init__(self, msg, pairs, newv):
        super().__init__(msg)
        self.pairs, self.newv = pairs, newv


class QhullMergeSuspect(LqroError):
    """lqro_step returned LQRO_E_QHMERGE: the step completed, but for some
    inside-hull pairs the winning facet may be one that qconvex's default
    pre-merge joins into a merged facet (LQRO_REC_QHMERGE_WIN; convexHull
    then measures from the merged facet's first Fv vertex with its merged
    plane, LQRO:925-939, 956-967).  Qhull's merging is not restated, so those
    pairs' half-planes are not pinned to the reference.  .pairs: their (i, j);
    .newv: the step's new velocities."""

    def __init__(self, msg, pairs, newv):
        super().__init__(msg)
        self.pairs, self.newv = pairs, newv


def _check(rc: int, what: str):
    if rc != LQRO_OK:
        msg = lib().lqro_status_string(rc).decode()
        raise LqroError(f"{what}: {msg} ({rc})")


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def default_model() -> Model:
    m = Model()
    lib().lqro_model_default(C.byref(m))
    return m


def gain_shapes(x_dim: int = 16) -> dict:
    """controlMatrices' outputs in the reference's argument order (LQRO:520)."""
    X = x_dim
    return dict(A=(X, X), B=(X, 4), c=(X,), L=(4, X), E=(4, 3), l=(4,), Lh=(3, X), Eh=(3, 3))


GAIN_SHAPES = gain_shapes(16)


def synthesize_gains(model: Model | None = None, x_dim: int = 16) -> dict:
    """controlMatrices at hover (LQRO:520-582): A, B, c, L, E, l, Lh, Eh.
    x_dim = 12: BASELINE config 5's reduced model (rotor-force states
    dropped, F = u; lqro_synthesize_gains_x)."""
    m = model or default_model()
    shp = gain_shapes(x_dim)
    out = {k: np.zeros(s) for k, s in shp.items()}
    _check(lib().lqro_synthesize_gains_x(C.byref(m), x_dim, *[_p(out[k]) for k in shp]),
           "lqro_synthesize_gains_x")
    return out


def synthesize_gains_batch(models, device: int = 0, x_dim: int = 16) -> dict:
    """controlMatrices for heterogeneous agents, on the GPU (one agent per
    lane): arrays with a leading agent axis, bit-identical to
    synthesize_gains(models[k], x_dim); L and E feed
    Context.set_gains(per_agent=1)."""
    n = len(models)
    arr = (Model * n)(*models)
    shp = gain_shapes(x_dim)
    out = {k: np.zeros((n,) + s) for k, s in shp.items()}
    _check(lib().lqro_synthesize_gains_batch_x(arr, n, x_dim, *[_p(out[k]) for k in shp], device),
           "lqro_synthesize_gains_batch_x")
    return out


def perturbed_models(n: int, rel: float = 0.01, seed: int | None = None) -> list:
    """n agent models with mass, inertia, arm length, moment constant, thrust
    latency and the cost weights qv, qp, r each scaled by a factor in
    [1 - rel, 1 + rel] (SplitMix64, seeded): the heterogeneous swarm of
    BASELINE config 5."""
    g = _splitmix(SEED_MODELS if seed is None else seed)
    base = default_model()
    out = []
    for _ in range(n):
        m = Model.from_buffer_copy(base)
        for f in ("mass", "inertia", "length", "moment_const", "thrust_latency", "qv", "qp", "r"):
            setattr(m, f, getattr(base, f) * (1.0 + rel * (2.0 * next(g) - 1.0)))
        out.append(m)
    return out


def create_spheres(n_points: int = 100, xy_radius: float = 0.26, z_radius: float = 0.75):
    """createSpheres (LQRO:735-750)."""
    s = np.zeros((n_points, 3))
    _check(lib().lqro_sphere(n_points, xy_radius, z_radius, _p(s)), "lqro_sphere")
    return s


def config(n_agents: int, horizon: int, n_points: int = 100, **kw) -> Config:
    c = Config()
    lib().lqro_config_default(C.byref(c), n_agents, horizon, n_points)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


class Context:
    """One liblqro context: owns device buffers and a HIP stream."""

    def __init__(self, cfg: Config):
        self.cfg = cfg
        h = C.c_void_p()
        _check(lib().lqro_create(C.byref(cfg), C.byref(h)), "lqro_create")
        self._h = h
        rb, re = cfg.row_begin, cfg.row_end
        if rb == 0 and re == 0:
            re = cfg.n_agents
        self.rows = (rb, re)
        self.row_ids = np.arange(rb, re, max(cfg.row_stride, 1))   # the agents whose rows this computes
        self.n_obstacles = 0
        self._obs_keep = None      # a device tensor given to set_obstacles, kept alive
        self._act_keep = None      # ... and one given to set_active
        self._ix_keep = None       # ... and one given to set_interaction

    def close(self):
        if self._h:
            lib().lqro_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_neighbors(self, neighbor_dist: float, max_neighbors: int):
        """Opt-in neighbour culling (lqro_set_neighbors; RVO2 computeNeighbors,
        AGT:74-81,153-174).  Changes results; max_neighbors <= 0 = all pairs."""
        _check(lib().lqro_set_neighbors(self._h, float(neighbor_dist), int(max_neighbors)),
               "lqro_set_neighbors")

    def set_user_planes(self, plane_lists):
        """Opt-in half-planes of each agent's LP ahead of its pair planes
        (lqro_set_user_planes; RVO2's obstacle-first order, AGT:84-151).
        plane_lists: one (m_i, 6) float32 array per agent (point, normal; v is
        allowed when normal.(v - point) >= 0), in push order, indexed by the
        global agent id; None clears.  Changes results against the reference."""
        if plane_lists is None:
            _check(lib().lqro_set_user_planes(self._h, None, None), "lqro_set_user_planes")
            return
        n = self.cfg.n_agents
        if len(plane_lists) != n:
            raise LqroError(f"set_user_planes: {len(plane_lists)} lists for {n} agents")
        offs = np.zeros(n + 1, dtype=np.int64)
        for r, p in enumerate(plane_lists):
            offs[r + 1] = offs[r] + len(p)
        flat = np.zeros((max(int(offs[-1]), 1), 6), dtype=np.float32)
        for r, p in enumerate(plane_lists):
            if len(p):
                flat[offs[r]:offs[r + 1]] = np.asarray(p, dtype=np.float32).reshape(-1, 6)
        _check(lib().lqro_set_user_planes(self._h, _p(flat), _p(offs)), "lqro_set_user_planes")

    def set_user_planes_device(self, ptr: int, max_per_agent: int, counts_ptr: int = 0):
        """The same from device memory at a fixed pitch (e.g. a float32 torch
        tensor (N, max_per_agent, 6) and an int32 (N,) tensor of live counts,
        by .data_ptr(); counts_ptr = 0: all live).  The pointers are read when
        the step's LP runs: keep the tensors alive and write them on the
        step's stream before the step.  max_per_agent <= 0 clears."""
        _check(lib().lqro_set_user_planes_device(self._h, C.c_void_p(ptr or None), int(max_per_agent),
                                                 C.c_void_p(counts_ptr or None)), "lqro_set_user_planes_device")

    def set_fence(self, lo, hi, tau: float):
        """An axis-aligned box [lo, hi] the agents' ellipsoids should stay
        inside within tau seconds, as up to six half-planes per agent ahead of
        the user and pair planes (lqro_set_fence).  -inf / +inf bounds emit no
        face (lo = (-inf, -inf, 0), hi = inf: a floor); lo = None or tau <= 0
        turns the fence off.  Changes results against the reference."""
        if lo is None or hi is None:
            _check(lib().lqro_set_fence(self._h, None, None, 0.0), "lqro_set_fence")
            return
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (3,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (3,)))
        _check(lib().lqro_set_fence(self._h, _p(lo), _p(hi), float(tau)), "lqro_set_fence")

    def set_obstacles(self, states, xy_radius=None, z_radius=None, responsibility=1.0):
        """Obstacles: M columns of every row's pair loop that are not agents
        (lqro_set_obstacles; the reference's commented floor block,
        LQRO:1377-1379, 1421-1434, 752-767).  states: (M, x_dim) — a numpy
        array (copied), or a float64 torch tensor on the context's device,
        read when each step runs (rewrite it on the step's stream before the
        step: obstacles that move); obstacle_states() builds hover-trim ones.
        None or M = 0 clears.  xy_radius / z_radius: the obstacles' ellipsoid
        (default: the agents'; (0, 0): a point); responsibility in (0, 1]
        replaces the 0.5 of LQRO:1416 for an obstacle column (1.0: the agent
        does all the avoiding).  Each of the three is a scalar for all the
        obstacles or a sequence of M, one value per obstacle
        (lqro_set_obstacles_ex: up to LQRO_OBS_SHAPES_MAX distinct shapes
        besides the agents').  A row then has n_agents - 1 + M records, the
        obstacle ones with j = n_agents + o.  Changes results against the
        reference."""
        X = self.cfg.x_dim
        if states is None:
            _check(lib().lqro_set_obstacles(self._h, None, 0, self.cfg.xy_radius, self.cfg.z_radius, 1.0),
                   "lqro_set_obstacles")
            self.n_obstacles, self._obs_keep = 0, None
            return
        dev = not (isinstance(states, np.ndarray) or not hasattr(states, "data_ptr"))
        if dev:
            import torch
            if states.dtype != torch.float64 or not states.is_cuda or not states.is_contiguous() or \
                    states.dim() != 2 or states.shape[1] != X:
                raise LqroError(f"set_obstacles: need a contiguous float64 device tensor (M, {X})")
            m = int(states.shape[0])
            ptr = C.c_void_p(states.data_ptr() if m else None)
        else:
            st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, X)
            m, ptr = st.shape[0], _p(st)
        per, oxy, oz, resp = obstacle_arrays(m, xy_radius, z_radius, responsibility, self.cfg.xy_radius,
                                             self.cfg.z_radius)
        if per:
            name = "lqro_set_obstacles_ex_device" if dev else "lqro_set_obstacles_ex"
            _check(getattr(lib(), name)(self._h, ptr, m, _p(oxy), _p(oz), _p(resp)), name)
        else:
            name = "lqro_set_obstacles_device" if dev else "lqro_set_obstacles"
            _check(getattr(lib(), name)(self._h, ptr, m, oxy, oz, resp), name)
        self.n_obstacles, self._obs_keep = m, (states if dev and m else None)

    def set_active(self, mask):
        """Which agents take part in the steps that follow (lqro_set_active):
        an inactive agent is neither a row nor a column, the step equals the
        step over the compacted swarm, and its own row's newV is +0.0.  mask:
        a numpy bool / uint8 array of n_agents entries (copied; another length
        raises ValueError), or a uint8 torch tensor of n_agents bytes on the
        context's device, or an integer device pointer to as many, read when
        each step runs (rewrite it on the step's stream before the step; the
        tensor is kept alive here).  None clears: everybody takes part."""
        n = self.cfg.n_agents
        if mask is None:
            _check(lib().lqro_set_active(self._h, None), "lqro_set_active")
            self._act_keep = None
            return
        if isinstance(mask, (int, np.integer)) and not isinstance(mask, (bool, np.bool_)):
            _check(lib().lqro_set_active_device(self._h, C.c_void_p(int(mask))), "lqro_set_active_device")
            self._act_keep = None
            return
        if hasattr(mask, "data_ptr"):
            import torch
            if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or mask.numel() != n:
                raise ValueError(f"set_active: need a contiguous uint8 device tensor of {n} bytes")
            _check(lib().lqro_set_active_device(self._h, C.c_void_p(mask.data_ptr())), "lqro_set_active_device")
            self._act_keep = mask
            return
        m = np.asarray(mask)
        if m.dtype != np.bool_ and m.dtype != np.uint8:
            raise ValueError("set_active: a bool or uint8 array")
        if m.ndim != 1 or m.shape[0] != n:
            raise ValueError(f"set_active: {m.shape} entries for {n} agents")
        m = np.ascontiguousarray(m != 0, dtype=np.uint8)
        _check(lib().lqro_set_active(self._h, _p(m)), "lqro_set_active")
        self._act_keep = None

    def set_interaction(self, cls, share, device=False):
        """Interaction classes (lqro_set_interaction): agent i belongs to class
        cls[i], and share[a][b] in [0, 1] is the factor a row of class a applies
        against an agent column of class b in place of the reference's 0.5; a
        share of exactly 0.0: the row ignores the column (the slot is dead, as
        an inactive column's under set_active).  share: a C x C array, C <=
        LQRO_CLASSES_MAX, copied.  cls: a numpy integer array of n_agents
        entries below C (copied; another length, an entry outside 0..C-1 or a
        share outside [0, 1] raises ValueError).  device=True: cls is a uint8
        torch tensor of n_agents bytes on the context's device, or an integer
        device pointer to as many, read when each step runs (rewrite it on the
        step's stream before the step; the tensor is kept alive here; a byte
        >= C reads as C - 1).  cls or share None clears: no table."""
        n = self.cfg.n_agents
        if cls is None or share is None:
            _check(lib().lqro_set_interaction(self._h, None, 0, None), "lqro_set_interaction")
            self._ix_keep = None
            return
        sh = np.ascontiguousarray(share, dtype=np.float64)
        if sh.ndim != 2 or sh.shape[0] != sh.shape[1] or not 1 <= sh.shape[0] <= LQRO_CLASSES_MAX:
            raise ValueError(f"set_interaction: share is C x C, 1 <= C <= {LQRO_CLASSES_MAX}")
        if not (np.isfinite(sh).all() and (sh >= 0.0).all() and (sh <= 1.0).all()):
            raise ValueError("set_interaction: every share lies in [0, 1]")
        nc = int(sh.shape[0])
        if device:
            if isinstance(cls, (int, np.integer)) and not isinstance(cls, (bool, np.bool_)):
                ptr, keep = int(cls), None
            elif hasattr(cls, "data_ptr"):
                import torch
                if cls.dtype != torch.uint8 or not cls.is_cuda or not cls.is_contiguous() or cls.numel() != n:
                    raise ValueError(f"set_interaction: need a contiguous uint8 device tensor of {n} bytes")
                ptr, keep = cls.data_ptr(), cls
            else:
                raise ValueError("set_interaction: device=True takes a device tensor or pointer")
            _check(lib().lqro_set_interaction_device(self._h, C.c_void_p(ptr), nc, _p(sh)),
                   "lqro_set_interaction_device")
            self._ix_keep = keep
            return
        k = np.asarray(cls)
        if k.dtype.kind not in "iu":
            raise ValueError("set_interaction: cls is an integer array")
        if k.ndim != 1 or k.shape[0] != n:
            raise ValueError(f"set_interaction: {k.shape} entries for {n} agents")
        if n and (k.min() < 0 or k.max() >= nc):
            raise ValueError(f"set_interaction: a class outside 0..{nc - 1}")
        k = np.ascontiguousarray(k, dtype=np.uint8)
        _check(lib().lqro_set_interaction(self._h, _p(k), nc, _p(sh)), "lqro_set_interaction")
        self._ix_keep = None

    def set_hard_planes(self, level: int):
        """Which planes linearProgram4 keeps out of its relaxation
        (lqro_set_hard_planes; RVO2's obstacle lines): LQRO_HARD_NONE (the
        default), LQRO_HARD_FENCE (the fence planes), LQRO_HARD_HEAD (the user
        planes too), LQRO_HARD_OBSTACLES (also the obstacle columns' planes,
        which the LP then takes ahead of the agent planes).  Once the hard
        planes and the speed sphere are feasible together and the result
        satisfies them, no later relaxation leaves them; hard planes that are
        infeasible among themselves guarantee nothing.  The level stays when
        fence, user planes or obstacles are set or cleared later."""
        _check(lib().lqro_set_hard_planes(self._h, int(level)), "lqro_set_hard_planes")

    def clearance(self, x):
        """How clear the own rows of the (n_agents, x_dim) host array x are of
        every column (lqro_clearance: the agents j != i, then the obstacles as
        the step reads them; lqro.h states the formulas): (rows, total) — a
        CLEARANCE_ROW_DTYPE array in own-row order and the total as a dict.
        Also becomes the context's last total and folds into its since-reset
        one (monitor())."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.cfg.n_agents, self.cfg.x_dim):
            raise LqroError(f"clearance: x has shape {x.shape}, expected {(self.cfg.n_agents, self.cfg.x_dim)}")
        rows = np.zeros(len(self.row_ids), dtype=CLEARANCE_ROW_DTYPE)
        t = ClearanceTotal()
        _check(lib().lqro_clearance(self._h, _p(x), _p(rows), C.byref(t)), "lqro_clearance")
        return rows, _total_dict(t)

    def clearance_device(self, ptr: int, rows_ptr: int = 0, stream: int = 0):
        """The same on a device array (e.g. x_true.data_ptr()), enqueued on
        `stream` behind the context's last step, without a host wait
        (lqro_clearance_device).  rows_ptr = 0: the context's own row buffer;
        monitor() / monitor_rows() read the result."""
        _check(lib().lqro_clearance_device(self._h, C.c_void_p(ptr or None), C.c_void_p(rows_ptr or None),
                                           C.c_void_p(stream or None)), "lqro_clearance_device")

    def set_monitor(self, on):
        """on: every step measures its own columns at its head, on the step's
        stream, and accumulates on the device (lqro_set_monitor); the step's
        results do not change.  Off: no launch."""
        _check(lib().lqro_set_monitor(self._h, int(on)), "lqro_set_monitor")

    def monitor(self, reset: bool = False):
        """(last, since_reset) totals as dicts, after waiting for the last
        step or measurement (lqro_get_monitor); reset clears the since-reset
        total after reading it."""
        a, b = ClearanceTotal(), ClearanceTotal()
        _check(lib().lqro_get_monitor(self._h, C.byref(a), C.byref(b), int(bool(reset))), "lqro_get_monitor")
        return _total_dict(a), _total_dict(b)

    def monitor_rows(self) -> np.ndarray:
        """The last measurement's rows (empty before the first)."""
        rows = np.zeros(len(self.row_ids), dtype=CLEARANCE_ROW_DTYPE)
        n = C.c_int64()
        _check(lib().lqro_get_monitor_rows(self._h, _p(rows), len(rows), C.byref(n)), "lqro_get_monitor_rows")
        return rows[:n.value]

    def monitor_pairs(self) -> np.ndarray:
        """The last measurement's hit pairs (i, column) in (i, column) order,
        at most six a row: compare len() with the total's n_hit."""
        out = np.zeros((6 * len(self.row_ids), 2), np.int64)
        n = C.c_int64()
        _check(lib().lqro_get_monitor_pairs(self._h, _p(out), len(out), C.byref(n)), "lqro_get_monitor_pairs")
        return out[:n.value]

    def predict(self, x, v):
        """Horizon conflict prediction (lqro_predict): with the states x
        (N, X) and the commanded velocities v (N, 3), each own row's smallest
        predicted separation over the horizon, its first predicted hit and its
        conflict columns.  Returns (rows, total): PREDICT_ROW_DTYPE records in
        row order and this prediction's total; prediction() reads the
        accumulated ones, paths() the agents' predicted paths."""
        x = np.ascontiguousarray(x, np.float64)
        v = np.ascontiguousarray(v, np.float64)
        if x.shape != (self.cfg.n_agents, self.cfg.x_dim) or v.shape != (self.cfg.n_agents, 3):
            raise LqroError(f"predict: x {x.shape}, v {v.shape}, expected "
                            f"{(self.cfg.n_agents, self.cfg.x_dim)} and {(self.cfg.n_agents, 3)}")
        rows = np.zeros(len(self.row_ids), PREDICT_ROW_DTYPE)
        t = PredictTotal()
        _check(lib().lqro_predict(self._h, _p(x), _p(v), _p(rows), C.byref(t)), "lqro_predict")
        return rows, _predict_total_dict(t)

    def predict_device(self, x_ptr: int, v_ptr: int, rows_ptr: int = 0, stream: int = 0):
        """The same on device arrays, asynchronous on `stream`, ordered behind
        the context's last step and measurement (lqro_predict_device)."""
        _check(lib().lqro_predict_device(self._h, C.c_void_p(x_ptr or None), C.c_void_p(v_ptr or None),
                                         C.c_void_p(rows_ptr or None), C.c_void_p(stream or None)),
               "lqro_predict_device")

    def predict_paths(self, paths):
        """The same measurement over caller-given paths (N + M, H, 3), the
        obstacle columns the caller's own (lqro_predict_paths)."""
        paths = np.ascontiguousarray(paths, np.float64)
        want = (self.cfg.n_agents + self.n_obstacles, self.cfg.horizon, 3)
        if paths.shape != want:
            raise LqroError(f"predict_paths: paths has shape {paths.shape}, expected {want}")
        rows = np.zeros(len(self.row_ids), PREDICT_ROW_DTYPE)
        t = PredictTotal()
        _check(lib().lqro_predict_paths(self._h, _p(paths), _p(rows), C.byref(t)), "lqro_predict_paths")
        return rows, _predict_total_dict(t)

    def predict_paths_device(self, paths_ptr: int, rows_ptr: int = 0, stream: int = 0):
        _check(lib().lqro_predict_paths_device(self._h, C.c_void_p(paths_ptr or None), C.c_void_p(rows_ptr or None),
                                               C.c_void_p(stream or None)), "lqro_predict_paths_device")

    def prediction(self, reset: bool = False):
        """(last, since_reset) prediction totals as dicts (lqro_get_prediction);
        reset clears the since-reset total after reading it."""
        a, b = PredictTotal(), PredictTotal()
        _check(lib().lqro_get_prediction(self._h, C.byref(a), C.byref(b), int(bool(reset))), "lqro_get_prediction")
        return _predict_total_dict(a), _predict_total_dict(b)

    def prediction_rows(self) -> np.ndarray:
        """The last prediction's row records (empty before the first)."""
        rows = np.zeros(len(self.row_ids), PREDICT_ROW_DTYPE)
        n = C.c_int64()
        _check(lib().lqro_get_prediction_rows(self._h, _p(rows), len(rows), C.byref(n)), "lqro_get_prediction_rows")
        return rows[:n.value]

    def paths(self) -> np.ndarray:
        """The agents' paths (N, H, 3) of the last predict / predict_device."""
        out = np.zeros((self.cfg.n_agents, self.cfg.horizon, 3))
        _check(lib().lqro_get_paths(self._h, _p(out)), "lqro_get_paths")
        return out

    def set_lp_audit(self, on, tol: float = 0.0):
        """on: every step audits its own rows at its end, on the step's
        stream: the result against each plane the row's LP saw
        (lqro_set_lp_audit; lqro.h states the formulas); the step's results do
        not change.  tol >= 0: the margin above which a plane counts as
        violated (RVO_EPSILON suits).  Off: no launch."""
        _check(lib().lqro_set_lp_audit(self._h, int(on), float(tol)), "lqro_set_lp_audit")

    def lp_audit(self, reset: bool = False):
        """(last, since_reset) LP-audit totals as dicts, after waiting for the
        last step (lqro_get_lp_audit); reset clears the since-reset total
        after reading it."""
        a, b = LpTotal(), LpTotal()
        _check(lib().lqro_get_lp_audit(self._h, C.byref(a), C.byref(b), int(bool(reset))), "lqro_get_lp_audit")
        return _lp_total_dict(a), _lp_total_dict(b)

    def lp_audit_rows(self) -> np.ndarray:
        """The last audit's rows, an LP_ROW_DTYPE array in own-row order
        (empty before the first)."""
        rows = np.zeros(len(self.row_ids), dtype=LP_ROW_DTYPE)
        n = C.c_int64()
        _check(lib().lqro_get_lp_audit_rows(self._h, _p(rows), len(rows), C.byref(n)), "lqro_get_lp_audit_rows")
        return rows[:n.value]

    def set_gains(self, A, B, L, E, per_agent: bool = False):
        A, B, L, E = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, B, L, E))
        X, U, n = self.cfg.x_dim, self.cfg.u_dim, self.cfg.n_agents
        lead = (n,) if per_agent else ()
        for name, v, shp in (("A", A, (X, X)), ("B", B, (X, U)), ("L", L, lead + (U, X)),
                             ("E", E, lead + (U, 3))):
            if v.shape != shp and not (per_agent is False and v.shape == (1,) + shp):
                raise LqroError(f"set_gains: {name} has shape {v.shape}, expected {shp}")
        _check(lib().lqro_set_gains(self._h, _p(A), _p(B), _p(L), _p(E), int(per_agent)),
               "lqro_set_gains")

    def step(self, x: np.ndarray, vgoal: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        vgoal = np.ascontiguousarray(vgoal, dtype=np.float64)
        n = self.cfg.n_agents
        if x.shape != (n, self.cfg.x_dim):
            raise LqroError(f"step: x has shape {x.shape}, expected {(n, self.cfg.x_dim)}")
        if vgoal.shape != (n, 3):
            raise LqroError(f"step: vgoal has shape {vgoal.shape}, expected {(n, 3)}")
        newv = np.zeros((self.cfg.n_agents, 3))
        rc = lib().lqro_step(self._h, _p(x), _p(vgoal), _p(newv))
        if rc == LQRO_E_HULL:
            pairs = self.hull_failures()
            raise HullFailure(f"lqro_step: {len(pairs)} inside-hull pair(s) without a half-plane: "
                              f"{[tuple(p) for p in pairs[:8]]}", pairs, newv)
        if rc == LQRO_E_QHMERGE:
            pairs = self.qhmerge_pairs()
            raise QhullMergeSuspect(f"lqro_step: {len(pairs)} inside-hull pair(s) whose winning facet qconvex may "
                                    f"merge: {[tuple(p) for p in pairs[:8]]}", pairs, newv)
        _check(rc, "lqro_step")
        return newv

    def hull_failures(self) -> np.ndarray:
        """(i, j) of the last step's pairs left without a half-plane (at most 64)."""
        out = np.zeros((64, 2), np.int64)
        n = C.c_int64()
        _check(lib().lqro_get_hull_failures(self._h, _p(out), 64, C.byref(n)), "lqro_get_hull_failures")
        return out[:min(n.value, 64)]

    def qhmerge_pairs(self) -> np.ndarray:
        """(i, j) of the last step's LQRO_REC_QHMERGE_WIN pairs (at most 64)."""
        out = np.zeros((64, 2), np.int64)
        n = C.c_int64()
        _check(lib().lqro_get_qhmerge_pairs(self._h, _p(out), 64, C.byref(n)), "lqro_get_qhmerge_pairs")
        return out[:min(n.value, 64)]

    def step_device(self, d_x: int, d_vgoal: int, d_newv: int, stream: int = 0):
        """Device pointers (e.g. torch tensor .data_ptr()) on the context's
        device, enqueued on `stream` (a hipStream_t handle such as
        torch.cuda.current_stream().cuda_stream; 0 = the null stream, which is
        torch's default stream), so it is ordered with the caller's work."""
        _check(lib().lqro_step_device(self._h, C.c_void_p(d_x), C.c_void_p(d_vgoal),
                                      C.c_void_p(d_newv), C.c_void_p(stream or None)),
               "lqro_step_device")

    def step_device_begin(self, d_x: int, d_vgoal: int, d_rowtab: int, stream: int = 0):
        """The first half of step_device for row shards in Qhull order: sweep
        and hulls; this context's rows of the (N, 4) row-normal table
        d_rowtab are written (lqro_step_device_begin)."""
        _check(lib().lqro_step_device_begin(self._h, C.c_void_p(d_x), C.c_void_p(d_vgoal),
                                            C.c_void_p(d_rowtab), C.c_void_p(stream or None)),
               "lqro_step_device_begin")

    def step_device_end(self, d_rowtab: int, d_newv: int, stream: int = 0):
        """The second half, once every rank's rows of d_rowtab are present:
        the facet-0 pairs' loop-carried normals, then the LP."""
        _check(lib().lqro_step_device_end(self._h, C.c_void_p(d_rowtab), C.c_void_p(d_newv),
                                          C.c_void_p(stream or None)), "lqro_step_device_end")

    def records(self) -> np.ndarray:
        n = len(self.row_ids) * (self.cfg.n_agents - 1 + self.n_obstacles)
        out = np.zeros(n, dtype=RECORD_DTYPE)
        got = C.c_int64()
        _check(lib().lqro_get_records(self._h, _p(out), n, C.byref(got)), "lqro_get_records")
        return out[:got.value]   # rows x K with neighbour culling on

    def stats(self) -> dict:
        s = np.zeros(12, dtype=np.int64)
        _check(lib().lqro_get_stats_ex(self._h, _p(s), 12), "lqro_get_stats_ex")
        keys = ("pairs", "planes", "inside", "hull_ok", "hull_fail", "gjk_backups",
                "sum_n_reach", "sum_gtests", "qhull_merged", "qhull_retried", "qhull_timeouts",
                "qhull_merge_win")
        return dict(zip(keys, (int(v) for v in s)))

    def hull_builds(self) -> np.ndarray:
        """LQRO_FLAG_QHULL_ORDER: the last step's hull builds (lqro_get_hull_builds):
        i, j, n_points, insertions, facet_slots, kernel (0 k_qhull, 1 k_qhull_big,
        2 a k_qhull build handed over), t_start / t_end in 100 MHz ticks."""
        out = np.zeros(16384, dtype=HULL_BUILD_DTYPE)
        n = C.c_int64()
        _check(lib().lqro_get_hull_builds(self._h, _p(out), len(out), C.byref(n)), "lqro_get_hull_builds")
        return out[:min(n.value, len(out))]

    def carry_normal(self, n=None):
        """LQRO_FLAG_QHULL_ORDER: get (n=None) the loop-carried normalVector
        (LQRO:1385) the last step left, or set the one entering the next."""
        if n is None:
            out = np.zeros(3)
            _check(lib().lqro_get_carry_normal(self._h, _p(out)), "lqro_get_carry_normal")
            return out
        v = np.ascontiguousarray(n, dtype=np.float64)
        _check(lib().lqro_set_carry_normal(self._h, _p(v)), "lqro_set_carry_normal")

    def debug_qhull(self, rounded: np.ndarray, full: np.ndarray, vrel, max_facets: int = 0):
        """Test hook: k_qhull on given points (rounded = qconvex's input, full =
        the distances' points): (record, build status bits[, facet list in
        Qhull's order, Fv triples, when max_facets > 0]).  self.debug_status:
        the hook's C-ABI status, LQRO_E_QHMERGE for a merge-suspect winner
        (lqro_step's rule)."""
        n = rounded.shape[0]
        pts = np.ascontiguousarray(np.concatenate([rounded.reshape(-1), full.reshape(-1)]), dtype=np.float64)
        v = np.ascontiguousarray(vrel, dtype=np.float64)
        rec = PairRecord()
        nf = C.c_int32()
        fn = lib().lqro_debug_hull_points
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                       C.POINTER(C.c_int32), C.POINTER(PairRecord)]
        fl = np.zeros((max(max_facets, 1), 3), np.int32)
        rc = fn(self._h, _p(pts), n, _p(v), 2, _p(fl) if max_facets else None, max_facets, C.byref(nf),
                C.byref(rec))
        self.debug_status = rc
        if rc != LQRO_E_QHMERGE:
            _check(rc, "lqro_debug_hull_points")
        r = np.frombuffer(bytes(rec), dtype=RECORD_DTYPE)[0]
        if max_facets:
            end = np.nonzero(fl[:, 0] < 0)[0]
            return r, int(nf.value), fl[: end[0] if len(end) else max_facets]
        return r, int(nf.value)

    def debug_hull(self, points: np.ndarray, vrel, mode: int = 0, max_facets: int = 0):
        """Test hook (lqro_debug_hull_points_ex): the canonical rule's hull
        kernels on given points (already %g-rounded; n <= H * NP): mode 0
        k_hull, 1 k_lhull, 3 k_hull_big alone, 4 k_hull then k_hull_big on its
        retry queue, as the step launches them.  Returns (record, facets,
        status).  facets: k_hull's facet list (point ids, k x 3) where it
        finished a build (modes 0 and 4), else None.  status, modes 0 and 4:
        k_hull's facet count, -2: it handed the points to k_hull_big (mode 4:
        which has decided; the record is its); mode 3: the record's facet
        count, -1: no hull; mode 1: 0 when k_lhull decided, else its hand-over
        reason (its fail code 21..35; 20: the point set or the initial
        tetrahedron).  self.debug_hull_fails (modes 0, 3, 4): the fail codes
        the call's builds ended with, ascending (1 the vertex cap, 4 the face
        slots, 8 a degenerate set, ...; empty: every build finished)."""
        if mode not in (0, 1, 3, 4):
            raise ValueError("debug_hull: mode 0, 1, 3 or 4 (k_qhull: debug_qhull)")
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        v = np.ascontiguousarray(vrel, dtype=np.float64)
        lists = mode in (0, 4)
        cap = (max_facets if max_facets > 0 else 2 * pts.shape[0]) if lists else 1   # (a hull has 2n - 4 facets at most)
        fl = np.zeros((cap, 3), np.int32)
        rec = PairRecord()
        nf = C.c_int32()
        reason = np.zeros(16, np.int64)
        fn = lib().lqro_debug_hull_points_ex
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                       C.POINTER(C.c_int32), C.POINTER(PairRecord), C.c_void_p]
        _check(fn(self._h, _p(pts), pts.shape[0], _p(v), mode, _p(fl) if lists else None, cap if lists else 0,
                  C.byref(nf), C.byref(rec), _p(reason)), "lqro_debug_hull_points_ex")
        r = np.frombuffer(bytes(rec), dtype=RECORD_DTYPE)[0]
        status = int(nf.value)
        self.debug_hull_fails = () if mode == 1 else tuple(int(k) for k in np.nonzero(reason[1:])[0] + 1)
        if mode == 1:
            k = np.nonzero(reason)[0]
            status = 0 if status == 0 else 20 + int(k[0]) if len(k) else -1
        facets = fl[:min(status, cap)].copy() if lists and status > 0 else None
        return r, facets, status

    def timings(self) -> dict:
        t = np.zeros(4, dtype=np.float32)
        _check(lib().lqro_get_timings(self._h, _p(t)), "lqro_get_timings")
        return dict(pair_ms=float(t[0]), hull_ms=float(t[1]), lp_ms=float(t[2]),
                    step_ms=float(t[3]))


def calculate_new_v(plane_lists, vgoals, vmax_lp: float = 100.0, device: int = 0, n_hard=None) -> np.ndarray:
    """calculateNewV (LQRO:1223-1234) for many agents at once on the GPU.
    plane_lists: sequence of (m_r, 6) float32 arrays (point, normal) in push
    order; vgoals: (n, 3).  n_hard: per agent, how many of its first planes
    linearProgram4 does not relax (lqro_calculate_new_v_hard; clamped to the
    agent's plane count, negative raises); None: none, the reference's LP."""
    n = len(plane_lists)
    offs = np.zeros(n + 1, dtype=np.int64)
    for r, p in enumerate(plane_lists):
        offs[r + 1] = offs[r] + len(p)
    flat = np.zeros((max(int(offs[-1]), 1), 6), dtype=np.float32)
    for r, p in enumerate(plane_lists):
        if len(p):
            flat[offs[r]:offs[r + 1]] = np.asarray(p, dtype=np.float32).reshape(-1, 6)
    vg = np.ascontiguousarray(vgoals, dtype=np.float64).reshape(n, 3)
    out = np.zeros((n, 3))
    if n_hard is not None:
        nh = np.ascontiguousarray(n_hard, dtype=np.int32).reshape(n)
        _check(lib().lqro_calculate_new_v_hard(_p(flat), _p(offs), _p(nh), n, _p(vg), vmax_lp, _p(out), device),
               "lqro_calculate_new_v_hard")
        return out
    _check(lib().lqro_calculate_new_v(_p(flat), _p(offs), n, _p(vg), vmax_lp, _p(out), device),
           "lqro_calculate_new_v")
    return out


def audit_new_v(plane_lists, vgoals, newv, tol: float = 0.0, n_hard=None, device: int = 0):
    """The LP audit without a context (lqro_audit_new_v), calculate_new_v's
    twin: newv ((n, 3)) against the same plane lists, agent r's first
    n_hard[r] planes hard (clamped; None: none).  Returns (rows, total): an
    LP_ROW_DTYPE array and the total as a dict; every plane has kind
    LQRO_AUDIT_USER and id = k."""
    n = len(plane_lists)
    offs = np.zeros(n + 1, dtype=np.int64)
    for r, p in enumerate(plane_lists):
        offs[r + 1] = offs[r] + len(p)
    flat = np.zeros((max(int(offs[-1]), 1), 6), dtype=np.float32)
    for r, p in enumerate(plane_lists):
        if len(p):
            flat[offs[r]:offs[r + 1]] = np.asarray(p, dtype=np.float32).reshape(-1, 6)
    vg = np.ascontiguousarray(vgoals, dtype=np.float64).reshape(n, 3)
    nv = np.ascontiguousarray(newv, dtype=np.float64).reshape(n, 3)
    nh = None if n_hard is None else np.ascontiguousarray(n_hard, dtype=np.int32).reshape(n)
    rows = np.zeros(n, dtype=LP_ROW_DTYPE)
    t = LpTotal()
    _check(lib().lqro_audit_new_v(_p(flat), _p(offs), None if nh is None else _p(nh), n, _p(vg), _p(nv), float(tol),
                                  _p(rows), C.byref(t), device), "lqro_audit_new_v")
    return rows, _lp_total_dict(t)


# ---------------------------------------------------------------------------
# Synthetic swarms: SplitMix64, seed "LQRO"
# ---------------------------------------------------------------------------
SEED = 0x4C51524F
SEED_MODELS = 0x4D4F444C   # "MODL"
_M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix(seed: int):
    s = seed & _M64
    while True:
        s = (s + 0x9E3779B97F4A7C15) & _M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        yield ((z ^ (z >> 31)) >> 11) * 2.0 ** -53


def synthetic_swarm(n: int, x_dim: int = 16, seed: int = SEED, box: float | None = None):
    """N agents at constant density: position U[-L/2,L/2]^3 with L = 4 N^(1/3),
    velocity U[-1,1]^3, hover attitude, rotor forces at nominalInput
    (LQRO:188); vGoal U[-1,1]^3.  Draw order per agent: 3 position, 3
    velocity, 3 vGoal."""
    g = _splitmix(seed)
    side = box if box is not None else 4.0 * n ** (1.0 / 3.0)
    nominal = 9.80665 * 0.500 / 4
    x = np.zeros((n, x_dim))
    vg = np.zeros((n, 3))
    for i in range(n):
        for k in range(3):
            x[i, k] = (next(g) - 0.5) * side
        for k in range(3):
            x[i, 3 + k] = 2.0 * next(g) - 1.0
        if x_dim == 16:
            x[i, 12:16] = nominal
        for k in range(3):
            vg[i, k] = 2.0 * next(g) - 1.0
    return x, vg


LQRO_OBS_SHAPES_MAX = 8


def obstacle_arrays(m: int, xy_radius, z_radius, responsibility, agent_xy: float, agent_z: float):
    """Context.set_obstacles's three arguments for M obstacles: (False, oxy,
    oz, resp) as floats when each is a scalar or None (the one-shape call), or
    (True, oxy, oz, resp) as float64 arrays of M with the scalars broadcast
    when any is a sequence (lqro_set_obstacles_ex).  A sequence of another
    length than M raises LqroError."""
    vals = [agent_xy if xy_radius is None else xy_radius, agent_z if z_radius is None else z_radius,
            1.0 if responsibility is None else responsibility]
    if all(np.ndim(v) == 0 for v in vals):
        return (False, *(float(v) for v in vals))
    out = []
    for name, v in zip(("xy_radius", "z_radius", "responsibility"), vals):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != m):
            raise LqroError(f"set_obstacles: {name} has {a.shape} values for {m} obstacles")
        out.append(np.ascontiguousarray(np.broadcast_to(a, (m,))))
    return (True, *out)


def obstacle_states(pos, vel=None, x_dim: int = 16) -> np.ndarray:
    """Hover-trim states for Context.set_obstacles: zeros, then position
    [0..2] and velocity [3..5] (default 0: a static obstacle), and for x_dim =
    16 the rotor forces at nominalInput (LQRO:188), as synthetic_swarm has
    them — so that x_i - x_o is a position / velocity difference only."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    st = np.zeros((pos.shape[0], x_dim))
    st[:, 0:3] = pos
    if vel is not None:
        st[:, 3:6] = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    if x_dim == 16:
        st[:, 12:16] = 9.80665 * 0.500 / 4
    return st


def swap_scenario():
    """The scripted 4-quad swap of LQRO:1308-1331 at its first step: states
    (x = xInit, hover forces) and the position goals."""
    nominal = 9.80665 * 0.500 / 4
    pos = [(4.0, 0.0, 2.0), (-4.0, -0.0, 2.0), (0.0, 4.0, 2.0), (0.0, -4.0, 2.0)]
    goal = [(-4.0, 0.0, 2.0), (4.0, 0.0, 2.0), (0.0, -4.0, 2.0), (0.0, 4.0, 2.0)]
    x = np.zeros((4, 16))
    for i, p in enumerate(pos):
        x[i, :3] = p
        x[i, 12:16] = nominal
    return x, np.array(goal)


# ---------------------------------------------------------------------------
# The per-agent step after the pair loop (LQRO:1437-1446), SURVEY §8f next #1
# ---------------------------------------------------------------------------
AGENT_FIELDS = dict(x=(16,), rot=(3, 3), x_true=(16,), rot_true=(3, 3), P=(16, 16), vgoal=(3,),
                    u_goal=(4,), p_goal=(3,))


def normals(seed: int, count: int) -> tuple[np.ndarray, int]:
    """`count` draws of the reference's normal() (LQRO:340-350) on the MSVC
    rand() stream seeded with `seed` (srand); returns (draws, next seed)."""
    st = C.c_uint32(seed & 0xFFFFFFFF)
    out = np.zeros(count)
    _check(lib().lqro_normals(C.byref(st), count, _p(out)), "lqro_normals")
    return out, int(st.value)


def agent_states(x, u_goal=None, p_goal=None, p0: float = 1e-9) -> dict:
    """Host-side agent records for dynamics_step: the estimate x, Rot = I,
    xTrue = x, RotTrue = I, P = p0 I (Pinit, LQRO:1297), vGoal = 0, uGoal =
    hover thrust, pGoal = 0 (setupQuadrotors, LQRO:107-122, without its
    initial noise draw)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.shape[0]
    hover = default_model().gravity * default_model().mass / 4
    st = dict(x=x.copy(), rot=np.tile(np.eye(3), (n, 1, 1)), x_true=x.copy(),
              rot_true=np.tile(np.eye(3), (n, 1, 1)), P=np.tile(p0 * np.eye(16), (n, 1, 1)),
              vgoal=np.zeros((n, 3)),
              u_goal=np.full((n, 4), hover) if u_goal is None else np.array(u_goal, dtype=np.float64),
              p_goal=np.zeros((n, 3)) if p_goal is None else np.array(p_goal, dtype=np.float64))
    return st


def dynamics_step(st: dict, gains: dict, nrm: np.ndarray, models=None, M=None, N=None,
                  per_agent: bool = False, device: int = 0, keyframes: np.ndarray | None = None,
                  time: float = 0.0) -> np.ndarray:
    """lqro_dynamics_step: advances every agent of `st` in place (x, rot,
    x_true, rot_true, P; vgoal in = newV, out = findVGoal()) and returns u.
    keyframes: optional n x 8 float32 array that receives visualize's
    keyframe (time, xTrue position, quatFromRot(RotTrue)) at `time`.
    gains: L, E, l, Lh, Eh (one set, or a leading agent axis with
    per_agent=True).  nrm: n x 22 draws.  M, N default to the reference's
    1e-9 I (LQRO:1285-1286)."""
    n = st["x"].shape[0]
    models = [default_model()] if models is None else list(models)
    marr = (Model * len(models))(*models)
    M = 1e-9 * np.eye(16) if M is None else M
    N = 1e-9 * np.eye(6) if N is None else N
    for k, shp in AGENT_FIELDS.items():
        if st[k].shape != (n,) + shp or st[k].dtype != np.float64 or not st[k].flags.c_contiguous:
            raise LqroError(f"dynamics_step: {k} must be C-contiguous float64 {(n,) + shp}")
    keep = [np.ascontiguousarray(v, dtype=np.float64) for v in
            (gains["L"], gains["E"], gains["l"], gains["Lh"], gains["Eh"], M, N, nrm)]
    if keep[-1].size != n * NORMALS_PER_AGENT:
        raise LqroError("dynamics_step: need n x 22 normals")
    u = np.zeros((n, 4))
    a = Agents(*[_p(st[k]).value for k in ("x", "rot", "x_true", "rot_true", "P", "vgoal")],
               _p(u).value, _p(st["u_goal"]).value, _p(st["p_goal"]).value,
               *[_p(v).value for v in keep])
    if keyframes is not None:
        if keyframes.shape != (n, 8) or keyframes.dtype != np.float32 or not keyframes.flags.c_contiguous:
            raise LqroError("dynamics_step: keyframes must be C-contiguous float32 (n, 8)")
        a.keyframes = _p(keyframes).value
    a.time = float(time)
    _check(lib().lqro_dynamics_step(marr, len(models), n, int(per_agent), C.byref(a), device),
           "lqro_dynamics_step")
    return u


# ---------------------------------------------------------------------------
# Reference-shaped interface
# ---------------------------------------------------------------------------
class Quadrotor:
    """The fields of class Quadrotor (LQRO:73-165) that the pair loop and the
    agent update (LQRO:1437-1446) use."""

    def __init__(self, x, vGoal=None, pGoal=None):
        self.x = np.asarray(x, dtype=np.float64).copy()
        self.vGoal = np.zeros(3) if vGoal is None else np.asarray(vGoal, dtype=np.float64).copy()
        self.newV = np.zeros(3)
        self.pGoal = np.zeros(3) if pGoal is None else np.asarray(pGoal, dtype=np.float64).copy()
        self.L = None
        self.E = None
        self.l = np.zeros(4)   # feedforward (LQRO:557), set by findMatrices; the pair path never reads it
        self.Lh = None
        self.Eh = None
        # estimation state (setupQuadrotors, LQRO:107-122, without its noise draw)
        self.Rot = np.eye(3)
        self.xTrue = self.x.copy()
        self.RotTrue = np.eye(3)
        self.P = 1e-9 * np.eye(16)


class Simulator:
    """The per-step driver of LQRO:1391-1436 on the GPU: ``findMatrices``
    once, then ``step()`` each control step fills every ``Quadrotor.newV``."""

    def __init__(self, qlist, horizon: int = 45, n_points: int = 100, device: int = 0,
                 records: bool = False, model: Model | None = None, hull_rule: str = "reference",
                 fence=None):
        self.qlist = list(qlist)
        self.model = model or default_model()
        # hull_rule "reference": the reference's own inside-hull rule (Qhull's
        # order, LQRO:925-968); "canonical": the faster deviating rule
        if hull_rule not in ("reference", "canonical"):
            raise ValueError(f"hull_rule {hull_rule!r}")
        flags = (LQRO_FLAG_RECORDS if records else 0) | (LQRO_FLAG_QHULL_ORDER if hull_rule == "reference" else 0)
        self.device = device
        self.t = 0                 # control steps taken (LQRO:1392)
        self.trajectory = []       # keyframes per step (update())
        self.ctx = Context(config(len(self.qlist), horizon, n_points, device=device,
                                  flags=flags))
        if fence is not None:      # (lo, hi, tau): Context.set_fence
            self.ctx.set_fence(*fence)
        self.A = self.B = self.c = None

    def findMatrices(self):
        g = synthesize_gains(self.model)
        self.A, self.B, self.c = g["A"], g["B"], g["c"]
        for q in self.qlist:
            q.L, q.E, q.l, q.Lh, q.Eh = g["L"], g["E"], g["l"], g["Lh"], g["Eh"]
        Ls = np.stack([q.L for q in self.qlist])
        Es = np.stack([q.E for q in self.qlist])
        per_agent = not all(np.array_equal(Ls[0], l) for l in Ls) or \
            not all(np.array_equal(Es[0], e) for e in Es)
        if per_agent:
            self.ctx.set_gains(self.A, self.B, Ls, Es, per_agent=True)
        else:
            self.ctx.set_gains(self.A, self.B, Ls[0], Es[0])
        return g

    def set_obstacles(self, states, xy_radius=None, z_radius=None, responsibility=1.0):
        """Bodies that are not in qlist as extra columns of every agent's pair
        loop (Context.set_obstacles: scalars, or one value per obstacle); None clears."""
        self.ctx.set_obstacles(states, xy_radius, z_radius, responsibility)

    def set_hard_planes(self, level: int):
        """Which of the fence, user and obstacle planes the LP never relaxes
        (Context.set_hard_planes)."""
        self.ctx.set_hard_planes(level)

    def set_active(self, mask):
        """Which quadrotors of qlist take part in step() (Context.set_active;
        None: all).  An inactive one is avoided by nobody and step() leaves its
        newV at zero; update() goes on propagating every agent."""
        self.ctx.set_active(mask)

    def set_interaction(self, cls, share, device=False):
        """Who of qlist avoids whom, and by how much (Context.set_interaction;
        None: no table).  It governs step() alone."""
        self.ctx.set_interaction(cls, share, device=device)

    def clearance(self):
        """Context.clearance on the agents' current estimates q.x."""
        return self.ctx.clearance(np.stack([q.x for q in self.qlist]))

    def predict(self):
        """Context.predict on the agents' current estimates q.x and the
        velocities newV the last step() chose."""
        return self.ctx.predict(np.stack([q.x for q in self.qlist]), np.stack([q.newV for q in self.qlist]))

    def set_lp_audit(self, on, tol: float = 0.0):
        """Every step() audits its LP's result on the device (Context.set_lp_audit)."""
        self.ctx.set_lp_audit(on, tol)

    def lp_audit(self, reset: bool = False):
        """(last, since_reset) totals of the steps' LP audits (Context.lp_audit)."""
        return self.ctx.lp_audit(reset)

    def step(self):
        x = np.stack([q.x for q in self.qlist])
        vg = np.stack([q.vGoal for q in self.qlist])
        try:
            newv = self.ctx.step(x, vg)
        except (QhullMergeSuspect, HullFailure) as e:
            # the step completed and wrote newV: stored, then raised (as
            # lqro::Simulator::step does)
            for q, v in zip(self.qlist, e.newv):
                q.newV = v.copy()
            raise
        for q, v in zip(self.qlist, newv):
            q.newV = v.copy()
        return newv

    def save_trajectory(self, path: str):
        """The keyframes update() recorded (Quadrotor::visualize's Callisto
        keys, LQRO:128-133): an .npz with `keyframes` (steps x agents x 8:
        time, xTrue position, quaternion) for offline diffing/plotting."""
        kf = np.stack(self.trajectory) if self.trajectory else np.zeros((0, len(self.qlist), 8),
                                                                        np.float32)
        np.savez_compressed(path, keyframes=kf, fields=np.array(
            ["time", "px", "py", "pz", "qx", "qy", "qz", "qw"]))

    def update(self, seed: int) -> int:
        """The agent loop after the pair loop (LQRO:1437-1446) on the GPU:
        vGoal = newV, findU, propagateU, kalmanFilter1, the observation draw,
        kalmanFilter2, vGoal = findVGoal.  Noise from the reference's rand()
        stream seeded with `seed`; returns the next seed."""
        n = len(self.qlist)
        nrm, seed = normals(seed, n * NORMALS_PER_AGENT)
        hover = self.model.gravity * self.model.mass / 4
        st = dict(x=np.stack([q.x for q in self.qlist]), rot=np.stack([q.Rot for q in self.qlist]),
                  x_true=np.stack([q.xTrue for q in self.qlist]),
                  rot_true=np.stack([q.RotTrue for q in self.qlist]),
                  P=np.stack([q.P for q in self.qlist]), vgoal=np.stack([q.newV for q in self.qlist]),
                  u_goal=np.full((n, 4), hover), p_goal=np.stack([q.pGoal for q in self.qlist]))
        gains = {k: np.stack([getattr(q, k) for q in self.qlist]) for k in ("L", "E", "l", "Lh", "Eh")}
        kf = np.zeros((n, 8), np.float32)
        dynamics_step(st, gains, nrm, models=[self.model], per_agent=True, device=self.device,
                      keyframes=kf, time=self.t * self.model.dt)
        self.trajectory.append(kf)
        self.t += 1
        for a, q in enumerate(self.qlist):
            q.x, q.Rot, q.xTrue, q.RotTrue, q.P = (st["x"][a].copy(), st["rot"][a].copy(),
                                                   st["x_true"][a].copy(), st["rot_true"][a].copy(),
                                                   st["P"][a].copy())
            q.vGoal = st["vgoal"][a].copy()
        return seed


# ---------------------------------------------------------------------------
# Multi-GPU: rows (agents i) block-sharded over ranks
# ---------------------------------------------------------------------------
ROW_MODES = ("block", "cyclic")


def row_shard(n_agents: int, rank: int, world: int) -> tuple[int, int]:
    """Rows [rb, re) owned by `rank`: balanced contiguous blocks (sizes
    differ by at most one).  Every pair (i, j) of row i is computed by the
    owner of i; no pair is split across ranks."""
    if not (0 <= rank < world) or n_agents < world:
        raise ValueError(f"cannot shard {n_agents} agents over {world} ranks")
    return rank * n_agents // world, (rank + 1) * n_agents // world


def shard_rows(n_agents: int, rank: int, world: int, mode: str = "block") -> dict:
    """The lqro_config fields of `rank`'s shard.  "block": row_shard's
    contiguous rows.  "cyclic": rows rank, rank + world, ... (row_stride =
    world) — agents that crowd into one region of the index space (a
    formation, the hull-heavy rows of SURVEY §8e) spread over every rank
    instead of loading one."""
    if mode not in ROW_MODES:
        raise ValueError(f"row mode {mode!r} not in {ROW_MODES}")
    if mode == "block":
        rb, re = row_shard(n_agents, rank, world)
        return dict(row_begin=rb, row_end=re, row_stride=0)
    if not (0 <= rank < world) or n_agents < world:
        raise ValueError(f"cannot shard {n_agents} agents over {world} ranks")
    return dict(row_begin=rank, row_end=n_agents, row_stride=world if world > 1 else 0)


def shard_row_ids(n_agents: int, rank: int, world: int, mode: str = "block") -> np.ndarray:
    f = shard_rows(n_agents, rank, world, mode)
    return np.arange(f["row_begin"], f["row_end"], max(f["row_stride"], 1))


def step_rows(ctx, dist, x, vgoal, newv, rowtab, rank: int, world: int, mode: str = "block", stream=None):
    """One pair-loop step of this rank's rows on torch device tensors, then
    the all-gather of newV.  In Qhull order with more than one rank the step
    is split around the all-gather of the (N, 4) row-normal table `rowtab`
    (lqro_step_device_begin / _end): the loop-carried normalVector
    (LQRO:1385) runs through the whole swarm's pairs in (i, j) order."""
    import torch
    st = stream if stream is not None else torch.cuda.current_stream(x.device)
    sid = st.cuda_stream
    if world > 1 and ctx.cfg.flags & LQRO_FLAG_QHULL_ORDER:
        ctx.step_device_begin(x.data_ptr(), vgoal.data_ptr(), rowtab.data_ptr(), sid)
        with torch.cuda.stream(st):
            allgather_rows(dist, rowtab, rank, world, mode=mode)
        ctx.step_device_end(rowtab.data_ptr(), newv.data_ptr(), sid)
    else:
        ctx.step_device(x.data_ptr(), vgoal.data_ptr(), newv.data_ptr(), sid)
    if world > 1:
        with torch.cuda.stream(st):
            allgather_rows(dist, newv, rank, world, mode=mode)


def allgather_rows(dist, full, rank: int, world: int, group=None, mode: str = "block"):
    """The per-step exchange: every rank holds its own rows of `full`
    (an (N, k) tensor, rows from shard_rows(mode)); afterwards every rank
    holds all rows.  One all-gather of equal ceil(N/world)-row chunks — RCCL
    over xGMI with the "nccl" backend, gloo on the CPU."""
    import torch

    n = full.shape[0]
    chunk = -(-n // world)

    def own(r):
        if mode == "cyclic":
            return full[r::world]
        b, e = row_shard(n, r, world)
        return full[b:e]

    if mode not in ROW_MODES:
        raise ValueError(f"row mode {mode!r} not in {ROW_MODES}")
    mine = own(rank)
    send = torch.zeros((chunk,) + tuple(full.shape[1:]), dtype=full.dtype, device=full.device)
    send[: mine.shape[0]] = mine
    recv = torch.empty((chunk * world,) + tuple(full.shape[1:]), dtype=full.dtype,
                       device=full.device)
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(recv, send, group=group)
    else:
        dist.all_gather(list(recv.chunk(world)), send, group=group)
    for r in range(world):
        dst = own(r)
        dst.copy_(recv[r * chunk: r * chunk + dst.shape[0]])
    return full


class DeviceLoop:
    """The whole control loop LQRO:1391-1446 on device buffers, for the rows
    this rank owns (rows="block": [rb, re); "cyclic": rank, rank + world, ...,
    gathered into contiguous copies around the dynamics): ``step()`` is the pair loop (lqro_step_device),
    ``update()`` the agent loop after it (vGoal = newV, lqro_dynamics_step_device
    on the own rows), then the single exchange per step: an all-gather of the
    new estimates x.  Every launch goes on `stream` (default:
    torch's current stream), so RCCL's stream waits order the exchange against
    the kernels and no device synchronisation is needed between the calls.

    The noise of step t is the reference's rand() stream for all N agents in
    agent order (LQRO:1437-1446 draws per agent in turn); each rank uses its
    own rows' draws, so a sharded run equals the single-context run bit for
    bit."""

    def __init__(self, x0, vgoal0, gains: dict, horizon: int, n_points: int = 100, *,
                 p_goal=None, rank: int = 0, world: int = 1, dist=None, device=None,
                 model: Model | None = None, seed: int = 1, stream=None, rows: str = "block",
                 flags: int = LQRO_FLAG_QHULL_ORDER, fence=None, user_planes=None, obstacles=None,
                 monitor: bool = False, lp_audit=False, predict: bool = False):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.dev)
        n = x0.shape[0]
        self.n, self.rank, self.world, self.dist = n, rank, world, dist
        self.mode = rows
        sh = shard_rows(n, rank, world, rows)
        ids = shard_row_ids(n, rank, world, rows)
        self.rb, self.re = int(ids[0]), int(ids[-1]) + 1     # block mode: the own rows [rb, re)
        rows = len(ids)
        self.model = model or default_model()
        self.seed = seed
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.ctx = Context(config(n, horizon, n_points, device=self.dev.index, flags=flags, **sh))
        self.ids_h = ids
        self.ids = torch.from_numpy(ids.astype(np.int64)).to(self.dev)
        self.ctx.set_gains(gains["A"], gains["B"], gains["L"], gains["E"])
        # opt-in constraints ahead of the pair planes: fence = (lo, hi, tau),
        # user_planes = one (m_i, 6) array per agent (global ids: every rank the same)
        if fence is not None:
            self.ctx.set_fence(*fence)
        if user_planes is not None:
            self.ctx.set_user_planes(user_planes)
        # obstacles = states, or (states, xy_radius, z_radius, responsibility):
        # every rank the same set (Context.set_obstacles)
        if obstacles is not None:
            self.set_obstacles(*(obstacles if isinstance(obstacles, tuple) else (obstacles,)))
        # monitor: every step measures its own rows' clearance on the device (monitor() reads it)
        if monitor:
            self.ctx.set_monitor(1)
        # lp_audit: every step audits its own rows' LP result on the device (lp_audit() reads it);
        # True, or the tolerance itself
        if lp_audit is not False and lp_audit is not None:
            self.ctx.set_lp_audit(1, 0.0 if lp_audit is True else float(lp_audit))
        # predict: every step() ends with a horizon conflict prediction of (x, newV) (prediction() reads it)
        self.predict_each = bool(predict)
        self.x = torch.from_numpy(np.ascontiguousarray(x0, np.float64)).to(self.dev)
        self.vgoal = torch.from_numpy(np.ascontiguousarray(vgoal0, np.float64)).to(self.dev)
        self.newv = torch.zeros((n, 3), **f64)
        self.flags = flags
        self.rowtab = torch.zeros((n, 4), **f64)   # per-row loop-carried normals (Qhull order, world > 1)
        eye3 = torch.eye(3, **f64).repeat(rows, 1, 1).contiguous()
        hover = self.model.gravity * self.model.mass / 4
        pg = np.zeros((n, 3)) if p_goal is None else np.asarray(p_goal, np.float64)
        self.own = dict(rot=eye3.clone(), x_true=self.x[self.ids].clone(), rot_true=eye3.clone(),
                        P=(1e-9 * torch.eye(16, **f64)).repeat(rows, 1, 1).contiguous(),
                        u_goal=torch.full((rows, 4), hover, **f64),
                        p_goal=torch.from_numpy(np.ascontiguousarray(pg[ids])).to(self.dev))
        self.g = {k: torch.from_numpy(np.ascontiguousarray(gains[k], np.float64)).to(self.dev)
                  for k in ("L", "E", "Lh", "Eh")}
        self.g["l"] = torch.from_numpy(np.ascontiguousarray(gains.get("l", np.zeros(4)), np.float64)).to(self.dev)
        self.M = 1e-9 * torch.eye(16, **f64)
        self.Nz = 1e-9 * torch.eye(6, **f64)
        self.model_d = torch.frombuffer(bytearray(bytes(self.model)), dtype=torch.uint8).to(self.dev)
        self.nrm = None
        self._nrm_host = None   # the next update's noise draws, pinned (drawn while the GPU runs)
        self.t = 0

    def _sid(self):
        return self.stream.cuda_stream

    def set_obstacles(self, states, xy_radius=None, z_radius=None, responsibility=1.0):
        """This rank's context takes the obstacle set (every rank the same
        arguments: scalars, or one value per obstacle); a device tensor is
        read by every later step."""
        self.ctx.set_obstacles(states, xy_radius, z_radius, responsibility)

    def set_hard_planes(self, level: int):
        """This rank's context takes the hardness level (every rank the same;
        Context.set_hard_planes)."""
        self.ctx.set_hard_planes(level)

    def set_active(self, mask):
        """This rank's context takes the activity mask (every rank the same
        global array; Context.set_active).  It governs step() alone: update()
        goes on propagating every own agent."""
        self.ctx.set_active(mask)

    def set_interaction(self, cls, share, device=False):
        """This rank's context takes the interaction classes (every rank the
        same global class array and table; Context.set_interaction)."""
        self.ctx.set_interaction(cls, share, device=device)

    def monitor(self, reset: bool = False):
        """This rank's (last, since_reset) clearance totals (Context.monitor);
        merge_clearance joins the ranks'."""
        return self.ctx.monitor(reset)

    def lp_audit(self, reset: bool = False):
        """This rank's (last, since_reset) LP-audit totals (Context.lp_audit);
        merge_lp_audit joins the ranks'."""
        return self.ctx.lp_audit(reset)

    def predict(self):
        """The horizon conflict prediction of this rank's rows with the
        velocities the last step() chose, on the loop's stream: an all-gather
        of newV first when there is more than one rank (a row shard does not
        hold the other rows' newV), then Context.predict_device(x, newV)."""
        if self.world > 1:
            with self.torch.cuda.stream(self.stream):
                allgather_rows(self.dist, self.newv, self.rank, self.world, mode=self.mode)
        self.ctx.predict_device(self.x.data_ptr(), self.newv.data_ptr(), 0, self._sid())

    def prediction(self, reset: bool = False):
        """This rank's (last, since_reset) prediction totals
        (Context.prediction); merge_prediction joins the ranks'."""
        return self.ctx.prediction(reset)

    def step(self, gather: bool = False):
        """The pair loop for the own rows; newV of the own rows on the device
        (all rows with gather=True: one all-gather of newV)."""
        if self.world > 1 and self.flags & LQRO_FLAG_QHULL_ORDER:
            # the loop-carried normal crosses the shards: the row-normal
            # table's all-gather between the hulls and the LP
            self.ctx.step_device_begin(self.x.data_ptr(), self.vgoal.data_ptr(), self.rowtab.data_ptr(),
                                       self._sid())
            with self.torch.cuda.stream(self.stream):
                allgather_rows(self.dist, self.rowtab, self.rank, self.world, mode=self.mode)
            self.ctx.step_device_end(self.rowtab.data_ptr(), self.newv.data_ptr(), self._sid())
        else:
            self.ctx.step_device(self.x.data_ptr(), self.vgoal.data_ptr(), self.newv.data_ptr(), self._sid())
        if gather and self.world > 1:
            with self.torch.cuda.stream(self.stream):
                allgather_rows(self.dist, self.newv, self.rank, self.world, mode=self.mode)
        if self.predict_each:
            if gather and self.world > 1:   # (newV is whole already)
                self.ctx.predict_device(self.x.data_ptr(), self.newv.data_ptr(), 0, self._sid())
            else:
                self.predict()
        return self.newv

    def own_rows(self, t):
        """The own rows of an (N, k) tensor, in row order."""
        return t[self.rb:self.re] if self.mode == "block" else t[self.ids]

    def update(self):
        """LQRO:1437-1446 for the own rows, then the all-gather of x."""
        torch = self.torch
        rb, re = self.rb, self.re
        block = self.mode == "block"
        if self._nrm_host is None:
            self._nrm_host = self._draw_normals()
        with torch.cuda.stream(self.stream):
            # pinned + non-blocking: no host wait on the stream's earlier work
            self.nrm = self._nrm_host.to(self.dev, non_blocking=True)
            if block:
                self.vgoal[rb:re].copy_(self.newv[rb:re])      # vGoal = newV (LQRO:1438)
                xs, vs = self.x[rb:re], self.vgoal[rb:re]
            else:                                              # cyclic rows: contiguous copies
                xs = self.x.index_select(0, self.ids)
                vs = self.newv.index_select(0, self.ids)
        o, g = self.own, self.g
        a = Agents(xs.data_ptr(), o["rot"].data_ptr(), o["x_true"].data_ptr(), o["rot_true"].data_ptr(),
                   o["P"].data_ptr(), vs.data_ptr(), None, o["u_goal"].data_ptr(), o["p_goal"].data_ptr(),
                   g["L"].data_ptr(), g["E"].data_ptr(), g["l"].data_ptr(), g["Lh"].data_ptr(),
                   g["Eh"].data_ptr(), self.M.data_ptr(), self.Nz.data_ptr(), self.nrm.data_ptr())
        a.time = self.t * self.model.dt
        _check(lib().lqro_dynamics_step_device(C.c_void_p(self.model_d.data_ptr()), 1, len(self.ids_h), 0,
                                               C.byref(a), C.c_void_p(self._sid() or None)),
               "lqro_dynamics_step_device")
        with torch.cuda.stream(self.stream):
            if not block:
                self.x.index_copy_(0, self.ids, xs)
                self.vgoal.index_copy_(0, self.ids, vs)
            if self.world > 1:
                allgather_rows(self.dist, self.x, self.rank, self.world, mode=self.mode)
        self.t += 1
        # the next step's draws (the reference's rand() stream, in agent order)
        # on the host while this step's kernels run
        self._nrm_host = self._draw_normals()

    def _draw_normals(self):
        nrm, self.seed = normals(self.seed, self.n * NORMALS_PER_AGENT)
        host = self.torch.from_numpy(np.ascontiguousarray(nrm.reshape(self.n, NORMALS_PER_AGENT)[self.ids_h]))
        return host.pin_memory()

    def close(self):
        self.ctx.close()
