"""The LP audit restated in numpy (lqro.h's contract): float32,
elementwise, every operation rounded once in the order the header states, so
liblqro.so's kernels match it bit for bit.  tests/test_lp_audit_cpu.py pins it
to a plain scalar loop over np.float32 scalars.

A row's list is a dict: planes (m, 6) float32 (point, normal), n_hard (as
given: the audit clamps it), kind (m,), id (m,)."""
import numpy as np

F = np.float32
NINF = F(-np.inf)
FENCE, USER, COLUMN = 0, 1, 2
ROW_DTYPE = np.dtype([("viol_max", "<f4"), ("hard_viol_max", "<f4"), ("v2", "<f4"), ("dv2", "<f4"),
                      ("i", "<i4"), ("m", "<i4"), ("n_hard", "<i4"), ("n_viol", "<i4"), ("n_viol_tol", "<i4"),
                      ("n_hard_viol", "<i4"), ("k_viol", "<i4"), ("kind_viol", "<i4"), ("id_viol", "<i4"),
                      ("k_hard", "<i4"), ("kind_hard", "<i4"), ("id_hard", "<i4")])
MAXIMA = (("viol_max", ("viol_i", "viol_k", "viol_kind", "viol_id")),
          ("hard_viol_max", ("hard_i", "hard_k", "hard_kind", "hard_id")),
          ("dv2_max", ("dv2_i",)))
COUNTS = ("n_rows_viol", "n_rows_hard_viol", "n_viol_tol", "n_planes")


# ---- the list a row's LP saw ----------------------------------------------
def fence_planes(x, lo, hi, tau, m=(0.26, 0.26, 0.75)):
    """((N, faces, 6) float32, [face index 2 a + side of each emitted face]):
    lqro_set_fence's planes, the bound in fp64 in the header's order, rounded
    once; a face at infinity is not emitted."""
    x = np.asarray(x, np.float64)
    out, faces = [], []
    for a in range(3):
        for side, b in ((0, lo[a]), (1, hi[a])):
            if np.isinf(b):
                continue
            p = np.zeros((x.shape[0], 6), np.float32)
            bound = (np.float64(b) + np.float64(m[a])) if side == 0 else (np.float64(b) - np.float64(m[a]))
            p[:, a] = ((bound - x[:, a]) / np.float64(tau)).astype(np.float32)
            p[:, 3 + a] = 1.0 if side == 0 else -1.0
            out.append(p)
            faces.append(2 * a + side)
    return (np.stack(out, 1) if out else np.zeros((x.shape[0], 0, 6), np.float32)), faces


def plain_lists(plane_lists, n_hard=None):
    """lqro_audit_new_v's lists: every plane LQRO_AUDIT_USER with id = k."""
    out = []
    for r, p in enumerate(plane_lists):
        p = np.asarray(p, np.float32).reshape(-1, 6)
        k = np.arange(len(p), dtype=np.int32)
        out.append(dict(planes=p, n_hard=0 if n_hard is None else int(n_hard[r]), kind=np.full(len(p), USER, np.int32),
                        id=k))
    return out


def assemble(recs, row_ids, n_agents, level=0, fence=None, faces=(), user=None):
    """The step's lists from its records (LQRO_FLAG_RECORDS; nrows x npr, slot
    order: with culling the neighbour list's order), per own row: the emitted
    fence faces (fence[i], ids `faces`), agent i's live user planes (user[i]),
    then the slots whose record has a plane (LQRO_REC_PLANE, bit 0), a
    column's id the record's j; at level 3 the obstacle columns
    (j >= n_agents) ahead of the agents'.  n_hard from the level."""
    row_ids = list(row_ids)
    rows = recs.reshape(len(row_ids), -1)
    none = np.zeros((0, 6), np.float32)
    out = []
    for r, i in zip(rows, row_ids):
        f = np.asarray(fence[i], np.float32).reshape(-1, 6) if fence is not None else none
        u = np.asarray(user[i], np.float32).reshape(-1, 6) if user is not None else none
        has = (r["flags"] & 1) != 0
        pl = np.concatenate([r["plane_point"], r["plane_normal"]], 1).astype(np.float32)
        ob = r["j"] >= n_agents
        order = np.nonzero(has)[0]
        if level >= 3:
            order = np.concatenate([np.nonzero(has & ob)[0], np.nonzero(has & ~ob)[0]])
            n_hard = len(f) + len(u) + int((has & ob).sum())
        else:
            n_hard = (0, len(f), len(f) + len(u))[level]
        planes = np.concatenate([f, u, pl[order]])
        kind = np.concatenate([np.full(len(f), FENCE), np.full(len(u), USER), np.full(len(order), COLUMN)])
        ids = np.concatenate([np.asarray(faces, np.int64)[:len(f)], np.arange(len(u)), r["j"][order]])
        out.append(dict(planes=planes, n_hard=n_hard, kind=kind.astype(np.int32), id=ids.astype(np.int32)))
    return out


# ---- the audit --------------------------------------------------------------
def _first_max(val, valid, tie):
    """Per row (value, k) of the maximum of val where valid; tie: which of the
    equal maxima wins — "lowest" k is the contract; "highest" and "lane_ge"
    (the highest k within a lane k % 64, the lowest lane's candidate across
    lanes: a >= in the lane's running maximum) are wrong rules the tests show
    their inputs tell apart."""
    R, M = val.shape
    w = np.where(valid, val, NINF)
    if M == 0:
        return np.full(R, NINF), np.full(R, -1, np.int32)
    any_ = valid.any(axis=1)
    if tie == "lowest":
        k = np.argmax(w, axis=1)
    else:
        mx = w.max(axis=1)
        eq = valid & (w == mx[:, None])
        if tie == "highest":
            k = M - 1 - np.argmax(eq[:, ::-1], axis=1)
        else:
            kk = np.arange(M)
            cand = eq.copy()
            for r in range(R):
                ks = kk[eq[r]]
                keep = {}
                for q in ks:
                    keep[q % 64] = q
                cand[r] = False
                cand[r, list(keep.values())] = True
            k = np.argmax(cand, axis=1)
    v = np.where(any_, w[np.arange(R), k], NINF).astype(np.float32)
    return v, np.where(any_, k, -1).astype(np.int32)


def rows(lists, newv, vgoal, tol, row_ids=None, tie="lowest"):
    """The records of the own rows `row_ids` (global agent ids; default 0 ..),
    lists[r] the list of row_ids[r]; newv, vgoal: (n_agents, 3) float64."""
    R = len(lists)
    row_ids = np.arange(R) if row_ids is None else np.asarray(row_ids, np.int64)
    tol = F(tol)
    M = max([len(c["planes"]) for c in lists], default=0)
    P = np.zeros((R, M, 6), np.float32)
    kind = np.full((R, M), -1, np.int32)
    ids = np.full((R, M), -1, np.int32)
    m = np.array([len(c["planes"]) for c in lists], np.int32)
    for r, c in enumerate(lists):
        P[r, :m[r]] = c["planes"]
        kind[r, :m[r]] = c["kind"]
        ids[r, :m[r]] = c["id"]
    n_hard = np.minimum(np.array([c["n_hard"] for c in lists], np.int64), m).astype(np.int32)
    v = np.asarray(newv, np.float64)[row_ids].astype(np.float32)
    pref = np.asarray(vgoal, np.float64)[row_ids].astype(np.float32)
    kk = np.arange(M)[None, :]
    valid = kk < m[:, None]
    hard = kk < n_hard[:, None]
    # viol_k = n.x (p.x - v.x) + n.y (p.y - v.y) + n.z (p.z - v.z), left to right
    with np.errstate(all="ignore"):
        t0 = P[:, :, 3] * (P[:, :, 0] - v[:, None, 0])
        t1 = P[:, :, 4] * (P[:, :, 1] - v[:, None, 1])
        t2 = P[:, :, 5] * (P[:, :, 2] - v[:, None, 2])
        viol = (t0 + t1) + t2
    assert viol.dtype == np.float32
    out = np.zeros(R, ROW_DTYPE)
    out["i"], out["m"], out["n_hard"] = row_ids, m, n_hard
    out["v2"] = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    d = v - pref
    out["dv2"] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    out["n_viol"] = (valid & (viol > F(0.0))).sum(axis=1)
    out["n_viol_tol"] = (valid & (viol > tol)).sum(axis=1)
    out["n_hard_viol"] = (hard & (viol > tol)).sum(axis=1)
    ar = np.arange(R)
    for val, k, kd, idn, mask in (("viol_max", "k_viol", "kind_viol", "id_viol", valid),
                                  ("hard_viol_max", "k_hard", "kind_hard", "id_hard", hard)):
        vm, km = _first_max(viol, mask, tie)
        out[val], out[k] = vm, km
        if M:
            out[kd] = np.where(km >= 0, kind[ar, np.maximum(km, 0)], -1)
            out[idn] = np.where(km >= 0, ids[ar, np.maximum(km, 0)], -1)
        else:
            out[kd] = out[idn] = -1
    return out


def empty_total():
    t = {n: -1 for _, idx in MAXIMA for n in idx}
    t.update({v: NINF for v, _ in MAXIMA})
    t.update({k: 0 for k in COUNTS})
    t["n_measured"] = 0
    return t


def _better(v, key, bv, bkey):
    return v > bv or (v == bv and key < bkey)


def total(rws):
    """One audit's total: per maximum the largest value, then the smallest i,
    then the smallest k; a -inf maximum has indices -1."""
    t = empty_total()
    for (v, idx), (rv, cols) in zip(MAXIMA, (("viol_max", ("i", "k_viol", "kind_viol", "id_viol")),
                                           ("hard_viol_max", ("i", "k_hard", "kind_hard", "id_hard")),
                                           ("dv2", ("i",)))):
        best = None
        for r in rws:
            val = F(r[rv])
            if not val > NINF:
                continue
            key = (int(r["i"]), int(r[cols[1]]) if len(cols) > 1 else 0)
            if best is None or _better(val, key, best[0], best[1]):
                best = (val, key, r)
        if best is not None:
            t[v] = best[0]
            for n, c in zip(idx, cols):
                t[n] = int(best[2][c])
    t["n_rows_viol"] = int((rws["n_viol_tol"] > 0).sum())
    t["n_rows_hard_viol"] = int((rws["n_hard_viol"] > 0).sum())
    t["n_viol_tol"] = int(rws["n_viol_tol"].astype(np.int64).sum())
    t["n_planes"] = int(rws["m"].astype(np.int64).sum())
    t["n_measured"] = 1
    return t


def fold(since, last):
    """The since-reset total after one more audit: a strictly larger maximum
    replaces the kept one (the earliest audit keeps a tie); counts add."""
    s = dict(since)
    for v, idx in MAXIMA:
        if F(last[v]) > F(s[v]):
            s[v] = last[v]
            for n in idx:
                s[n] = last[n]
    for k in COUNTS:
        s[k] += last[k]
    s["n_measured"] += 1
    return s


def same_total(a, b):
    """Two totals (dicts) equal in every field, the floats bit for bit."""
    if set(a) != set(b):
        return False
    for k in a:
        if k.endswith("_max"):
            if np.float32(a[k]).view(np.uint32) != np.float32(b[k]).view(np.uint32):
                return False
        elif int(a[k]) != int(b[k]):
            return False
    return True


def same_rows(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def audit(lists, newv, vgoal, tol, row_ids=None):
    """(rows, total) as lqro_audit_new_v and the step's audit return them."""
    r = rows(lists, newv, vgoal, tol, row_ids)
    return r, total(r)
