"""The clearance measurement restated in numpy (lqro.h's contract, DESIGN
§6.14): fp64, elementwise, every operation rounded once in the order the
header states, so liblqro.so's kernels match it bit for bit.
tests/test_clearance_cpu.py pins it to a plain scalar Python loop over the same
formulas."""
import numpy as np

ROW_DTYPE = np.dtype([("s2_min", "<f8"), ("d2_min", "<f8"), ("fence_min", "<f8"), ("j_s2", "<i4"), ("j_d2", "<i4"),
                      ("n_hit", "<i4"), ("fence_face", "<i4"), ("hit", "<i4", (6,))])
INF = float("inf")


def weights(n_agents, xy_radius, z_radius, obs_xy=(), obs_z=()):
    """(wxy, wz) per column: 1 / a^2 and 1 / b^2 over the summed radii, the
    agents' own radii for an agent column."""
    rxy = np.concatenate([np.full(n_agents, float(xy_radius)), np.asarray(obs_xy, np.float64).reshape(-1)])
    rz = np.concatenate([np.full(n_agents, float(z_radius)), np.asarray(obs_z, np.float64).reshape(-1)])
    a = np.float64(xy_radius) + rxy
    b = np.float64(z_radius) + rz
    return 1.0 / (a * a), 1.0 / (b * b)


def fence_faces(lo, hi, xy_radius, z_radius):
    """[(face index, axis, side, bound)] of the emitted faces, in face order."""
    if lo is None or hi is None:
        return []
    m = (xy_radius, xy_radius, z_radius)
    out = []
    for a in range(3):
        if np.isfinite(lo[a]):
            out.append((2 * a, a, 0, np.float64(lo[a]) + np.float64(m[a])))
        if np.isfinite(hi[a]):
            out.append((2 * a + 1, a, 1, np.float64(hi[a]) - np.float64(m[a])))
    return out


def rows(pos, wxy, wz, row_ids, faces=()):
    """The row records of the own rows `row_ids` (agents) against every column
    of pos ((n_agents + M, 3): the agents' positions, then the obstacles')."""
    pos = np.ascontiguousarray(pos, np.float64)
    row_ids = np.asarray(row_ids, np.int64)
    ncols = pos.shape[0]
    p = pos[row_ids]
    dx = p[:, None, 0] - pos[None, :, 0]
    dy = p[:, None, 1] - pos[None, :, 1]
    dz = p[:, None, 2] - pos[None, :, 2]
    q = dx * dx + dy * dy
    zz = dz * dz
    d2 = q + zz
    s2 = q * wxy[None, :] + zz * wz[None, :]
    self_ = np.arange(ncols)[None, :] == row_ids[:, None]      # self by index, never by distance
    out = np.zeros(len(row_ids), ROW_DTYPE)
    s2m = np.where(self_, INF, s2)
    d2m = np.where(self_, INF, d2)
    out["s2_min"] = s2m.min(axis=1) if ncols else INF
    out["d2_min"] = d2m.min(axis=1) if ncols else INF
    out["j_s2"] = np.where(out["s2_min"] < INF, s2m.argmin(axis=1), -1)   # (argmin: the smallest column of equals)
    out["j_d2"] = np.where(out["d2_min"] < INF, d2m.argmin(axis=1), -1)
    hit = (s2 < 1.0) & ~self_
    out["n_hit"] = hit.sum(axis=1)
    out["hit"] = -1
    for r in range(len(row_ids)):
        h = np.nonzero(hit[r])[0][:6]
        out["hit"][r, :len(h)] = h
    fm = np.full(len(row_ids), INF)
    ff = np.full(len(row_ids), -1, np.int32)
    for face, a, side, bound in faces:        # face order: the lowest index wins a tie
        g = p[:, a] - bound if side == 0 else bound - p[:, a]
        take = g < fm
        fm = np.where(take, g, fm)
        ff = np.where(take, face, ff)
    out["fence_min"] = fm
    out["fence_face"] = ff
    return out


def empty_total():
    return dict(s2_min=INF, d2_min=INF, fence_min=INF, s2_i=-1, s2_j=-1, d2_i=-1, d2_j=-1, fence_i=-1, fence_face=-1,
                n_hit=0, n_rows_hit=0, n_fence_out=0, n_measured=0)


def total(rws, row_ids):
    """One measurement's total: the smallest (value, i, j) per minimum."""
    t = empty_total()
    for v, a, b, col in (("s2_min", "s2_i", "s2_j", "j_s2"), ("d2_min", "d2_i", "d2_j", "j_d2"),
                         ("fence_min", "fence_i", "fence_face", "fence_face")):
        keys = [(float(r[v]), int(i), int(r[col])) for r, i in zip(rws, row_ids) if float(r[v]) < INF]
        if keys:
            t[v], t[a], t[b] = min(keys)
    t["n_hit"] = int(rws["n_hit"].astype(np.int64).sum())
    t["n_rows_hit"] = int((rws["n_hit"] > 0).sum())
    t["n_fence_out"] = int((rws["fence_min"] < 0).sum())
    t["n_measured"] = 1
    return t


def fold(since, last):
    """The since-reset total after one more measurement: a strictly smaller
    minimum replaces the kept one (the earliest measurement keeps a tie)."""
    s = dict(since)
    for v, a, b in (("s2_min", "s2_i", "s2_j"), ("d2_min", "d2_i", "d2_j"), ("fence_min", "fence_i", "fence_face")):
        if last[v] < s[v]:
            s[v], s[a], s[b] = last[v], last[a], last[b]
    for k in ("n_hit", "n_rows_hit", "n_fence_out"):
        s[k] += last[k]
    s["n_measured"] += 1
    return s


def pairs(rws, row_ids):
    """(i, column) of the rows' hit lists, in (i, column) order."""
    return np.array([(int(i), int(c)) for r, i in zip(rws, row_ids) for c in r["hit"] if c >= 0],
                    np.int64).reshape(-1, 2)


def measure(x, n_agents, xy_radius, z_radius, row_ids=None, obs=None, obs_xy=(), obs_z=(), lo=None, hi=None):
    """(rows, total) of the states x ((n_agents, X)) and obstacle states obs
    ((M, X) or None), as lqro_clearance returns them."""
    x = np.asarray(x, np.float64)
    pos = x[:, :3] if obs is None or len(obs) == 0 else np.concatenate([x[:, :3], np.asarray(obs, np.float64)[:, :3]])
    if obs is None or len(obs) == 0:
        obs_xy, obs_z = (), ()
    wxy, wz = weights(n_agents, xy_radius, z_radius, obs_xy, obs_z)
    row_ids = np.arange(n_agents) if row_ids is None else np.asarray(row_ids)
    r = rows(pos, wxy, wz, row_ids, fence_faces(lo, hi, xy_radius, z_radius))
    return r, total(r, row_ids)
