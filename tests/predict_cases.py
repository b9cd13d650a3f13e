"""Inputs shared by tests/test_predict_cpu.py and tests/test_gpu_predict.py."""
import numpy as np

import clearance_cases as cc
from clearance_cases import same_rows, same_total, states  # noqa: F401

TR, CHUNK = 8, 256       # k_conf: own rows a workgroup, columns a pass (lqro_kern_predict.hip)
LATTICE_RADII = cc.LATTICE_RADII


def lattice_paths(h, scaled_slice=None):
    """(64, h, 3): clearance_cases' 4 x 4 x 4 lattice translating rigidly by
    (0.25, 0, 0) a slice (every axis neighbour at s2 == 1.0 in every slice,
    exactly); with scaled_slice the lattice of that slice is scaled by 0.75
    (axis neighbours at 0.5625, diagonals at 1.125)."""
    p = np.zeros((64, h, 3))
    for k in range(h):
        p[:, k] = cc.lattice(0.75 if k == scaled_slice else 1.0)
        p[:, k, 0] += 0.25 * k
    return p


def random_paths(ncols, h, seed, clusters=3, per_cluster=3):
    """(ncols, h, 3): straight paths from random starts with random
    velocities, the first clusters x per_cluster bodies (where ncols has room
    for them) starting within 0.1 m of a common centre so that hits exist."""
    rng = np.random.default_rng(seed)
    side = 2.0 * ncols ** (1.0 / 3.0)
    p0 = (rng.random((ncols, 3)) - 0.5) * side
    v = (rng.random((ncols, 3)) - 0.5) * 2.0
    for c in range(clusters):
        step = max(1, (ncols - 1) // per_cluster)   # (a cluster's bodies spread over the lanes and passes)
        ids = np.unique((2 * c + np.arange(per_cluster) * step) % ncols)
        p0[ids] = p0[ids[0]] + (rng.random((len(ids), 3)) - 0.5) * 0.1
        v[ids] = v[ids[0]] + (rng.random((len(ids), 3)) - 0.5) * 0.05
    t = 0.1 * (np.arange(h) + 1.0)
    return p0[:, None, :] + t[None, :, None] * v[:, None, :]


def row_windows(n):
    """Own-row ranges of TR - 1, TR and TR + 1 rows around the lanes 0 and
    CHUNK - 1 of every column pass, and every row."""
    tr, ch = TR, CHUNK
    out = {(0, n)}
    for b, k in ((0, tr - 1), (0, tr), (0, tr + 1), (ch - tr + 1, tr - 1), (ch - 4, tr), (ch - 4, tr + 1),
                 (2 * ch - tr, tr), (2 * ch - tr, tr + 1), (n - tr + 1, tr - 1)):
        if b >= 0 and b + k <= n:
            out.add((b, b + k))
    return sorted(out)


def scalar_rows(P, wxy, wz, row_ids, row_dtype, active=None, n_agents=None):
    """lqro.h's pair formulas and tie rules as a plain loop over Python floats
    (P: (columns, H, 3), columns every row shares)."""
    P = [[[float(v) for v in s] for s in b] for b in np.asarray(P)]
    wxy, wz = [float(v) for v in wxy], [float(v) for v in wz]
    inf = float("inf")
    n_agents = len(P) if n_agents is None else n_agents
    on = [True] * len(P)
    if active is not None:
        for c in range(n_agents):
            on[c] = bool(active[c])
    out = np.zeros(len(row_ids), row_dtype)
    for r, i in enumerate(int(v) for v in row_ids):
        s2m, d2m, js, ks, jd, kd, kf, jf, conf = inf, inf, -1, -1, -1, -1, -1, -1, []
        for c in range(len(P)):
            if c == i or not on[c] or not on[i]:
                continue
            any_hit = False
            for k in range(len(P[c])):
                dx = P[i][k][0] - P[c][k][0]
                dy = P[i][k][1] - P[c][k][1]
                dz = P[i][k][2] - P[c][k][2]
                q = dx * dx + dy * dy
                zz = dz * dz
                d2 = q + zz
                s2 = q * wxy[c] + zz * wz[c]
                if s2 < s2m:
                    s2m, js, ks = s2, c, k
                if d2 < d2m:
                    d2m, jd, kd = d2, c, k
                if s2 < 1.0:
                    any_hit = True
                    if kf < 0 or k < kf:
                        kf, jf = k, c
            if any_hit:
                conf.append(c)
        out[r] = (s2m, d2m, js, ks, jd, kd, kf, jf, len(conf), 0, (conf[:4] + [-1] * 4)[:4])
    return out
