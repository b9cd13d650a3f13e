"""The horizon conflict prediction restated in numpy (lqro.h's contract,
DESIGN §6.17): fp64, every operation rounded once, sums taken in ascending
index order starting from 0.0, so liblqro.so's kernels match it bit for bit.
tests/test_predict_cpu.py pins it to pyoracle.tables and to a plain scalar
Python loop over the same formulas.

Tables, for each gains set: At = A + (B L), Bt = B E, G <- 0, then H times
G <- (sum_m At[r][m] G[m][c]) + Bt[r][c]; CG_k is rows 0..2 of G after update
k + 1 (slice k: the state k + 1 steps ahead, the index of T_k and NCF_k).
Path of body b with velocity v_b: P_b,k[r] = (sum_c CG_k[r][c] v_b[c]) -
(sum_m NCF_k[r][m] x_b[m]); an agent uses its own set, an obstacle in row i
uses row i's tables and v_o = x_o[3..5]; the affine terms c and l are left out.
Pair (row i, column c, slice k), d = P_i,k - P_c,k: q = dx dx + dy dy,
d2 = q + dz dz, s2 = q wxy_c + (dz dz) wz_c with the clearance monitor's
weights; a hit is s2 < 1.0, strictly; self is skipped by index; an inactive
agent is neither a row nor a column (its row gets the cleared record)."""
import numpy as np

from clearance_ref import weights  # noqa: F401  (the summed-radii weights, §6.14)

ROW_DTYPE = np.dtype([("s2_min", "<f8"), ("d2_min", "<f8"), ("j_s2", "<i4"), ("k_s2", "<i4"), ("j_d2", "<i4"),
                      ("k_d2", "<i4"), ("k_first", "<i4"), ("j_first", "<i4"), ("n_conf", "<i4"), ("reserved", "<i4"),
                      ("conf", "<i4", (4,))])
INF = float("inf")


def _ordered_matmul(a, b):
    """sum_m a[r][m] b[m][c], m ascending from 0.0."""
    out = np.zeros((a.shape[0], b.shape[1]))
    for m in range(a.shape[1]):
        out = out + a[:, m:m + 1] * b[m:m + 1, :]
    return out


def tables(A, B, L, E, H):
    """(CG, NCF) of one gains set: (H, 3, 3) and (H, 3, X), k_tables' recursion."""
    A, B, L, E = (np.asarray(v, np.float64) for v in (A, B, L, E))
    X = A.shape[0]
    At = A + _ordered_matmul(B, L)
    Bt = _ordered_matmul(B, E)
    F, G = np.eye(X), np.zeros((X, 3))
    negC = np.full((3, X), -0.0)
    negC[np.arange(3), np.arange(3)] = -1.0
    CG, NCF = np.zeros((H, 3, 3)), np.zeros((H, 3, X))
    for k in range(H):
        F = _ordered_matmul(At, F)
        G = _ordered_matmul(At, G) + Bt
        NCF[k] = _ordered_matmul(negC, F)
        CG[k] = G[:3]
    return CG, NCF


def table_sets(A, B, L, E, H):
    """(CG, NCF) with a leading set axis: one set, or one per agent (L: (N, U, X))."""
    L, E = np.asarray(L, np.float64), np.asarray(E, np.float64)
    if L.ndim == 2:
        L, E = L[None], E[None]
    t = [tables(A, B, l, e, H) for l, e in zip(L, E)]
    return np.stack([a for a, _ in t]), np.stack([b for _, b in t])


def body_paths(CG, NCF, x, v):
    """P[b][k][r] for bodies with per-body tables CG (B, H, 3, 3), NCF (B, H, 3, X)."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    s = np.zeros(CG.shape[:3])
    for c in range(3):
        s = s + CG[..., c] * v[:, None, None, c]
    f = np.zeros(CG.shape[:3])
    for m in range(x.shape[1]):
        f = f + NCF[..., m] * x[:, None, None, m]
    return s - f


def agent_paths(CG, NCF, x, v):
    """(N, H, 3): every agent under its own set."""
    n = len(x)
    g = np.arange(n) if CG.shape[0] > 1 else np.zeros(n, np.int64)
    return body_paths(CG[g], NCF[g], x, v)


def obstacle_paths(CG, NCF, row_ids, obs):
    """(rows, M, H, 3): each obstacle under each own row's tables, v_o = x_o[3..5]."""
    obs = np.asarray(obs, np.float64)
    out = np.zeros((len(row_ids), len(obs), CG.shape[1], 3))
    for r, i in enumerate(row_ids):
        g = int(i) if CG.shape[0] > 1 else 0
        out[r] = body_paths(np.broadcast_to(CG[g], (len(obs),) + CG.shape[1:]),
                            np.broadcast_to(NCF[g], (len(obs),) + NCF.shape[1:]), obs, obs[:, 3:6])
    return out


def cleared_row():
    r = np.zeros((), ROW_DTYPE)
    r["s2_min"] = r["d2_min"] = INF
    for f in ("j_s2", "k_s2", "j_d2", "k_d2", "k_first", "j_first"):
        r[f] = -1
    r["conf"] = -1
    return r


def rows(P, n_agents, wxy, wz, row_ids, active=None, obs_paths=None):
    """The row records of the own rows `row_ids`.  P: (columns, H, 3), the
    columns every row shares (agents first); obs_paths: None, or (rows, M, H, 3),
    per-row columns behind them (the predicting calls' obstacles).  active:
    None or n_agents bytes; obstacle columns are never masked."""
    P = np.asarray(P, np.float64)
    row_ids = np.asarray(row_ids, np.int64)
    wxy, wz = np.asarray(wxy, np.float64), np.asarray(wz, np.float64)
    ncols = P.shape[0] + (0 if obs_paths is None else obs_paths.shape[1])
    on = np.ones(ncols, bool)
    if active is not None:
        on[:n_agents] = np.asarray(active)[:n_agents] != 0
    out = np.zeros(len(row_ids), ROW_DTYPE)
    for r, i in enumerate(row_ids):
        out[r] = cleared_row()
        if not on[i]:
            continue
        cols = P if obs_paths is None else np.concatenate([P, obs_paths[r]])
        d = P[i][None] - cols                       # (columns, H, 3)
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        q = dx * dx + dy * dy
        zz = dz * dz
        d2 = q + zz
        s2 = q * wxy[:ncols, None] + zz * wz[:ncols, None]
        valid = on.copy()
        valid[i] = False                            # self by index, never by distance
        if not valid.any():
            continue
        H = s2.shape[1]
        s2m = np.where(valid[:, None], s2, INF)
        d2m = np.where(valid[:, None], d2, INF)
        a, b = int(s2m.argmin()), int(d2m.argmin())   # (C order: the smallest (column, slice) of equals)
        out[r]["s2_min"], out[r]["j_s2"], out[r]["k_s2"] = s2m.flat[a], a // H, a % H
        out[r]["d2_min"], out[r]["j_d2"], out[r]["k_d2"] = d2m.flat[b], b // H, b % H
        hit = (s2 < 1.0) & valid[:, None]
        cc = np.nonzero(hit.any(axis=1))[0]
        out[r]["n_conf"] = len(cc)
        out[r]["conf"][:min(4, len(cc))] = cc[:4]
        if len(cc):
            kf = int(np.nonzero(hit.any(axis=0))[0][0])
            out[r]["k_first"], out[r]["j_first"] = kf, int(np.nonzero(hit[:, kf])[0][0])
    return out


def empty_total():
    return dict(s2_min=INF, d2_min=INF, s2_i=-1, s2_j=-1, s2_k=-1, d2_i=-1, d2_j=-1, d2_k=-1, first_k=-1, first_i=-1,
                first_j=-1, reserved=0, n_conf=0, n_rows_conf=0, n_measured=0)


def total(rws, row_ids):
    """One measurement's total: the smallest (value, i, j, k) per minimum, the
    smallest (k, i, j) first hit."""
    t = empty_total()
    for v, j, k in (("s2", "j_s2", "k_s2"), ("d2", "j_d2", "k_d2")):
        keys = [(float(r[v + "_min"]), int(i), int(r[j]), int(r[k])) for r, i in zip(rws, row_ids)
                if float(r[v + "_min"]) < INF]
        if keys:
            t[v + "_min"], t[v + "_i"], t[v + "_j"], t[v + "_k"] = min(keys)
    keys = [(int(r["k_first"]), int(i), int(r["j_first"])) for r, i in zip(rws, row_ids) if r["k_first"] >= 0]
    if keys:
        t["first_k"], t["first_i"], t["first_j"] = min(keys)
    t["n_conf"] = int(rws["n_conf"].astype(np.int64).sum())
    t["n_rows_conf"] = int((rws["n_conf"] > 0).sum())
    t["n_measured"] = 1
    return t


def fold(since, last):
    """The since-reset total after one more measurement: a strictly smaller
    value replaces the kept one (the earliest measurement keeps a tie)."""
    s = dict(since)
    for v in ("s2", "d2"):
        if last[v + "_min"] < s[v + "_min"]:
            for f in ("_min", "_i", "_j", "_k"):
                s[v + f] = last[v + f]
    if last["first_k"] >= 0 and (s["first_k"] < 0 or last["first_k"] < s["first_k"]):
        s["first_k"], s["first_i"], s["first_j"] = last["first_k"], last["first_i"], last["first_j"]
    s["n_conf"] += last["n_conf"]
    s["n_rows_conf"] += last["n_rows_conf"]
    s["n_measured"] += 1
    return s


def predict(x, v, gains, H, xy_radius, z_radius, row_ids=None, obs=None, obs_xy=(), obs_z=(), active=None):
    """(rows, total, paths) as lqro_predict returns them; gains: dict with A,
    B, L, E (L, E with a leading agent axis for per-agent gains)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    row_ids = np.arange(n) if row_ids is None else np.asarray(row_ids)
    CG, NCF = table_sets(gains["A"], gains["B"], gains["L"], gains["E"], H)
    P = agent_paths(CG, NCF, x, v)
    op = None
    if obs is not None and len(obs):
        op = obstacle_paths(CG, NCF, row_ids, obs)
    else:
        obs_xy, obs_z = (), ()
    wxy, wz = weights(n, xy_radius, z_radius, obs_xy, obs_z)
    r = rows(P, n, wxy, wz, row_ids, active, op)
    return r, total(r, row_ids), P


def predict_paths(paths, n_agents, xy_radius, z_radius, row_ids=None, obs_xy=(), obs_z=(), active=None):
    """(rows, total) as lqro_predict_paths returns them; paths: (N + M, H, 3)."""
    row_ids = np.arange(n_agents) if row_ids is None else np.asarray(row_ids)
    wxy, wz = weights(n_agents, xy_radius, z_radius, obs_xy, obs_z)
    r = rows(paths, n_agents, wxy, wz, row_ids, active)
    return r, total(r, row_ids)


def pair_s2(P, wxy, wz):
    """s2[i][c][k] of every ordered pair of the shared columns P (the link to
    the method, tests/test_predict_cpu.py)."""
    P = np.asarray(P, np.float64)
    d = P[:, None] - P[None, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    q = dx * dx + dy * dy
    return q * np.asarray(wxy)[None, :, None] + (dz * dz) * np.asarray(wz)[None, :, None]
