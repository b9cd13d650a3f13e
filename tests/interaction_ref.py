"""The interaction classes' reference (lqro_set_interaction):
numpy plus the oracle as it stands.  No pair-local record field depends on the
share, so they come from one `pyoracle.step` without a table; the three fields
that depend on the factor of LQRO:1416 and on the loop-carried normal are redone
in (i, j) order, as `walk` of tests/test_gpu_obstacles.py does, with a factor
per slot:

    a dead slot (row or column inactive, or share[cls_i][cls_j] == 0):
        the zero record with i and j set; skipped
    a live slot with REC_PLANE and without HULLFAIL:
        n = carry if REC_STALE else rec.normal;  carry = n
        d = rec.dist * share[cls_i][cls_j]        (an obstacle column: resp)
        mult = +1 if REC_INSIDE else -1
        point[k] = float32(x[i, 3 + k] + mult * d * n[k]);  plane_normal = float32(n)

and each active row's newV is the oracle's LP (pyoracle.newv) over its walked
planes; an inactive row's is +0.0.  Also here: the pairs statistic and the
issue's tables, by name.  No GPU, no library."""
import numpy as np

CLASSES_MAX = 16

# name: (C, share); the class of agent i is i % C unless a test says otherwise
TABLES = {
    "uniform": (3, np.full((3, 3), 0.5)),
    "ghost": (2, np.array([[0.5, 0.0], [0.0, 0.0]])),
    "priority": (2, np.array([[0.5, 1.0], [0.0, 0.5]])),
    "teams": (3, np.full((3, 3), 0.5) - 0.5 * np.eye(3)),
    "weights": (3, np.array([[0.5, 0.25, 1.0], [0.75, 0.5, 1e-300], [0.0, 1.0, 0.5]])),
}


def table(name):
    """(C, a fresh copy of the C x C share table)."""
    c, sh = TABLES[name]
    return c, np.array(sh, np.float64)


def classes(n, c):
    return (np.arange(n) % c).astype(np.uint8)


def column(i, q):
    """Slot q of row i is column q + (q >= i)."""
    return q + (q >= i)


def factors(cls, share, n, m=0, resp=0.5, active=None, rows=None):
    """(factor, live) per slot, (len(rows), n - 1 + m): the share of the row's
    class against the column's for an agent column, resp (a scalar or one per
    obstacle) for an obstacle column; live: row active, column active, share >
    0 (an obstacle column of an active row is always live)."""
    cls = np.asarray(cls).astype(int)
    share = np.asarray(share, np.float64)
    on = np.ones(n, bool) if active is None else np.asarray(active) != 0
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    resp = np.broadcast_to(np.asarray(resp, np.float64), (m,))
    fac = np.zeros((len(rows), n - 1 + m))
    live = np.zeros(fac.shape, bool)
    for r, i in enumerate(rows):
        for q in range(n - 1 + m):
            j = column(i, q)
            if j >= n:
                fac[r, q], live[r, q] = resp[j - n], on[i]
            else:
                fac[r, q] = share[cls[i], cls[j]]
                live[r, q] = on[i] and on[j] and fac[r, q] > 0.0
    return fac, live


def pairs(cls, share, n, m=0, active=None, rows=None):
    """stats()["pairs"]: for each active own row i the active agents of every
    class b with share[cls_i][b] > 0, minus 1 when share[cls_i][cls_i] > 0,
    plus the m obstacle columns."""
    cls = np.asarray(cls).astype(int)
    share = np.asarray(share, np.float64)
    on = np.ones(n, bool) if active is None else np.asarray(active) != 0
    rows = range(n) if rows is None else rows
    count = np.bincount(cls[on], minlength=share.shape[0])
    total = 0
    for i in rows:
        i = int(i)
        if not on[i]:
            continue
        total += int(sum(count[b] for b in range(share.shape[0]) if share[cls[i], b] > 0.0))
        total -= 1 if share[cls[i], cls[i]] > 0.0 else 0
        total += m
    return total


def walk(lqro, oracle, local, x_all, vg, n, fac, live, carry, head=None, active=None):
    """The module docstring's walk over `local` (all n rows x slots, in (i, j)
    order) with the per-slot factors and liveness of `factors`: (records with
    the walked fields, newV per row, carry out, planes walked per row).
    head[i]: planes ahead of row i's pair planes.  The slots whose normal is
    their own are done at once; only the REC_STALE ones go one by one."""
    exp = local.copy()
    assert exp.shape == live.shape == fac.shape and exp.shape[0] == n
    dead = ~live
    ids = exp[["i", "j"]].copy()
    exp[dead] = np.zeros((), exp.dtype)
    exp["i"][dead], exp["j"][dead] = ids["i"][dead], ids["j"][dead]
    fl = exp["flags"]
    plane = live & ((fl & lqro.REC_PLANE) != 0) & ((fl & lqro.REC_HULLFAIL) == 0)
    flat = np.flatnonzero(plane.reshape(-1))                 # the walked slots, in (i, j) order
    nrm = exp["normal"].reshape(-1, 3)[flat].copy()
    stale = (fl.reshape(-1)[flat] & lqro.REC_STALE) != 0
    carry = np.array(carry, np.float64)
    for p in np.flatnonzero(stale):
        nrm[p] = nrm[p - 1] if p > 0 else carry
    if len(flat):
        carry = nrm[-1].copy()
    inside = (fl.reshape(-1)[flat] & lqro.REC_INSIDE) != 0
    md = np.where(inside, 1.0, -1.0) * (exp["dist"].reshape(-1)[flat] * fac.reshape(-1)[flat])
    rows_of = flat // exp.shape[1]
    pt = (x_all[rows_of, 3:6] + md[:, None] * nrm).astype(np.float32)
    for f, v in (("normal", nrm), ("plane_point", pt), ("plane_normal", nrm.astype(np.float32))):
        col = exp[f].reshape(-1, 3)
        col[flat] = v
        exp[f] = col.reshape(exp[f].shape)
    on = np.ones(n, bool) if active is None else np.asarray(active) != 0
    nv = np.zeros((n, 3))
    count = np.bincount(rows_of, minlength=n)
    six = np.concatenate([pt, nrm.astype(np.float32)], 1)
    for i in range(n):
        if not on[i]:
            continue
        planes = six[rows_of == i]
        if head is not None:
            planes = np.concatenate([np.asarray(head[i], np.float32).reshape(-1, 6), planes])
        nv[i] = oracle.newv(np.ascontiguousarray(planes, np.float32), vg[i], 100.0)
    return exp, nv, carry, count


def stale_from_another_row(lqro, recs, live):
    """The live REC_STALE slots (row, slot) whose carry comes from another row:
    no live plane with a normal of its own ahead of them in their row."""
    out = []
    for r in range(recs.shape[0]):
        own = False
        for q in range(recs.shape[1]):
            if not live[r, q]:
                continue
            fl = int(recs[r, q]["flags"])
            if not (fl & lqro.REC_PLANE) or (fl & lqro.REC_HULLFAIL):
                continue
            if fl & lqro.REC_STALE:
                if not own:
                    out.append((r, q))
            else:
                own = True
    return out
