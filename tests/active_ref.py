"""The activity mask's reference (lqro_set_active): the step over
N agents with mask a IS the oracle's step over the compacted swarm x[a],
vgoal[a].  What is here maps between the two numberings: mask -> ids, a compact
record (i', j') -> the slot of (i, j) in the N-agent context, column ids back.
No GPU, no library: numpy only."""
import numpy as np

# the masks of the issue's table, by name
MASKS = {
    "ends": lambda n: np.array([0 < i < n - 1 for i in range(n)]),       # 0 and n - 1 inactive
    "half": lambda n: np.arange(n) < n // 2,                             # i < n / 2 active
    "mod3": lambda n: np.arange(n) % 3 != 1,                             # i % 3 == 1 inactive
    "odd": lambda n: np.arange(n) % 2 == 1,                              # odd i active
    "all": lambda n: np.ones(n, bool),
}


def mask(name, n):
    return MASKS[name](n).astype(np.uint8)


def ids(a):
    """The active agents' global ids, ascending: compact index -> global id."""
    return np.nonzero(np.asarray(a) != 0)[0]


def compact(a, *arrays):
    """Each per-agent array restricted to the active agents (obstacle rows
    behind the n agents, if any, are kept)."""
    a = np.asarray(a) != 0
    n = len(a)
    out = []
    for v in arrays:
        v = np.asarray(v)
        keep = np.concatenate([a, np.ones(len(v) - n, bool)])
        out.append(np.ascontiguousarray(v[keep]))
    return out if len(out) > 1 else out[0]


def slot(i, j):
    """Column j's slot in row i of a context without culling."""
    return j - (j > i)


def column(i, q):
    """Slot q of row i is column q + (q >= i)."""
    return q + (q >= i)


def global_column(a, jc, n):
    """A compact column id (agents 0..A-1, then obstacles) as the N-agent
    context numbers it (obstacle o is n + o)."""
    g = ids(a)
    return int(g[jc]) if jc < len(g) else n + (jc - len(g))


def expand_records(a, recs_c, n, m=0, rows=None):
    """The compact step's records (A x (A - 1 + m)) as the N-agent context
    returns them: (len(rows), n - 1 + m), rows the context's own (default all
    n).  A slot whose row or column is inactive has i and j set and every
    other field zero; the others are the compact records with their ids
    mapped back.  Returns (records, live) with live the mask of mapped slots."""
    a = np.asarray(a) != 0
    g = ids(a)
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    recs_c = np.asarray(recs_c).reshape(len(g), -1) if len(g) else recs_c
    out = np.zeros((len(rows), n - 1 + m), dtype=recs_c.dtype)
    live = np.zeros(out.shape, bool)
    where = {int(i): k for k, i in enumerate(g)}
    for r, i in enumerate(rows):
        for q in range(n - 1 + m):
            out[r, q]["i"], out[r, q]["j"] = i, column(i, q)
        if i not in where:
            continue
        ic = where[i]
        for qc in range(len(g) - 1 + m):
            jc = column(ic, qc)
            j = global_column(a, jc, n)
            rec = recs_c[ic, qc].copy()
            assert rec["i"] == ic and rec["j"] == jc
            rec["i"], rec["j"] = i, j
            out[r, slot(i, j)] = rec
            live[r, slot(i, j)] = True
    return out, live


def expand_newv(a, nv_c, n):
    """The compact step's newV (A x 3) in the N-agent numbering: +0.0 rows for
    the inactive agents."""
    out = np.zeros((n, 3))
    out[ids(a)] = nv_c
    return out


def pairs(a, m=0, rows=None):
    """stats()["pairs"]: for each active own row the active columns other than
    itself plus the m obstacle columns."""
    a = np.asarray(a) != 0
    rows = range(len(a)) if rows is None else rows
    on = int(a.sum())
    return sum(on - 1 + m for i in rows if a[int(i)])


def park(a, x):
    """Today's workaround: inactive agent k moved to (1e6 (k + 1), -2e6 (k + 1),
    3e6), at rest."""
    x = np.array(x, np.float64)
    for k in np.nonzero(np.asarray(a)[:len(a)] == 0)[0]:
        x[k, 0:3] = (1e6 * (k + 1), -2e6 * (k + 1), 3e6)
        x[k, 3:6] = 0.0
    return x
