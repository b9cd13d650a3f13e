#!/usr/bin/env python3
"""Golden fixture: the reference's calculateNewV (LQRO:1223-1234) on the
directed LP families of tests/lp_cases.py — exactly and nearly parallel
planes, planes at the speed limit, zero normals, subnormal squares, and
twelve rows with subnormal coordinates (lp_cases.fixture_rows) — and on
six long rows that sit on both sides of every switch of launch_lp's plane
layouts (lp_cases.LONG_SIZES).

TEST INFRASTRUCTURE, build container (needs oracle/_ref/libref.so).  Every
row goes through ref_newv; nothing is written if the oracle disagrees
anywhere or a result is not finite.  Writes tests/golden/lp_edges.npz:
planes float32 [P, 6], offsets [R + 1], vgoal [R, 3], family [R] (index into
families), newv [R, 3] for the edge cases; for the long rows only long_m,
long_seed, long_newv and the SHA-256 of each regenerated row (long_sha), so
that a test can tell a drifted generator from a wrong LP.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import pyoracle  # noqa: E402
import lp_cases  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_newv(r, c, g):
    c = np.ascontiguousarray(c, np.float32).reshape(-1, 6)
    g = np.ascontiguousarray(g, np.float64)
    out = np.zeros(3)
    r.ref_newv(c.shape[0], _p(c), _p(g), _p(out))
    return out


def main():
    r = pyoracle.reflib()
    if r is None:
        sys.exit("oracle/_ref/libref.so is needed")
    cases, goals, names = lp_cases.fixture_rows()
    fams = lp_cases.FAMILIES + ("subnormal",)
    longs = [lp_cases.long_row(m, m) for m in lp_cases.LONG_SIZES]
    out = []
    for c, g in list(zip(cases, goals)) + longs:
        v = ref_newv(r, c, g)
        o = pyoracle.newv(c, g)
        if not np.array_equal(v.view(np.uint64), o.view(np.uint64)):
            sys.exit(f"oracle != ref_newv on row {len(out)} ({len(c)} planes): {o} {v}")
        if not np.isfinite(v).all():
            sys.exit(f"row {len(out)}: {v}")
        out.append(v)
    out = np.array(out)
    n = len(cases)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(c) for c in cases])
    # plain savez of a fixed key order: the same bytes on every run
    path = os.path.join(HERE, "lp_edges.npz")
    np.savez_compressed(
        path, planes=np.concatenate(cases).astype(np.float32), offsets=offs, vgoal=goals,
        family=np.array([fams.index(f) for f in names], np.int8),
        families=np.array(fams), newv=out[:n],
        long_m=np.array(lp_cases.LONG_SIZES, np.int64), long_seed=np.array(lp_cases.LONG_SIZES, np.int64),
        long_newv=out[n:], long_sha=np.array([lp_cases.digest(c, g) for c, g in longs]))
    print(n, "edge rows,", int(offs[-1]), "planes,", len(longs), "long rows,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
