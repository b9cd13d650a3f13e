#!/usr/bin/env python3
"""Generate tests/golden/dyn.npz and dyn_hard.npz from the REFERENCE's own code.

TEST INFRASTRUCTURE.  Runs only in the build container (needs
oracle/_ref/libref.so, built from /root/reference by oracle/Makefile).  Stores
inputs and the reference's outputs of the per-agent step after the pair loop:

  l                     controlMatrices' l (LQRO:552,557) at hover
  ctl_*                 riccatiControllerSteady (LQRO:594-617) and
                        riccatiControllerSteadyPosition (LQRO:619-645)
  k1_*                  kalmanFilter1 (LQRO:488-505)
  k2_*                  kalmanFilter2 (LQRO:507-518)
  quat_*                quatFromRot (stdafx.h:24-33), Quadrotor::visualize's
                        keyframe orientation (LQRO:128-133)

and tests/golden/dyn_hard.npz: for the hard families of tests/dyn_cases.py
(dense noise covariances, large attitudes; 4 or 8 agents each, default model)
the inputs and the reference's results of one agent step taken function by
function (tests/dyn_hard.py by_function): findU, propagate (LQRO:473-486),
kalmanFilter1, the observation draw (sampleGaussian, simulator2.h:21-32),
kalmanFilter2, findVGoal, sampleGaussian<16> on M itself, and jacobi
(MAT:674-759) of M and N.  The reference's jacobi is built with glibc's hypot
in place of MSVC's _hypot (oracle/ref_harness.cpp).  Not written when the
oracle differs from the reference anywhere.

Usage:  python tests/golden/make_golden_dyn.py
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import pyoracle  # noqa: E402
import dyn_hard  # noqa: E402
from dyn_cases import hard_case, quat_cases, random_agent_cases  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    r = pyoracle.reflib()
    if r is None:
        raise SystemExit("needs oracle/_ref/libref.so (/root/reference)")
    g = pyoracle.synthesize()
    l = np.zeros(4)
    r.ref_gain_l(_p(l))
    cs = random_agent_cases(24, seed=0x44594E)
    n = cs["x"].shape[0]
    u = np.zeros((n, 4))
    v = np.zeros((n, 3))
    k1 = {k: cs[k].copy() for k in ("x", "rot", "P")}
    k2 = {k: cs[k].copy() for k in ("x", "rot", "P")}
    for a in range(n):
        r.ref_control_velocity(_p(cs["x"][a]), _p(cs["rot"][a]), _p(cs["vgoal"][a]),
                               _p(cs["u_goal"][a]), _p(g["L"]), _p(g["E"]), _p(l), _p(u[a]))
        r.ref_control_position(_p(cs["x"][a]), _p(cs["rot"][a]), _p(cs["p_goal"][a]),
                               _p(cs["u_goal"][a]), _p(g["Lh"]), _p(g["Eh"]), _p(v[a]))
        r.ref_kalman1(_p(k1["x"][a]), _p(k1["rot"][a]), _p(u[a]), _p(k1["P"][a]))
        r.ref_kalman2(_p(k2["x"][a]), _p(k2["rot"][a]), _p(cs["z"][a]), _p(k2["P"][a]))
    qin = quat_cases()
    qout = np.zeros((qin.shape[0], 4))
    for a in range(qin.shape[0]):
        r.ref_quat_from_rot(_p(qin[a]), _p(qout[a]))
    out = dict(l=l, u=u, v=v, quat_in=qin, quat_out=qout, **{"in_" + k: val for k, val in cs.items()},
               **{"k1_" + k: val for k, val in k1.items()},
               **{"k2_" + k: val for k, val in k2.items()})
    np.savez_compressed(os.path.join(HERE, "dyn.npz"), **out)
    print("wrote dyn.npz:", {k: val.shape for k, val in out.items()})
    hard(r)


def hard(r):
    g = pyoracle.synthesize()
    g["l"] = np.array(dyn_hard.L_TERM)
    out = {}
    for name in dyn_hard.REF_FAMILIES:
        cs = hard_case(name, dyn_hard.ref_agents(name))
        ref = dyn_hard.by_function(dyn_hard.RefFns(r), cs, g)
        orc = dyn_hard.by_function(dyn_hard.OracleFns(pyoracle), cs, g)
        for k, val in ref.items():
            if not (np.all(np.isfinite(val)) and np.array_equal(val.view(np.uint64), orc[k].view(np.uint64))):
                raise SystemExit(f"{name} {k}: the oracle differs from the reference; nothing written")
            out[f"{name}/{k}"] = val
        for k in dyn_hard.REF_INPUTS:
            out[f"{name}/in_{k}"] = np.ascontiguousarray(cs[k], np.float64)
    path = os.path.join(HERE, "dyn_hard.npz")
    np.savez_compressed(path, **out)
    print(f"wrote dyn_hard.npz: {len(dyn_hard.REF_FAMILIES)} families, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
