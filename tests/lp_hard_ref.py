"""The new-velocity LP with hard planes, restated in numpy float32: the
expected values of the hard-plane tests (tests/test_hard_planes_cpu.py,
tests/test_gpu_hard_planes.py).

linearProgram1-4 and calculateNewV of LQRObstacles.cpp:1001-1234 ("LQRO"),
with lqro_set_hard_planes' rule in linearProgram4: for a violated plane i the
projected list is planes[0 .. n_hard) as they are, then the projections of
planes j = n_hard .. i-1 (RVO2's linearProgram3(lines, numObstLines,
beginLine, ..) carried to three dimensions).  n_hard = 0 is the reference's
LP, and tests/test_hard_planes_cpu.py pins this file to oracle/pyoracle.py's
newv bit for bit there: that is the licence for using it everywhere else.

Every operation is an elementwise float32 one, dot and cross products are
written out term by term in the reference's order (Vector3.h), normalize is
v * (1.0f / sqrt(v.v)).  The plane scans ("the first plane at or after k that
the result violates") and linearProgram1's max / min run over arrays, as the
kernel's 64-lane scans do: a max or a min does not depend on the order, and
linearProgram1 returning false at the first failing plane or after the loop
is the same answer, because tLeft only grows and tRight only shrinks.
"""
import numpy as np

F = np.float32
EPS = F(0.00001)   # RVO_EPSILON
ZERO, HALF, ONE = F(0.0), F(0.5), F(1.0)
NINF, PINF = F(-np.inf), F(np.inf)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _smul(s, a):      # float * Vector3
    return (s * a[0], s * a[1], s * a[2])


def _vmul(a, s):      # Vector3 * float
    return (a[0] * s, a[1] * s, a[2] * s)


def _normalize(a):
    inv = ONE / np.sqrt(_dot(a, a))
    return (a[0] * inv, a[1] * inv, a[2] * inv)


def _pt(c, k=None):
    return (c[0], c[1], c[2]) if k is None else (c[0][k], c[1][k], c[2][k])


def _nm(c, k=None):
    return (c[3], c[4], c[5]) if k is None else (c[3][k], c[4][k], c[5][k])


def _first_violated(c, lo, hi, result, thresh):
    """The first plane k in [lo, hi) with normal.(point - result) > thresh, or hi."""
    if lo >= hi:
        return hi
    s = c[:, lo:hi]
    v = _dot(_nm(s), _sub(_pt(s), result)) > thresh
    k = int(np.argmax(v))
    return lo + k if v[k] else hi


def _max_ignoring_nan(t, init):
    # std::max(a, t) = (a < t) ? t : a never takes a NaN t
    t = t[~np.isnan(t)]
    return np.max(t, initial=init) if t.size else init


def _min_ignoring_nan(t, init):
    t = t[~np.isnan(t)]
    return np.min(t, initial=init) if t.size else init


def lp1(c, plane_no, lpt, ldir, radius, opt, dir_opt):
    """linearProgram1 (LQRO:1001-1066): (ok, result)."""
    dp = _dot(lpt, ldir)
    disc = dp * dp + radius * radius - _dot(lpt, lpt)
    if disc < ZERO:
        return False, None
    sq = np.sqrt(disc)
    t_left = -dp - sq
    t_right = -dp + sq
    if plane_no > 0:
        s = c[:, :plane_no]
        num = _dot(_sub(_pt(s), lpt), _nm(s))
        den = _dot(ldir, _nm(s))
        par = den * den <= EPS
        if np.any(par & (num > ZERO)):
            return False, None
        live = ~par
        t = num[live] / den[live]
        left = den[live] >= ZERO
        lmax = _max_ignoring_nan(t[left], NINF)
        lmin = _min_ignoring_nan(t[~left], PINF)
        if t_left < lmax:
            t_left = lmax
        if lmin < t_right:
            t_right = lmin
        if t_left > t_right:
            return False, None
    if dir_opt:
        if _dot(opt, ldir) > ZERO:
            return True, _add(lpt, _smul(t_right, ldir))
        return True, _add(lpt, _smul(t_left, ldir))
    t = _dot(ldir, _sub(opt, lpt))
    if t < t_left:
        return True, _add(lpt, _smul(t_left, ldir))
    if t > t_right:
        return True, _add(lpt, _smul(t_right, ldir))
    return True, _add(lpt, _smul(t, ldir))


def lp2(c, plane_no, radius, opt, dir_opt):
    """linearProgram2 (LQRO:1068-1127) for plane plane_no: (ok, result)."""
    pp, pn = _pt(c, plane_no), _nm(c, plane_no)
    plane_dist = _dot(pp, pn)
    plane_dist_sq = plane_dist * plane_dist
    radius_sq = radius * radius
    if plane_dist_sq > radius_sq:
        return False, None
    plane_radius_sq = radius_sq - plane_dist_sq
    center = _smul(plane_dist, pn)
    if dir_opt:
        pov = _sub(opt, _smul(_dot(opt, pn), pn))
        pov_sq = _dot(pov, pov)
        if pov_sq <= EPS:
            result = center
        else:
            result = _add(center, _smul(np.sqrt(plane_radius_sq / pov_sq), pov))
    else:
        result = _add(opt, _smul(_dot(_sub(pp, opt), pn), pn))
        if _dot(result, result) > radius_sq:
            pr = _sub(result, center)
            pr_sq = _dot(pr, pr)
            result = _add(center, _smul(np.sqrt(plane_radius_sq / pr_sq), pr))
    i = _first_violated(c, 0, plane_no, result, ZERO)
    while i < plane_no:
        qp, qn = _pt(c, i), _nm(c, i)
        cp = _cross(qn, pn)
        if _dot(cp, cp) <= EPS:
            return False, None
        ldir = _normalize(cp)
        line_normal = _cross(ldir, pn)
        lpt = _add(pp, _smul(_dot(_sub(qp, pp), qn) / _dot(line_normal, qn), line_normal))
        ok, r = lp1(c, i, lpt, ldir, radius, opt, dir_opt)
        if not ok:
            return False, None
        result = r
        i = _first_violated(c, i + 1, plane_no, result, ZERO)
    return True, result


def lp3(c, radius, opt, dir_opt):
    """linearProgram3 (LQRO:1129-1158): (the plane it fails on or m, result)."""
    m = c.shape[1]
    rf = F(radius)
    if dir_opt:
        result = _vmul(opt, rf)
    elif _dot(opt, opt) > rf * rf:
        result = _vmul(_normalize(opt), rf)
    else:
        result = opt
    i = _first_violated(c, 0, m, result, ZERO)
    while i < m:
        ok, r = lp2(c, i, rf, opt, dir_opt)
        if not ok:
            return i, result
        result = r
        i = _first_violated(c, i + 1, m, result, ZERO)
    return m, result


def projected(c, n_hard, i):
    """linearProgram4's list for the violated plane i: planes [0, n_hard) as
    they are, then the projections of planes [n_hard, i) (LQRO:1169-1191)."""
    hard = c[:, :n_hard]
    if n_hard >= i:
        return hard.copy()
    s = c[:, n_hard:i]
    ip, inn = _pt(c, i), _nm(c, i)
    jp, jn = _pt(s), _nm(s)
    cp = _cross(jn, inn)
    par = _dot(cp, cp) <= EPS
    same = par & (_dot(inn, jn) > ZERO)
    mid = _smul(HALF, _add(ip, jp))
    line_normal = _cross(cp, inn)
    isect = _add(ip, _smul(_dot(_sub(jp, ip), jn) / _dot(line_normal, jn), line_normal))
    nrm = _normalize(_sub(jn, inn))
    out = np.empty((6, i - n_hard), F)
    for a in range(3):
        out[a] = np.where(par, mid[a], isect[a])
        out[3 + a] = nrm[a]
    return np.concatenate([hard, out[:, ~same]], axis=1)


def lp4(c, n_hard, begin, radius, result, trace=None):
    """linearProgram4 (LQRO:1160-1206) with the first n_hard planes hard.
    trace: a list that receives (i, projected list) per violated plane."""
    m = c.shape[1]
    distance = ZERO
    i = _first_violated(c, begin, m, result, distance)
    while i < m:
        proj = projected(c, n_hard, i)
        if trace is not None:
            trace.append((i, proj))
        fail, r = lp3(proj, radius, _nm(c, i), True)
        if fail >= proj.shape[1]:
            result = r
        distance = _dot(_nm(c, i), _sub(_pt(c, i), result))
        i = _first_violated(c, i + 1, m, result, distance)
    return result


def new_v(planes, goal, n_hard=0, vmax=100.0, trace=None, info=None):
    """calculateNewV (LQRO:1223-1234): planes (m, 6) float32 (point, normal) in
    push order, goal (3,); the first min(n_hard, m) planes are hard.  Returns
    float64 (3,) holding the float32 result.  info: a dict that receives
    `fail` (linearProgram3's return) and `m`."""
    with np.errstate(all="ignore"):
        c = np.ascontiguousarray(np.asarray(planes, F).reshape(-1, 6).T)
        m = c.shape[1]
        g = np.asarray(goal, np.float64).astype(F)
        fail, r = lp3(c, vmax, (g[0], g[1], g[2]), False)
        if info is not None:
            info["fail"], info["m"] = fail, m
        if fail < m:
            r = lp4(c, min(max(int(n_hard), 0), m), fail, F(vmax), r, trace)
        return np.array([r[0], r[1], r[2]], F).astype(np.float64)
