// lqro_qh_front.inc — the front end of a Qhull-order build, the same for every
// layout of the facets: qh_maxmin, qh_detroundoff (C-0) and qh_maxsimplex on
// W.Pr[0..n).  Included by qh_build (lqro_qhull.hpp) and q3_build
// (lqro_qhull3.hpp) in their bodies, not called: with a function both call,
// k_qhull compiled to other code (394 VGPRs for 401), and the C3 step's median
// of four runs lay above the range of four alternated runs of the code written
// out, both times it was measured.  Expects W.Pr, n, lane, S (a QhTol with a status; all but
// S.interior is set) and QH_FRONT_FAIL, the statement that leaves the build
// (no simplex: S.status |= QHS_INPUT); declares simplex[4].  Wave-uniform.
int simplex[4];
{
  // qh_maxmin
  int maxpoints[6];
  S.max_outside = 0.0;
  S.MAXabs_coord = 0.0;
  S.MAXwidth = -DBL_MAX;
  S.MAXsumcoord = 0.0;
  for (int k = 0; k < 3; k++) {
    int mn, mx;
    qh_extreme(W.Pr, n, k, false, lane, &mn);
    qh_extreme(W.Pr, n, k, true, lane, &mx);
    const double maxk = W.Pr[3 * (size_t)mx + k], mink = W.Pr[3 * (size_t)mn + k];
    const double maxcoord = fmax(maxk, -mink);
    const double temp = maxk - mink;
    if (temp > S.MAXwidth) S.MAXwidth = temp;
    if (maxcoord > S.MAXabs_coord) S.MAXabs_coord = maxcoord;
    S.MAXsumcoord += maxcoord;
    maxpoints[2 * k] = mn;
    maxpoints[2 * k + 1] = mx;
    S.NEARzero[k] = 80 * S.MAXsumcoord * DBL_EPSILON;
  }
  // qh_detroundoff (C-0)
  {
    double maxdistsum = sqrt(3.0) * S.MAXabs_coord;
    if (S.MAXsumcoord < maxdistsum) maxdistsum = S.MAXsumcoord;
    S.DISTround = DBL_EPSILON * (3 * maxdistsum * 1.01 + S.MAXabs_coord);
    const double MINdenom_1 = fmax(1.0 / DBL_MAX, DBL_MIN);
    S.MINdenom = MINdenom_1 * S.MAXabs_coord;
    S.MINdenom_2 = sqrt(MINdenom_1 * 3) * S.MAXabs_coord;
    S.MINvisible = 0.0 + 2 * S.DISTround;
    S.MAXcoplanar = S.MINvisible;
    S.MINoutside = 2 * S.MINvisible;
  }
  // qh_maxsimplex
  {
    double maxcoord = -DBL_MAX, mincoord = DBL_MAX;
    int minx = -1, maxx = -1;
    for (int i = 0; i < 6; i++) {
      const double c = W.Pr[3 * (size_t)maxpoints[i]];
      if (maxcoord < c) { maxcoord = c; maxx = maxpoints[i]; }
      if (mincoord > c) { mincoord = c; minx = maxpoints[i]; }
    }
    double maxdet = maxcoord - mincoord;
    int ns = 0;
    simplex[ns++] = minx;
    if (maxx != minx) simplex[ns++] = maxx;
    if (ns < 2) { S.status |= QHS_INPUT; QH_FRONT_FAIL; }
    for (int i = 2; i < 4; i++) {
      const double prevdet = maxdet;
      int maxpoint = -1, maxnearzero = 0, nearzero;
      maxdet = -1.0;
      for (int m = 0; m < 6; m++) {
        const int p = maxpoints[m];
        bool ins = false;
        for (int t = 0; t < i; t++) ins |= simplex[t] == p;
        if (!ins && p != maxpoint) {
          double det = fabs(qh_detsimplex(S, W.Pr, simplex, i, p, &nearzero));
          if (det > maxdet) { maxdet = det; maxpoint = p; maxnearzero = nearzero; }
        }
      }
      const double targetdet = prevdet * S.MAXwidth;
      const bool falsenarrow = maxdet > 0.0 && maxdet / targetdet < 1.0e-3;
      if (maxpoint < 0 || maxnearzero || falsenarrow) {
        double key = -1.0;
        int idx = 0x7fffffff;
        for (int q = lane; q < n; q += 64) {
          bool skip = false;
          for (int t = 0; t < 6; t++) skip |= maxpoints[t] == q;
          for (int t = 0; t < i; t++) skip |= simplex[t] == q;
          if (skip) continue;
          const double det = fabs(qh_detsimplex(S, W.Pr, simplex, i, q, &nearzero));
          if (det > key || (det == key && q < idx)) { key = det; idx = q; }
        }
        for (int off = 32; off >= 1; off >>= 1) {
          const double ok = __shfl_xor(key, off);
          const int oi = __shfl_xor(idx, off);
          if (ok > key || (ok == key && oi < idx)) { key = ok; idx = oi; }
        }
        if (idx != 0x7fffffff && key > maxdet) { maxdet = key; maxpoint = idx; }
      }
      if (maxpoint < 0) { S.status |= QHS_INPUT; QH_FRONT_FAIL; }
      simplex[i] = maxpoint;
    }
  }
}
