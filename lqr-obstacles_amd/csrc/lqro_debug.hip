// lqro_debug.hip — the lqro_debug_* hooks: test and diagnostic entry points
// outside include/lqro.h (tests and scripts/ bind them by name).  None of
// them looks at a pending half-step.
#include <cstring>

#include "lqro_ctx.hpp"
#include "lqro_kern.hpp"

using namespace lqro;

extern "C" {

/* diagnostic (not in lqro.h): inside-hull pairs of the last step decided by
 * the local hull (out[0]) and handed to the full hull (out[1]); out[2..17]:
 * hand-over reasons since the context was created (k_lhull's fail code - 20;
 * 0: the point set / initial tetrahedron) */
int lqro_debug_local_hull(lqro_ctx* c, long long* out) {
  if (!c || !out) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, false)) return rc;
  int h[LQRO_HC_WORDS];
  HIPCHK(hipMemcpy(h, c->d_hcount, sizeof h, hipMemcpyDeviceToHost));
  unsigned long long r[16];
  HIPCHK(hipMemcpy(r, c->d_prof + LQRO_PROF_LFAIL, sizeof r, hipMemcpyDeviceToHost));
  out[0] = h[LQRO_HC_LDONE];
  out[1] = h[LQRO_HC_LHAND];
  for (int k = 0; k < 16; ++k) out[2 + k] = (long long)r[k];
  return LQRO_OK;
}

// lqro_debug_hull_points and lqro_debug_hull_points_ex: one job (slot 0 of a
// queue of the hook's own) on the given points.  reason: null, or 16 words
// that receive k_lhull's hand-over counters of this call (local = 1).
static int debug_hull_points(lqro_ctx* c, const double* pts, int32_t n, const double* vrel, int32_t local,
                             int32_t* facets, int32_t max_facets, int32_t* n_facets, lqro_pair_record* rec,
                             int32_t max_local, long long* reason) {
  const bool lists = local == 0 || local == 4;   // k_hull writes its facets out
  if (!c || !pts || !vrel || !n_facets || !rec || n < 4 || (size_t)n > (size_t)c->cfg.horizon * c->cfg.n_points ||
      (lists && (!facets || max_facets < 1)) || local < 0 || local > max_local)
    return LQRO_E_ARG;
  const lqro_config& g = c->cfg;
  if (int rc = ctx_enter(c, false)) return rc;
  const int X = g.x_dim;
  std::vector<double> xh(2 * (size_t)X, 0.0);
  for (int q = 0; q < 3; ++q) xh[3 + q] = vrel[q];       // x_i - x_j = vrel, at rest otherwise
  DevPool mem;
  double *d_pts = nullptr, *d_x = nullptr;
  int *d_q = nullptr, *d_f = nullptr;
  lqro_pair_record* d_rec = nullptr;
  float* d_pl = nullptr;
  unsigned long long *d_st = nullptr, *d_lf = nullptr, *d_pf = nullptr;
  char* d_qw = nullptr;
  double* d_qn = nullptr;
  const bool emit = facets && (lists || local == 2);
  const int fmax = emit ? max_facets : 1;
  const size_t qstride = (qhull_worker_bytes(g.horizon * g.n_points) + 255) & ~(size_t)255;
  if (local == 2 && (mem.get(d_qw, qstride, 0) || mem.get(d_qn, 8))) return LQRO_E_NOMEM;
  // the reason words come from buffers of the hook's own, never the context's
  // profile words: k_lhull's 16 counters, or the hull kernels' profile region
  // (their outcome histogram is its words 16 .. 31)
  if (local == 1 && reason && mem.get(d_lf, 16, 0)) return LQRO_E_NOMEM;
  if (local != 1 && local != 2 && reason && mem.get(d_pf, LQRO_PROF_HULL_WORDS, 0)) return LQRO_E_NOMEM;
  if (mem.get(d_st, LQRO_ST_WORDS, 0) || mem.get(d_pts, (size_t)(local == 2 ? 6 : 3) * n) ||
      mem.get(d_x, 2 * (size_t)X) || mem.get(d_q, 16) || mem.get(d_f, 3 * (size_t)fmax) || mem.get(d_rec, 1) ||
      mem.get(d_pl, 8))
    return LQRO_E_NOMEM;
  // queue = {slot 0}; count 1; next, local hand-over count / next, done, facet count 0
  const int q0[16] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  lqro_pair_record r0;
  memset(&r0, 0, sizeof r0);
  r0.flags = LQRO_REC_INSIDE;
  if (hipMemcpy(d_pts, pts, sizeof(double) * (local == 2 ? 6 : 3) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_x, xh.data(), sizeof(double) * 2 * X, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_q, q0, sizeof q0, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_rec, &r0, sizeof r0, hipMemcpyHostToDevice) != hipSuccess)
    return LQRO_E_HIP;
  HullArgs Hh{};
  Hh.N = 2; Hh.X = X; Hh.H = g.horizon; Hh.NP = g.n_points;
  Hh.row_begin = 0; Hh.row_stride = 1; Hh.npr = 1; Hh.per_agent = 0;
  Hh.r2 = g.vmax_reach * g.vmax_reach; Hh.r2_lo = Hh.r2; Hh.r2_hi = Hh.r2;
  Hh.T = c->d_T; Hh.NCF = c->d_NCF; Hh.S = c->d_S; Hh.x = d_x;
  Hh.planes = d_pl; Hh.recs = d_rec;
  Hh.queue = d_q + 8; Hh.count = d_q + 1; Hh.cap = 1; Hh.next = d_q + 2;   // d_q[8] = 0: slot 0
  Hh.scratch = c->d_hscratch; Hh.iscratch = c->d_hiscratch; Hh.fscratch = c->d_hfscratch;
  Hh.sb = c->d_hfaces;
  Hh.fbest = c->d_hfbest; Hh.vpid = c->d_hvpid; Hh.stack = c->d_hstack;
  Hh.rqueue = d_q + 12; Hh.rcount = d_q + 3; Hh.rnext = d_q + 4;
  Hh.bigmem = c->d_hbig; Hh.wide = c->d_hwide; Hh.bag = c->d_hbag;
  Hh.stats = d_st; Hh.prof = d_pf;      // the hook never alters the step's statistics
  Hh.lqueue = d_q + 13; Hh.lcount = d_q + 5; Hh.ldone = d_q + 6;
  Hh.lfail = d_lf;
  Hh.ext_pts = d_pts; Hh.ext_n = n; Hh.ext_max = fmax;
  Hh.ext_facets = emit ? d_f : nullptr; Hh.ext_nf = d_q + 7;
  Hh.ext_full = local == 2;   // k_qhull: rounded points, then the full-precision ones
  Hh.qscratch = d_qw; Hh.qstride = qstride; Hh.qnrm = d_qn; Hh.qflags = c->knobs.qhull_flags;
  Hh.qstale = d_q + 14; Hh.qstale_count = d_q + 9; Hh.qstale_cap = 1;
  if (local == 2) {
    Hh.big_main = c->knobs.qhull_big;
    if (!c->knobs.qhull_big) launch_qhull(dim3(1), c->stream, Hh);
    launch_qhull_big(dim3(1), c->stream, Hh);
  } else if (local == 1) {
    launch_lhull(dim3(1), c->stream, Hh);
  } else if (local == 3) {
    Hh.big_main = 1;                   // k_hull_big alone, on the main queue
    launch_hull_big(dim3(1), c->stream, Hh);
  } else {
    launch_hull(dim3(1), c->stream, Hh);
    if (local == 4) launch_hull_big(dim3(1), c->stream, Hh);   // its retry queue, as enqueue_full_hulls (big_main = 0)
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return LQRO_E_HIP;
  int qh[16];
  if (hipMemcpy(qh, d_q, sizeof qh, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(rec, d_rec, sizeof *rec, hipMemcpyDeviceToHost) != hipSuccess)
    return LQRO_E_HIP;
  if (local == 2) {
    *n_facets = qh[7];                 // k_qhull's build status
    if (facets && hipMemcpy(facets, d_f, sizeof(int) * 3 * fmax, hipMemcpyDeviceToHost) != hipSuccess)
      return LQRO_E_HIP;
    // lqro_step's rule: a merge-suspect winner is reported (LQRO_E_QHMERGE)
    unsigned long long mw = 0;
    if (hipMemcpy(&mw, d_st + LQRO_ST_MWIN, sizeof mw, hipMemcpyDeviceToHost) != hipSuccess) return LQRO_E_HIP;
    if (mw) return LQRO_E_QHMERGE;
  } else if (local == 1) {
    *n_facets = qh[5] > 0 ? -1 : 0;   // handed over: the full hull would decide
    if (reason) {
      unsigned long long r[16];
      if (hipMemcpy(r, d_lf, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) return LQRO_E_HIP;
      for (int k = 0; k < 16; ++k) reason[k] = (long long)r[k];
    }
  } else if (local == 3) {
    *n_facets = rec->n_facets;         // (k_hull_big writes no facet list)
  } else {
    *n_facets = qh[7];
    if (qh[3] > 0) *n_facets = -2;     // k_hull's capacity: k_hull_big decides (local = 4: has decided)
    const int k = std::min(qh[7], max_facets);
    if (k > 0 && hipMemcpy(facets, d_f, sizeof(int) * 3 * k, hipMemcpyDeviceToHost) != hipSuccess) return LQRO_E_HIP;
  }
  if (d_pf) {
    unsigned long long r[16];
    if (hipMemcpy(r, d_pf + 16, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) return LQRO_E_HIP;
    for (int k = 0; k < 16; ++k) reason[k] = (long long)r[k];
  }
  return LQRO_OK;
}

/* test hook (not in lqro.h): the inside-hull branch on n given points
 * (already %g-rounded, as qconvex reads them; n <= H * NP of the context)
 * with relative velocity vrel.  local = 0: k_hull, its facets (point ids)
 * into facets (max_facets x 3) and their count into *n_facets; local = 1:
 * k_lhull (no facet list; *n_facets = -1 when it handed the points over);
 * local = 2: k_qhull, Qhull's build order and the reference's selection;
 * pts then holds the n rounded points followed by the n full-precision ones
 * (*n_facets = the build's status bits, 0: Qhull's build reproduced).
 * rec receives the selected facet, distance and normal. */
int lqro_debug_hull_points(lqro_ctx* c, const double* pts, int32_t n, const double* vrel, int32_t local,
                           int32_t* facets, int32_t max_facets, int32_t* n_facets, lqro_pair_record* rec) {
  return debug_hull_points(c, pts, n, vrel, local, facets, max_facets, n_facets, rec, 2, nullptr);
}

/* test hook (not in lqro.h): lqro_debug_hull_points with two more modes and
 * one more output.  local = 3: k_hull_big alone on the points (big_main = 1;
 * no facet list, *n_facets = the record's facet count, -1: it could not
 * build).  local = 4: k_hull, then k_hull_big on k_hull's retry queue, as the
 * step launches them; *n_facets = k_hull's facet count (facets: its list)
 * when it finished, -2 when the retry ran; rec is whichever kernel's.
 * reason (16 words, or null): with local = 1, k_lhull's hand-over counters of
 * this call alone, index = its fail code - 20 (0: the point set or the
 * initial tetrahedron); with local = 0, 3, 4 how many of the call's builds
 * ended with hull fail code k (0: built; 1 the vertex cap, 4 the face slots,
 * 8 a degenerate set, ...), hull_select's outcome histogram.  Either from a
 * buffer of the hook's own. */
int lqro_debug_hull_points_ex(lqro_ctx* c, const double* pts, int32_t n, const double* vrel, int32_t local,
                              int32_t* facets, int32_t max_facets, int32_t* n_facets, lqro_pair_record* rec,
                              long long* reason) {
  if (reason) for (int k = 0; k < 16; ++k) reason[k] = 0;
  return debug_hull_points(c, pts, n, vrel, local, facets, max_facets, n_facets, rec, 4, reason);
}

/* diagnostic (not in lqro.h): n profile words from offset (k_qhull's wave 1
 * and per-class phases of a -DLQRO_QHULL_PROFILE build: offset Q3_PROF_W1) */
int lqro_debug_prof_words(lqro_ctx* c, int64_t offset, int64_t n, unsigned long long* out) {
  if (!c || !out || offset < 0 || n < 0 || offset + n > LQRO_PROF_WORDS) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, false)) return rc;
  HIPCHK(hipMemcpy(out, c->d_prof + offset, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
  return LQRO_OK;
}

/* diagnostic (not in lqro.h): k_lhull's per-job words of the last step
 * (4 x 4096: point ticks, loop ticks at 100 MHz, iterations | nv << 16 |
 * live points << 32, n | fail << 32 | faces << 40) */
int lqro_debug_local_hull_jobs(lqro_ctx* c, unsigned long long* out) {
  if (!c || !out) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, false)) return rc;
  HIPCHK(hipMemcpy(out, c->d_prof + LQRO_PROF_LJOBS, sizeof(unsigned long long) * 4 * 4096, hipMemcpyDeviceToHost));
  return LQRO_OK;
}

/* diagnostic (not in lqro.h): accumulated k_hull phase cycles of a
 * -DLQRO_HULL_PROFILE build */
int lqro_debug_hull_profile(lqro_ctx* c, unsigned long long* out16) {
  if (!c || !out16) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, false)) return rc;
  // the documented prefix only (32 hull counters, 2 x 4096 job words, 32
  // pair / wave-phase words): callers size their buffer to it
  HIPCHK(hipMemcpy(out16, c->d_prof, sizeof(unsigned long long) * LQRO_PROF_HULL_WORDS, hipMemcpyDeviceToHost));
  return LQRO_OK;
}

}  // extern "C"
