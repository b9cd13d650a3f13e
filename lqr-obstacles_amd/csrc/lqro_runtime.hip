// lqro_runtime.hip — the context-bound part of include/lqro.h's C-ABI:
// lqro_create / lqro_destroy, the setters, the step and the getters.  The
// context is lqro_ctx.hpp; the kernels live in objects of their own
// (lqro_kern_*.hip, lqro_pair_inst.hip; launched through lqro_kern.hpp and
// lqro_pair_launch.hpp), the context-free entry points in lqro_oneshot.hip,
// the lqro_debug_* hooks in lqro_debug.hip.
// One control step = the pair loop of LQRObstacles.cpp:1393-1436: k_pair per
// ordered pair, the hull kernels for the inside-hull pairs (in place of
// qconvex.exe), k_lp per agent.  Exactness: see lqro_device.hpp.
#define LQRO_RUNTIME_TU 1   // (lqro_ctx.hpp: this object holds lqro_pair.hpp's non-template kernels)
#include <cmath>
#include <cstring>
#include <new>

#include "lqro_ctx.hpp"
#include "lqro_kern.hpp"

using namespace lqro;

// device memory as lqro_devmem.hpp's pools get it
namespace lqro {
int devmem_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
int devmem_free(void* p) { return (int)hipFree(p); }
int devmem_fill(void* p, int byte, size_t bytes) { return (int)hipMemset(p, byte, bytes); }
}  // namespace lqro

// k_pair / k_side / k_qside for the context's state width and record mode
// (the instantiations live in lqro_pair_inst.hip, one object per combination)
#define PAIR_INST(x_dim, recs, fn, ...)                                                          \
  do {                                                                                           \
    if ((x_dim) == 16) { if (recs) fn<16, true>(__VA_ARGS__); else fn<16, false>(__VA_ARGS__); } \
    else { if (recs) fn<12, true>(__VA_ARGS__); else fn<12, false>(__VA_ARGS__); }               \
  } while (0)
static void launch_pair(int x_dim, dim3 grid, dim3 block, size_t lds, hipStream_t s, const PairArgs& P) {
  PAIR_INST(x_dim, P.recs != nullptr, launch_pair_t, grid, block, lds, s, P);
}
static void launch_side(int x_dim, dim3 grid, dim3 block, hipStream_t s, const HullArgs& H, const PairArgs& P) {
  PAIR_INST(x_dim, P.recs != nullptr, launch_side_t, grid, block, s, H, P);
}
static void launch_qside(int x_dim, dim3 grid, hipStream_t s, const HullArgs& H, const PairArgs& P) {
  PAIR_INST(x_dim, P.recs != nullptr, launch_qside_t, grid, s, H, P);
}

// a kernel launch, then its status
#define LAUNCH(call) do { call; HIPCHK(hipGetLastError()); } while (0)

constexpr size_t kHullLdsMaxHNP = (size_t)(1 << 19) / HULL_SBMULT;   // 21,845 (C5: H*NP = 20,000)

extern "C" {

void lqro_destroy(lqro_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  c->mem.free_all();   // the device buffers first, while the streams and events still exist
  for (int k = 0; k < 5; ++k)
    if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
  for (int k = 0; k < 2; ++k) {
    if (c->xev[k]) (void)hipEventDestroy(c->xev[k]);
    if (c->iev[k]) (void)hipEventDestroy(c->iev[k]);
  }
  if (c->cev) (void)hipEventDestroy(c->cev);
  if (c->h_feedback) (void)hipHostFree(c->h_feedback);
  if (c->side) (void)hipStreamDestroy(c->side);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// The buffers pitched in pair slots (rows x slots a row), and the capacities
// that follow them.  lqro_create allocates them; lqro_set_obstacles again when
// the number of columns changes: the new set first (a failed call leaves the
// context as it was), then the old one is released.
struct SlotBufs {
  float *d_planes, *d_lpscratch, *d_lpcompact;
  lqro_pair_record* d_recs;
  int *d_hq, *d_rq, *d_lq, *d_hotlist, *d_prevq, *d_qstale, *d_nbrlist;
  unsigned char* d_hotmark;
  double* d_qnrm;
  int hull_cap, hot_cap, lp_cap, nbr_cap;
};
#define SLOT_BUFS(F) \
  F(d_planes) F(d_lpscratch) F(d_lpcompact) F(d_recs) F(d_hq) F(d_rq) F(d_lq) F(d_hotlist) F(d_prevq) F(d_qstale) \
  F(d_hotmark) F(d_qnrm)

static void slots_release(lqro_ctx* c, SlotBufs& b) {
#define F(m) c->mem.release(b.m);
  SLOT_BUFS(F)
#undef F
  c->mem.release(b.d_nbrlist);
}

static int slots_alloc(lqro_ctx* c, int npr, SlotBufs& b) {
  const lqro_config& g = c->cfg;
  const size_t rows = (size_t)c->nrows, slots = rows * (size_t)npr;   // (both at least 1)
  b = SlotBufs{};
  b.lp_cap = npr + c->nfence + c->uplane_max;
  // one entry per slot: a pair enqueues at most one hull job per step, so the
  // queue cannot overflow (C5's 2048 x 16383-slot shard: 134 MB, of 288 GB)
  b.hull_cap = (int)slots;
  b.hot_cap = (int)std::max<size_t>(16384, slots / 32);
  bool bad = false;
#define SB(member, ...) bad = bad || c->mem.get(b.member, __VA_ARGS__) != 0
  SB(d_planes, 8 * slots);
  SB(d_lpscratch, 8 * rows * (size_t)b.lp_cap);
  SB(d_lpcompact, 8 * rows * (size_t)b.lp_cap);
  if (g.flags & LQRO_FLAG_RECORDS) SB(d_recs, slots);
  SB(d_hq, slots);
  SB(d_rq, slots);
  SB(d_lq, slots);
  SB(d_hotlist, (size_t)b.hot_cap);
  // (k_prio keeps a mark of 2 it finds — k_prio_prev's "listed" — so the marks
  // start at 0: the first split step after the plain ones would otherwise
  // take recycled device memory's bytes for marks and skip those pairs)
  SB(d_hotmark, slots, 0);
  if (c->qhull_order) {
    SB(d_qnrm, 4 * slots);
    SB(d_qstale, slots, 0xFF);
    SB(d_prevq, (size_t)b.hot_cap, 0xFF);
  }
  if (c->nbr_k > 0) {   // (culling on: the lists at the new K)
    b.nbr_cap = std::min(c->nbr_k, npr);
    SB(d_nbrlist, rows * (size_t)b.nbr_cap + 1);
  }
#undef SB
  if (bad) { slots_release(c, b); return LQRO_E_NOMEM; }
  return LQRO_OK;
}

// the context takes b (and npr) for its own; its old set goes
static void slots_adopt(lqro_ctx* c, int npr, SlotBufs& b) {
  SlotBufs old{};
#define F(m) old.m = c->m; c->m = b.m;
  SLOT_BUFS(F)
#undef F
  if (b.d_nbrlist) { old.d_nbrlist = c->d_nbrlist; c->d_nbrlist = b.d_nbrlist; c->nbr_cap = b.nbr_cap; }
  slots_release(c, old);
  c->npr = npr; c->hull_cap = b.hull_cap; c->hot_cap = b.hot_cap; c->lp_cap = b.lp_cap;
}

static int ctx_alloc(lqro_ctx* c) {
  const lqro_config& g = c->cfg;
  const size_t N = g.n_agents, X = g.x_dim, U = g.u_dim, H = g.horizon, NP = g.n_points;
  const size_t rows = (size_t)c->nrows;
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  for (int k = 0; k < 5; ++k) HIPCHK(hipEventCreate(&c->ev[k]));
  HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) HIPCHK(hipEventCreateWithFlags(&c->xev[k], hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->cev, hipEventDisableTiming));
  // one line per buffer: member, elements[, the byte every element starts as]
#define BUF(member, ...) HIPCHK((hipError_t)c->mem.get(c->member, __VA_ARGS__))
  BUF(d_S, NP * 3);
  BUF(d_x, N * X);
  BUF(d_vgoal, N * 3);
  BUF(d_newv, N * 3);
  BUF(d_A, X * X);
  BUF(d_B, X * U);
  BUF(d_L, N * U * X);
  BUF(d_E, N * U * 3);
  BUF(d_T, N * H * 9);
  BUF(d_NCF, N * H * 3 * X);
  BUF(d_R, N * H);
  BUF(d_TF, N * H);
  BUF(d_shash, H);
  {
    SlotBufs b;
    if (int rc = slots_alloc(c, c->npr, b)) return rc;
    slots_adopt(c, c->npr, b);
  }
  BUF(d_hcount, LQRO_HC_WORDS);
  BUF(d_err, 1);
  BUF(d_stats, LQRO_ST_WORDS);
  HIPCHK(hipHostMalloc((void**)&c->h_feedback, 2 * sizeof(StepFeedback), hipHostMallocDefault));
  for (int k = 0; k < 2; ++k) c->h_feedback[k] = kNoFeedback;
  for (int k = 0; k < 2; ++k) HIPCHK(hipEventCreateWithFlags(&c->iev[k], hipEventDisableTiming));
  BUF(d_prof, LQRO_PROF_WORDS, 0);
  c->hull_blocks = 256;   // one 138 KB-LDS workgroup per CU, persistent over the queue
  const size_t hb = (size_t)c->hull_blocks;
  BUF(d_hscratch, 6 * H * NP * hb);
  BUF(d_hiscratch, 2 * H * NP * HULL_SCR_WAVES * hb);
  BUF(d_hfscratch, H * NP * HULL_WAVES * hb);
  BUF(d_hfbest, HULL_FB_STRIDE * hb);
  BUF(d_hvpid, HULL_VG_STRIDE * hb);
  BUF(d_hstack, HULL_STKMULT * H * NP * hb);
  BUF(d_hfaces, HULL_SBMULT * H * NP * hb);
  c->hull_big_blocks = c->n_cu;   // one 1-inserting-wave hull per CU (topology in global memory)
  BUF(d_hbig, (size_t)c->hull_big_blocks);
  BUF(d_hwide, HULL_CWAVES * hb);
  BUF(d_hbag, HULL_BAGCAP * hb, 0xFF);
  BUF(d_lp4, 8 * rows, 0);
  BUF(d_carry, 6, 0);
  BUF(d_rowpend, 2 * rows, 0);
  c->d_rowclaim = c->d_rowpend + rows;   // (the second half of the same buffer)
  if (c->qhull_order) {
    // k_qhull: one one-wave worker per CU (the build's facets fill the CU's
    // LDS), each with its own build scratch
    c->qworkers = c->n_cu;
    c->qstride = (qhull_worker_bytes((int)(H * NP)) + 255) & ~(size_t)255;
    BUF(d_qscratch, c->qstride * (size_t)c->qworkers, 0);   // k_qhull_big's visit stamps
    BUF(d_hbuild, 4 * (size_t)LQRO_HBUILD_CAP, 0);
    BUF(d_hot2, LQRO_H2_WORDS, 0);
  }
#undef BUF
  return LQRO_OK;
}

// k_pair's LDS layout (lqro_plan.hpp pair_layout) into its arguments.
// n_cls: the obstacle shape classes that are not the agents'
// (lqro_set_obstacles[_ex]); 0: the layout a context is created with.  False
// when no wave's region fits.
static bool pair_layout(const lqro_config& g, int n_cls, PairArgs& P, int& lds_bytes) {
  PairLayout L{};
  if (!pair_layout(g.horizon, g.n_points, g.x_dim, n_cls, L, LQRO_PAIR_LB / 64)) return false;
  P.XP = L.XP; P.PW = L.PW;
  P.lds_T = L.lds_T; P.lds_N = L.lds_N; P.lds_S = L.lds_S; P.lds_R = L.lds_R; P.lds_TF = L.lds_TF; P.lds_H = L.lds_H;
  P.lds_cls = L.lds_cls; P.cls_doubles = L.cls_doubles; P.n_cls = n_cls;
  P.lds_wave = L.lds_wave; P.wave_doubles = L.wave_doubles;
  P.waves = L.waves;
  P.max_waves = L.waves;
  lds_bytes = L.lds_bytes;
  return true;
}

static bool pair_set_lds(int lds_bytes) {
  return pair_set_lds_t<16, false>(lds_bytes) && pair_set_lds_t<16, true>(lds_bytes) &&
         pair_set_lds_t<12, false>(lds_bytes) && pair_set_lds_t<12, true>(lds_bytes);
}

// max |u_p| with s_p = diag(rad) u_p (createSpheres, :743-745), with the
// bound's margin.  A zero semi-axis contributes nothing: every point's
// coordinate on it is 0, so its u is 0 (0 / 0 would make u2 a NaN that
// std::max drops, and the whole set's bound 0)
static double sphere_umax(const double* S, int NP, const double* rad) {
  double um = 0.0;
  for (int p = 0; p < NP; ++p) {
    double u2 = 0.0;
    for (int d = 0; d < 3; ++d) {
      if (rad[d] == 0.0) continue;
      const double u = S[3 * p + d] / rad[d];
      u2 += u * u;
    }
    um = std::max(um, std::sqrt(u2));
  }
  return um * (1.0 + 1e-12);
}

int lqro_create(const lqro_config* cfg, lqro_ctx** out) {
  if (!cfg || !out) return LQRO_E_ARG;
  *out = nullptr;
  const lqro_config& g = *cfg;
  if (g.n_agents < 2 || (g.x_dim != 16 && g.x_dim != 12) || g.u_dim != 4 || g.horizon < 1 ||
      g.n_points < 1 || g.vmax_reach <= 0 || g.n_points > 64 * kMaxPW || g.horizon > 64 * kMaxKS)
    return LQRO_E_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= g.device) return LQRO_E_NODEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, g.device) != hipSuccess) return LQRO_E_NODEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "liblqro: device %d is %s, built for gfx950\n", g.device, prop.gcnArchName);
    return LQRO_E_NODEVICE;
  }
  if (hipSetDevice(g.device) != hipSuccess) return LQRO_E_HIP;
  lqro_ctx* c = new (std::nothrow) lqro_ctx();   // every scalar and pointer zero
  if (!c) return LQRO_E_NOMEM;
  c->cfg = g;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->qhull_order = (g.flags & LQRO_FLAG_QHULL_ORDER) ? 1 : 0;
  c->knobs = knobs_from_env(c->n_cu);
  c->rb = g.row_begin;
  c->re = (g.row_end > g.row_begin) ? g.row_end : g.n_agents;
  c->rs = g.row_stride > 1 ? g.row_stride : 1;
  if (c->rb < 0 || c->re > g.n_agents || c->rb >= c->re || g.row_stride < 0) { delete c; return LQRO_E_ARG; }
  c->nrows = (c->re - c->rb + c->rs - 1) / c->rs;
  c->npr = g.n_agents - 1;
  const int H = g.horizon, NP = g.n_points;
  PairArgs& P = c->pa;
  P.obs_jj = INT_MAX;   // (no obstacle columns)
  int lds_bytes = 0;
  if (!pair_layout(g, 0, P, lds_bytes)) {
    fprintf(stderr, "liblqro: horizon %d x %d points does not fit in LDS\n", H, NP);
    delete c;
    return LQRO_E_ARG;
  }
  c->lds_bytes = lds_bytes;
  int rc = ctx_alloc(c);
  if (rc) { lqro_destroy(c); return rc; }
  std::vector<double> S(3 * (size_t)NP);
  lqro_sphere(NP, g.xy_radius, g.z_radius, S.data());
  {
    const double rad[3] = {2 * g.xy_radius, 2 * g.xy_radius, 2 * g.z_radius};
    c->umax = sphere_umax(S.data(), NP, rad);
    P.rad0 = rad[0]; P.rad1 = rad[1]; P.rad2 = rad[2]; P.umax = c->umax;
  }
  {
    std::vector<unsigned long long> sh(H, 0ull);
    for (int k = 0; k < H; ++k)
      for (int p = 0; p < NP; ++p) {
        unsigned long long z = (unsigned long long)(k * NP + p) + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        sh[k] += z ^ (z >> 31);
      }
    if (hipMemcpy(c->d_shash, sh.data(), sizeof(unsigned long long) * H, hipMemcpyHostToDevice) != hipSuccess) {
      lqro_destroy(c);
      return LQRO_E_HIP;
    }
  }
  if (hipMemcpy(c->d_S, S.data(), sizeof(double) * S.size(), hipMemcpyHostToDevice) != hipSuccess) {
    lqro_destroy(c);
    return LQRO_E_HIP;
  }
  if (!pair_set_lds(c->lds_bytes)) {
    lqro_destroy(c);
    return LQRO_E_HIP;
  }
  *out = c;
  return LQRO_OK;
}

int lqro_set_neighbors(lqro_ctx* c, double neighbor_dist, int32_t max_neighbors) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // lqro_step_device_begin's half-step still reads them
  if (max_neighbors <= 0) { c->nbr_k = 0; return LQRO_OK; }
  if (!(neighbor_dist > 0)) return LQRO_E_ARG;
  HIPCHK(hipSetDevice(c->cfg.device));
  const int K = std::min<int>(max_neighbors, c->npr);
  if (K > c->nbr_cap) {
    c->nbr_cap = 0;
    c->mem.release(c->d_nbrlist);
    if (c->mem.get(c->d_nbrlist, (size_t)c->nrows * K + 1)) return LQRO_E_NOMEM;
    c->nbr_cap = K;
  }
  c->nbr_r2 = neighbor_dist * neighbor_dist;
  c->nbr_k = max_neighbors;
  return LQRO_OK;
}

constexpr int kMaxUserPlanes = 8192;   // per agent

// the LP scratch at a pitch of npr + extra planes per row; only grows, and
// never in a step.  The caller has waited for the last step.
static int lp_scratch_reserve(lqro_ctx* c, int extra) {
  const int cap = c->npr + extra;
  if (cap <= c->lp_cap) return LQRO_OK;
  const size_t n = 8 * (size_t)c->nrows * (size_t)cap;
  float *a = nullptr, *b = nullptr;
  if (c->mem.get(a, n) || c->mem.get(b, n)) {
    c->mem.release(a);
    return LQRO_E_NOMEM;   // (the old buffers stay)
  }
  c->mem.release(c->d_lpscratch);
  c->mem.release(c->d_lpcompact);
  c->d_lpscratch = a; c->d_lpcompact = b; c->lp_cap = cap;
  return LQRO_OK;
}

// the user planes' fixed-pitch device layout becomes the context's; `own`:
// the context's copies (lqro_set_user_planes), freed when replaced
static int set_user_layout(lqro_ctx* c, const float* d_planes, int maxp, const int* d_counts, float* own,
                           int* cown) {
  if (maxp > 0)
    if (int rc = lp_scratch_reserve(c, c->nfence + maxp)) return rc;
  c->mem.release(c->d_uown);
  c->mem.release(c->d_ucown);
  c->d_uown = own; c->d_ucown = cown;
  c->d_uplanes = maxp > 0 ? d_planes : nullptr;
  c->d_ucounts = maxp > 0 ? d_counts : nullptr;
  c->uplane_max = maxp > 0 ? maxp : 0;
  return LQRO_OK;
}

int lqro_set_user_planes_device(lqro_ctx* c, const float* d_planes, int32_t max_per_agent, const int32_t* d_counts) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step's LP still reads them
  if (max_per_agent > kMaxUserPlanes || (max_per_agent > 0 && !d_planes)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, false)) return rc;
  return set_user_layout(c, d_planes, max_per_agent, d_counts, nullptr, nullptr);
}

int lqro_set_user_planes(lqro_ctx* c, const float* planes, const int64_t* offsets) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;
  if (planes && !offsets) return LQRO_E_ARG;
  const size_t N = (size_t)c->cfg.n_agents;
  int64_t maxp = 0;
  if (planes)
    for (size_t i = 0; i < N; ++i) {
      const int64_t m = offsets[i + 1] - offsets[i];
      if (m < 0 || m > kMaxUserPlanes) return LQRO_E_ARG;
      maxp = std::max(maxp, m);
    }
  if (int rc = ctx_enter(c, false)) return rc;
  if (maxp == 0) return set_user_layout(c, nullptr, 0, nullptr, nullptr, nullptr);
  // the same layout lqro_set_user_planes_device takes, in buffers of the context's own
  std::vector<float> h(N * (size_t)maxp * 6, 0.0f);
  std::vector<int> cnt(N);
  for (size_t i = 0; i < N; ++i) {
    cnt[i] = (int)(offsets[i + 1] - offsets[i]);
    if (cnt[i]) memcpy(&h[i * (size_t)maxp * 6], planes + 6 * offsets[i], sizeof(float) * 6 * (size_t)cnt[i]);
  }
  float* own = nullptr;
  int* cown = nullptr;
  if (c->mem.get(own, h.size()) || c->mem.get(cown, N)) {
    c->mem.release(own);
    return LQRO_E_NOMEM;
  }
  int rc = LQRO_OK;
  if (hipMemcpy(own, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(cown, cnt.data(), sizeof(int) * N, hipMemcpyHostToDevice) != hipSuccess)
    rc = LQRO_E_HIP;
  // (the stream the step reads them on may be non-blocking: the copies above are synchronous)
  if (rc == LQRO_OK) rc = set_user_layout(c, own, (int)maxp, cown, own, cown);
  if (rc != LQRO_OK) { c->mem.release(own); c->mem.release(cown); }   // (a failed call leaves the old planes in place)
  return rc;
}

int lqro_set_fence(lqro_ctx* c, const double* lo, const double* hi, double tau) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;
  const lqro_config& g = c->cfg;
  int faces = 0, n = 0;
  if (lo && hi && tau > 0) {
    for (int a = 0; a < 3; ++a) {
      const double m = a < 2 ? g.xy_radius : g.z_radius;
      if (lo[a] + 2 * m > hi[a]) return LQRO_E_ARG;   // (NaN bounds are outside the contract)
      if (!std::isinf(lo[a])) { faces |= 1 << (2 * a); ++n; }
      if (!std::isinf(hi[a])) { faces |= 1 << (2 * a + 1); ++n; }
    }
  }
  if (int rc = ctx_enter(c, false)) return rc;
  if (n > 0) {
    if (int rc = lp_scratch_reserve(c, n + c->uplane_max)) return rc;
    if (!c->d_fence && c->mem.get(c->d_fence, 36 * (size_t)c->nrows)) return LQRO_E_NOMEM;
    for (int a = 0; a < 3; ++a) { c->fence_lo[a] = lo[a]; c->fence_hi[a] = hi[a]; }
    c->fence_tau = tau;
  }
  c->nfence = n;
  c->fence_faces = faces;
  return LQRO_OK;
}

// lqro_set_active[_device].  own: `active` is a host array to copy.
static int set_active(lqro_ctx* c, const uint8_t* active, bool own) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step's tail was enqueued under the old mask
  if (int rc = ctx_enter(c, false)) return rc;
  if (!active) {   // the context that never had a mask: no buffer, no launch
    c->mem.release(c->d_actown);
    c->mem.release(c->d_act);
    c->d_actsrc = nullptr;
    return LQRO_OK;
  }
  const size_t N = (size_t)c->cfg.n_agents;
  // every new buffer first: a failed call leaves the context as it was
  unsigned char *copy = nullptr, *act = nullptr;
  int rc = LQRO_OK;
  if (!c->d_act && c->mem.get(act, (N + 3) & ~(size_t)3)) rc = LQRO_E_NOMEM;
  if (!rc && own && c->mem.get(copy, N)) rc = LQRO_E_NOMEM;
  // (the stream the step reads them on may be non-blocking: the copy is synchronous)
  if (!rc && own && hipMemcpy(copy, active, N, hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  if (rc) {
    c->mem.release(act); c->mem.release(copy);
    return rc;
  }
  if (act) c->d_act = act;
  c->mem.release(c->d_actown);
  c->d_actown = copy;
  c->d_actsrc = own ? copy : active;
  return LQRO_OK;
}

int lqro_set_active(lqro_ctx* c, const uint8_t* active) { return set_active(c, active, true); }

int lqro_set_active_device(lqro_ctx* c, const uint8_t* d_active) { return set_active(c, d_active, false); }

// lqro_set_interaction[_device].  own: `cls` is a host array to check and copy.
static int set_interaction(lqro_ctx* c, const uint8_t* cls, int32_t n_classes, const double* share, bool own) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step's tail was enqueued under the old table
  const size_t N = (size_t)c->cfg.n_agents;
  if (cls && share) {
    if (n_classes < 1 || n_classes > LQRO_CLASSES_MAX) return LQRO_E_ARG;
    for (int q = 0; q < n_classes * n_classes; ++q)
      if (!(share[q] >= 0.0 && share[q] <= 1.0)) return LQRO_E_ARG;   // (a NaN fails both)
    if (own)
      for (size_t q = 0; q < N; ++q)
        if (cls[q] >= n_classes) return LQRO_E_ARG;
  }
  if (int rc = ctx_enter(c, false)) return rc;
  if (!cls || !share) {   // the context that never had a table: no buffer, no launch
    c->mem.release(c->d_ixown);
    c->mem.release(c->d_ix);
    c->d_ixsrc = nullptr;
    return LQRO_OK;
  }
  // every new buffer first: a failed call leaves the context as it was
  static_assert(sizeof(((IxDev*)nullptr)->share) == sizeof(double) * LQRO_CLASSES_MAX * LQRO_CLASSES_MAX, "IxDev::share");
  IxDev head{};
  for (int q = 0; q < n_classes * n_classes; ++q) head.share[q] = share[q];
  head.C = n_classes;
  unsigned char *copy = nullptr, *dix = nullptr;
  int rc = LQRO_OK;
  if (c->mem.get(dix, offsetof(IxDev, cls) + ((N + 3) & ~(size_t)3), 0)) rc = LQRO_E_NOMEM;
  if (!rc && own && c->mem.get(copy, N)) rc = LQRO_E_NOMEM;
  // (the stream the step reads them on may be non-blocking: the copies are synchronous)
  if (!rc && hipMemcpy(dix, &head, offsetof(IxDev, cls), hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  if (!rc && own && hipMemcpy(copy, cls, N, hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  if (rc) {
    c->mem.release(dix); c->mem.release(copy);
    return rc;
  }
  c->mem.release(c->d_ix);
  c->d_ix = dix;
  c->mem.release(c->d_ixown);
  c->d_ixown = copy;
  c->d_ixsrc = own ? copy : cls;
  return LQRO_OK;
}

int lqro_set_interaction(lqro_ctx* c, const uint8_t* cls, int32_t n_classes, const double* share) {
  return set_interaction(c, cls, n_classes, share, true);
}

int lqro_set_interaction_device(lqro_ctx* c, const uint8_t* d_cls, int32_t n_classes, const double* share) {
  return set_interaction(c, d_cls, n_classes, share, false);
}

// the interaction table as the step's kernels read it (null: none)
static const IxDev* ix_tab(const lqro_ctx* c) {
  return c->d_ixsrc ? reinterpret_cast<const IxDev*>(c->d_ix) : nullptr;
}

int lqro_set_hard_planes(lqro_ctx* c, int32_t level) {
  if (!c || level < LQRO_HARD_NONE || level > LQRO_HARD_OBSTACLES) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step's LP was planned with the old level
  if (int rc = ctx_enter(c, false)) return rc;
  c->hard_level = level;   // (lp_args and step_shape read it per step; nothing is allocated)
  return LQRO_OK;
}

// lqro_set_obstacles[_ex] / _device.  own: `states` is a host array to copy.
// oxy, oz, resp: one value per obstacle (host).
static int set_obstacles(lqro_ctx* c, const double* states, int M, const double* oxy, const double* oz,
                         const double* resp, bool own) {
  if (!c) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step's tail still reads the slots
  const lqro_config& g = c->cfg;
  if (M <= 0 || !states) M = 0;
  if (M > 0) {
    for (int o = 0; o < M; ++o)
      if (!(oxy[o] >= 0) || !(oz[o] >= 0) || !std::isfinite(oxy[o]) || !std::isfinite(oz[o]) ||
          !(resp[o] > 0 && resp[o] <= 1))
        return LQRO_E_ARG;
    if ((long long)c->nrows * ((long long)g.n_agents - 1 + M) > (long long)INT_MAX) return LQRO_E_ARG;   // (slots are ints)
  }
  if (int rc = ctx_enter(c, false)) return rc;
  const size_t N = g.n_agents, X = g.x_dim, H = g.horizon, NP = g.n_points;
  // the obstacle columns' spheres: createSpheres over the summed radii, the
  // distinct ones found bit for bit; the agents' tables serve a set that is
  // theirs (class 0), the others are classes 1..K in order of first appearance
  std::vector<double> So;    // K x (NP x 3)
  std::vector<double> osc;   // K x (semi-axes, max |u_p|)
  std::vector<int> ocls((size_t)M, 0);
  int K = 0;
  if (M > 0) {
    std::vector<double> S(3 * NP), So_o(3 * NP);
    lqro_sphere((int)NP, g.xy_radius, g.z_radius, S.data());
    for (int o = 0; o < M; ++o) {
      int cl = -1;
      for (int p = 0; p < o && cl < 0; ++p)   // (the same radii: the same set)
        if (memcmp(&oxy[p], &oxy[o], sizeof(double)) == 0 && memcmp(&oz[p], &oz[o], sizeof(double)) == 0) cl = ocls[p];
      if (cl < 0) {
        sphere_axes((int)NP, g.xy_radius + oxy[o], g.z_radius + oz[o], So_o.data());
        if (memcmp(S.data(), So_o.data(), sizeof(double) * 3 * NP) == 0) cl = 0;
        for (int k = 0; k < K && cl < 0; ++k)
          if (memcmp(So.data() + (size_t)k * 3 * NP, So_o.data(), sizeof(double) * 3 * NP) == 0) cl = k + 1;
        if (cl < 0) {
          if (K == LQRO_OBS_SHAPES_MAX) return LQRO_E_ARG;
          So.insert(So.end(), So_o.begin(), So_o.end());
          const double rad[3] = {g.xy_radius + oxy[o], g.xy_radius + oxy[o], g.z_radius + oz[o]};
          osc.insert(osc.end(), rad, rad + 3);
          osc.push_back(sphere_umax(So_o.data(), (int)NP, rad));
          cl = ++K;
        }
      }
      ocls[o] = cl;
    }
  }
  PairArgs pa = c->pa;
  int lds_bytes = 0;
  if (!pair_layout(g, K, pa, lds_bytes)) return LQRO_E_ARG;   // (H x NP leaves no wave a region beside K more spheres)
  // every new buffer first: a failed call leaves the context as it was
  const int npr = (int)N - 1 + M;
  double *cols = nullptr, *copy = nullptr, *dSo = nullptr, *dRo = nullptr, *dresp = nullptr;
  double *clow = nullptr, *clpack = nullptr;   // clearance: the columns' weights; the pack buffer once it exists
  double *ppath = nullptr, *pgiven = nullptr;  // prediction: the path buffers once they exist
  int* dcls = nullptr;
  SlotBufs sb{};
  int rc = LQRO_OK;
  if (M > 0 && (c->mem.get(cols, (N + M) * X) || c->mem.get(dresp, (size_t)M))) rc = LQRO_E_NOMEM;
  if (!rc && M > 0 && own && c->mem.get(copy, (size_t)M * X)) rc = LQRO_E_NOMEM;
  if (!rc && M > 0 && c->mem.get(clow, 2 * (size_t)M)) rc = LQRO_E_NOMEM;
  if (!rc && c->d_clpack && M != c->nobs && c->mem.get(clpack, 5 * (N + M))) rc = LQRO_E_NOMEM;
  if (!rc && c->d_ppath && M != c->nobs && c->mem.get(ppath, 3 * H * (N + M))) rc = LQRO_E_NOMEM;
  if (!rc && c->d_pgiven && M != c->nobs && c->mem.get(pgiven, 3 * H * (N + M))) rc = LQRO_E_NOMEM;
  if (!rc && K > 0 && (c->mem.get(dSo, (size_t)K * (3 * NP + 4)) || c->mem.get(dRo, (size_t)K * N * H) ||
                       c->mem.get(dcls, (size_t)M)))
    rc = LQRO_E_NOMEM;
  if (!rc && npr != c->npr) rc = slots_alloc(c, npr, sb);
  if (!rc && copy && hipMemcpy(copy, states, sizeof(double) * M * X, hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  if (!rc && M > 0 && hipMemcpy(dresp, resp, sizeof(double) * M, hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  if (!rc && M > 0) {   // wxy = 1 / a^2, wz = 1 / b^2 over the summed radii, once, in fp64
    std::vector<double> w(2 * (size_t)M);
    for (int o = 0; o < M; ++o) {
      const double a = g.xy_radius + oxy[o], b = g.z_radius + oz[o];
      w[2 * o] = 1.0 / (a * a);
      w[2 * o + 1] = 1.0 / (b * b);
    }
    if (hipMemcpy(clow, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  }
  if (!rc && K > 0 &&
      (hipMemcpy(dSo, So.data(), sizeof(double) * So.size(), hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(dSo + So.size(), osc.data(), sizeof(double) * osc.size(), hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(dcls, ocls.data(), sizeof(int) * M, hipMemcpyHostToDevice) != hipSuccess))
    rc = LQRO_E_HIP;
  if (!rc && !pair_set_lds(lds_bytes)) rc = LQRO_E_HIP;
  if (rc) {
    c->mem.release(cols); c->mem.release(copy); c->mem.release(dSo); c->mem.release(dRo);
    c->mem.release(dresp); c->mem.release(dcls); c->mem.release(clow); c->mem.release(clpack);
    c->mem.release(ppath); c->mem.release(pgiven);
    slots_release(c, sb);
    (void)pair_set_lds(c->lds_bytes);
    return rc;
  }
  if (npr != c->npr) {
    // every slot number kept across steps is void: the last step's
    // inside-hull list (prevn = 0), the hot and speculation marks (the new
    // buffer is zeroed), the rows' counters; the schedule starts over as in
    // a new context.  The carried normal stays.
    slots_adopt(c, npr, sb);
    if (c->d_hot2) HIPCHK(hipMemset(c->d_hot2, 0, sizeof(int) * LQRO_H2_WORDS));
    HIPCHK(hipMemset(c->d_rowpend, 0, sizeof(int) * 2 * (size_t)c->nrows));
    for (int k = 0; k < 2; ++k) c->h_feedback[k] = kNoFeedback;
    c->nstep = 0;
  }
  c->mem.release(c->d_cols); c->mem.release(c->d_obsown); c->mem.release(c->d_So); c->mem.release(c->d_Ro);
  c->mem.release(c->d_oresp); c->mem.release(c->d_ocls);
  c->mem.release(c->d_clow);
  c->d_clow = clow;
  if (clpack) { c->mem.release(c->d_clpack); c->d_clpack = clpack; }
  if (ppath) { c->mem.release(c->d_ppath); c->d_ppath = ppath; c->pr_kind = 0; }   // (the old paths are gone)
  if (pgiven) { c->mem.release(c->d_pgiven); c->d_pgiven = pgiven; }
  c->d_cols = cols; c->d_obsown = copy; c->d_So = dSo; c->d_Ro = dRo; c->d_oresp = dresp; c->d_ocls = dcls;
  c->d_obs = M > 0 ? (own ? copy : states) : nullptr;
  c->nobs = M;
  c->n_ocls = K;
  pa.n_gain = (int)N;
  pa.ocls = dcls; pa.oresp = dresp;
  pa.So = dSo; pa.osc = K > 0 ? dSo + So.size() : nullptr; pa.Ro = dRo;
  c->pa = pa;
  c->lds_bytes = lds_bytes;
  if (K > 0 && c->have_gains) {   // (else lqro_set_gains builds it with its tables)
    LAUNCH(launch_obs_rtab(c->stream, K, c->per_agent ? (int)N : 1, (int)N, (int)H, c->d_T, pa.osc, c->d_Ro));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return LQRO_OK;
}

// the _ex calls' NULL arrays: the agents' radii, responsibility 1.0
static int set_obstacles_arrays(lqro_ctx* c, const double* states, int M, const double* oxy, const double* oz,
                                const double* resp, bool own) {
  if (!c) return LQRO_E_ARG;
  const size_t m = M > 0 && states ? (size_t)M : 0;
  std::vector<double> dxy, dz, dr;
  if (!oxy) { dxy.assign(m, c->cfg.xy_radius); oxy = dxy.data(); }
  if (!oz) { dz.assign(m, c->cfg.z_radius); oz = dz.data(); }
  if (!resp) { dr.assign(m, 1.0); resp = dr.data(); }
  return set_obstacles(c, states, (int)m, oxy, oz, resp, own);
}

int lqro_set_obstacles_ex(lqro_ctx* c, const double* states, int32_t n_obstacles, const double* xy_radius,
                          const double* z_radius, const double* responsibility) {
  return set_obstacles_arrays(c, states, n_obstacles, xy_radius, z_radius, responsibility, true);
}

int lqro_set_obstacles_ex_device(lqro_ctx* c, const double* d_states, int32_t n_obstacles, const double* xy_radius,
                                 const double* z_radius, const double* responsibility) {
  return set_obstacles_arrays(c, d_states, n_obstacles, xy_radius, z_radius, responsibility, false);
}

// the one-shape calls: their three scalars broadcast
int lqro_set_obstacles(lqro_ctx* c, const double* states, int32_t n_obstacles, double obs_xy_radius,
                       double obs_z_radius, double responsibility) {
  const size_t M = n_obstacles > 0 && states ? (size_t)n_obstacles : 0;
  const std::vector<double> oxy(M, obs_xy_radius), oz(M, obs_z_radius), resp(M, responsibility);
  return set_obstacles(c, states, (int)M, oxy.data(), oz.data(), resp.data(), true);
}

int lqro_set_obstacles_device(lqro_ctx* c, const double* d_states, int32_t n_obstacles, double obs_xy_radius,
                              double obs_z_radius, double responsibility) {
  const size_t M = n_obstacles > 0 && d_states ? (size_t)n_obstacles : 0;
  const std::vector<double> oxy(M, obs_xy_radius), oz(M, obs_z_radius), resp(M, responsibility);
  return set_obstacles(c, d_states, (int)M, oxy.data(), oz.data(), resp.data(), false);
}

int lqro_set_gains(lqro_ctx* c, const double* A, const double* B, const double* L,
                   const double* E, int32_t per_agent) {
  if (!c || !A || !B || !L || !E) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;   // (pending: the half-step reads d_T / d_NCF on the caller's stream;
                                                // a step in flight still reads them too)
  const lqro_config& g = c->cfg;
  const size_t X = g.x_dim, U = g.u_dim, N = g.n_agents;
  const size_t na = per_agent ? N : 1;
  HIPCHK(hipMemcpyAsync(c->d_A, A, sizeof(double) * X * X, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_B, B, sizeof(double) * X * U, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_L, L, sizeof(double) * na * U * X, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_E, E, sizeof(double) * na * U * 3, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
  LAUNCH(launch_tables(c->stream, (int)na, (int)X, (int)U, g.horizon, c->d_A, c->d_B, c->d_L, c->d_E, per_agent ? 1 : 0,
                       c->d_T, c->d_NCF, c->d_R, c->d_TF, c->pa.rad0, c->pa.rad1, c->pa.rad2, c->umax, c->d_err));
  if (c->n_ocls > 0)
    LAUNCH(launch_obs_rtab(c->stream, c->n_ocls, (int)na, (int)N, g.horizon, c->d_T, c->pa.osc, c->d_Ro));
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (err) return LQRO_E_SINGULAR;
  c->per_agent = per_agent ? 1 : 0;
  c->have_gains = 1;
  c->pcg_stale = 1;   // (the next predicting call rebuilds C G_k)
  return LQRO_OK;
}

// the LP launch's arguments for this context's rows (every row, the tail's
// k_lp4 list)
static LpArgs lp_args(const lqro_ctx* c, int npr, const double* d_vgoal, double* d_newv) {
  LpArgs La{};
  La.npr = npr; La.cap = npr + c->nfence + c->uplane_max; La.nrows = c->nrows; La.row_begin = c->rb; La.row_stride = c->rs; La.vmax = c->cfg.vmax_lp;
  La.slots = c->d_planes; La.compact = c->d_lpcompact; La.proj = c->d_lpscratch;
  La.vgoal = d_vgoal; La.newv = d_newv; La.prof = c->d_prof;
  La.lp4_list = c->d_lp4; La.lp4_count = c->d_hcount + LQRO_HC_LP4; La.lp4_next = c->d_hcount + LQRO_HC_LP4_NEXT;
  La.fence = c->d_fence; La.nfence = c->nfence;
  La.uplanes = c->d_uplanes; La.ucounts = c->d_ucounts; La.umax = c->uplane_max;
  // hard planes: at level 3 with obstacles the row's obstacle slots go ahead of its agent slots
  La.hard = c->hard_level;
  La.obs_first = c->hard_level >= LQRO_HARD_OBSTACLES && c->nobs > 0 ? c->cfg.n_agents - 1 : -1;
  La.nbr = c->nbr_k > 0 ? c->d_nbrlist : nullptr;
  La.active = c->d_actsrc ? c->d_act : nullptr;   // (k_active's bytes, written at the head of the step)
  return La;
}

// the LP audit's own arguments (lqro_set_lp_audit)
static LpAuditArgs audit_args(const lqro_ctx* c) {
  LpAuditArgs B{};
  B.tol = c->audit_tol; B.faces = c->nfence > 0 ? c->fence_faces : 0; B.plain = 0;
  B.rows = c->d_aurows; B.tot = c->d_autot;
  return B;
}

// what the planner reads of the context and of the kernels' headers
// (d_lpnv: where an early LP would write, d_newv: the caller's buffer)
static StepShape step_shape(const lqro_ctx* c, int phase, const double* d_lpnv, const double* d_newv) {
  StepShape S{};
  S.n_cu = c->n_cu; S.nrows = c->nrows; S.npr = c->npr - c->nobs; S.n_obs = c->nobs; S.nbr_k = c->nbr_k;
  S.hnp = (size_t)c->cfg.horizon * c->cfg.n_points;
  S.per_agent = c->per_agent; S.qhull_order = c->qhull_order; S.phase = phase;
  S.has_newv = d_lpnv != nullptr; S.newv_is_callers = d_lpnv == d_newv;
  S.waves = c->pa.waves; S.lds_wave = c->pa.lds_wave; S.wave_doubles = c->pa.wave_doubles;
  S.hull_lds_max_hnp = kHullLdsMaxHNP; S.hull_lds_doubles = sizeof(HullMemC) / 8; S.hull_cwaves = HULL_CWAVES;
  S.qhull_lds_doubles = qhull_lds_doubles(); S.lp_lds_max = kLpLdsMax;
  S.early_lp_max_npr = LQRO_EARLY_LP_MAX_NPR; S.row_big = LQRO_ROW_BIG;
  S.extra_planes = c->nfence + c->uplane_max;
  S.hard_obs = c->hard_level >= LQRO_HARD_OBSTACLES && c->nobs > 0 ? 1 : 0;
  return S;
}

// k_pair's arguments for the row launch; the hot launches derive theirs
// (hot_main, hot_side)
static PairArgs pair_args(const lqro_ctx* c, const StepPlan& plan, const double* d_x) {
  const lqro_config& g = c->cfg;
  PairArgs P = c->pa;   // (the LDS layout and the sphere's bounds; the rest zero: no hot list)
  P.N = g.n_agents + c->nobs; P.H = g.horizon; P.NP = g.n_points; P.min_reach = g.min_reach;
  if (c->nobs > 0) {   // (d_x: the context's column array; else obs_jj stays INT_MAX)
    P.obs_jj = g.n_agents - 1;   // (the classes' arrays: c->pa, lqro_set_obstacles)
  }
  P.row_begin = c->rb; P.row_stride = c->rs; P.nrows = c->nrows; P.npr = plan.npr;
  P.per_agent = c->per_agent;
  P.vmax = g.vmax_reach;
  P.r2 = g.vmax_reach * g.vmax_reach;
  P.r2_lo = P.r2 * (1.0 - 1e-12);
  P.r2_hi = P.r2 * (1.0 + 1e-12);
  P.T = c->d_T; P.NCF = c->d_NCF; P.R = c->d_R; P.TF = c->d_TF; P.S = c->d_S;
  P.shash = c->d_shash; P.x = d_x;
  P.planes = c->d_planes; P.recs = c->d_recs;
  P.hull_queue = c->d_hq; P.hull_count = c->d_hcount + LQRO_HC_HULL; P.hull_cap = c->hull_cap;
  P.stats = c->d_stats;
  P.prof = c->d_prof + LQRO_PROF_PAIR;
  P.row_counter = c->d_hcount + LQRO_HC_ROW;
  P.row_split = plan.row_split;
  P.qnrm = c->qhull_order ? c->d_qnrm : nullptr;
  P.nbr_list = c->nbr_k > 0 ? c->d_nbrlist : nullptr;   // (k_nbr fills it)
  P.rowpend = plan.early ? c->d_rowpend : nullptr;
  P.active = c->d_actsrc ? c->d_act : nullptr;
  P.ix = ix_tab(c);
  if (plan.hot) {
    P.hot_list = c->d_hotlist; P.hot_mark = c->d_hotmark; P.hot_count = c->d_hcount + LQRO_HC_HOT;
    P.hot_next = c->d_hcount + LQRO_HC_HOT_NEXT; P.hot_cap = c->hot_cap;
  }
  return P;
}

// the split's hot launch on the main stream: k_prio's pairs after the last step's
static PairArgs hot_main(const lqro_ctx* c, const StepPlan& plan, PairArgs P) {
  P.hot_only = 1;
  P.hot_next = c->d_hot2 + LQRO_H2_HOT2_NEXT;
  P.hot_done = c->d_hot2 + LQRO_H2_HOT2_DONE;
  if (plan.spec) P.spec_mark = c->d_hotmark;   // (its list from position 0: the speculative pairs first)
  return P;
}

// the side stream's hot launch: the whole hot list, or with the split the
// last step's inside-hull pairs
static PairArgs hot_side(const lqro_ctx* c, const StepPlan& plan, PairArgs P) {
  P.hot_only = 1;
  if (plan.split) { P.hot_count = c->d_hot2 + LQRO_H2_HOT1; P.hot_next = c->d_hot2 + LQRO_H2_HOT1_NEXT; }
  return P;
}

static PrioArgs prio_args(const lqro_ctx* c, const StepPlan& plan, const PairArgs& P) {
  PrioArgs Q{};
  Q.npr = c->npr; Q.nrows = c->nrows; Q.row_begin = c->rb; Q.row_stride = c->rs; Q.X = c->cfg.x_dim; Q.x = P.x;
  Q.t_hot = c->knobs.hot_t; Q.r2_hot = c->knobs.hot_r * c->knobs.hot_r;   // seconds, metres (scheduling heuristic)
  Q.list = c->d_hotlist; Q.mark = c->d_hotmark; Q.count = c->d_hcount + LQRO_HC_HOT; Q.cap = c->hot_cap;
  Q.rowpend = P.rowpend;
  Q.act = P.active; Q.n_agents = c->cfg.n_agents; Q.ix = P.ix;
  if (plan.split) {
    Q.prev = c->d_prevq; Q.prevn = c->d_hot2 + LQRO_H2_PREV; Q.hot1n = c->d_hot2 + LQRO_H2_HOT1;
    Q.hot2next = c->d_hot2 + LQRO_H2_HOT2_NEXT;
    if (plan.spec) { Q.hq = c->d_hq; Q.hcount = c->d_hcount; Q.hq_cap = c->hull_cap; Q.spec_n = c->d_hot2 + LQRO_H2_SPEC; }
  }
  return Q;
}

// the hull kernels' arguments (every family reads the same struct): the main
// queue, block 0's scratch; the variants below derive from it
static HullArgs hull_args(const lqro_ctx* c, const StepPlan& plan, const PairArgs& P, const double* d_vgoal,
                          double* d_lpnv) {
  const lqro_config& g = c->cfg;
  HullArgs Hh{};   // (block 0's scratch, no external points: zero)
  Hh.N = g.n_agents + c->nobs; Hh.X = g.x_dim; Hh.H = g.horizon; Hh.NP = g.n_points;
  if (c->nobs > 0) { Hh.So = P.So; Hh.ocls = P.ocls; Hh.oresp = P.oresp; Hh.obs_jj = P.obs_jj; }
  Hh.row_begin = c->rb; Hh.row_stride = c->rs; Hh.npr = plan.npr; Hh.per_agent = c->per_agent;
  Hh.nbr_list = P.nbr_list;
  Hh.ix = P.ix;
  Hh.r2 = P.r2; Hh.r2_lo = P.r2_lo; Hh.r2_hi = P.r2_hi;
  Hh.T = c->d_T; Hh.NCF = c->d_NCF; Hh.S = c->d_S; Hh.x = P.x;
  Hh.planes = c->d_planes; Hh.recs = c->d_recs;
  Hh.queue = c->d_hq; Hh.count = c->d_hcount + LQRO_HC_HULL; Hh.cap = c->hull_cap;
  Hh.next = c->d_hcount + LQRO_HC_HULL_NEXT;
  Hh.scratch = c->d_hscratch; Hh.iscratch = c->d_hiscratch; Hh.fscratch = c->d_hfscratch;
  Hh.sb = c->d_hfaces;
  Hh.fbest = c->d_hfbest;
  Hh.vpid = c->d_hvpid; Hh.stack = c->d_hstack;
  Hh.rqueue = c->d_rq; Hh.rcount = c->d_hcount + LQRO_HC_RETRY; Hh.rnext = c->d_hcount + LQRO_HC_RETRY_NEXT;
  Hh.bigmem = c->d_hbig;
  Hh.wide = c->d_hwide;
  Hh.bag = c->d_hbag;
  Hh.stats = c->d_stats;
  Hh.prof = c->d_prof;
  Hh.lqueue = c->d_lq; Hh.lcount = c->d_hcount + LQRO_HC_LHAND; Hh.ldone = c->d_hcount + LQRO_HC_LDONE;
  Hh.lfail = c->d_prof + LQRO_PROF_LFAIL;
  // per-job stamps only when asked for (LQRO_LHULL_PROFILE=1, scripts/lhull_jobs.py);
  // lfail counts hand-over reasons since the context was created
  Hh.ljobs = c->knobs.lhull_prof ? c->d_prof + LQRO_PROF_LJOBS : nullptr;
  Hh.qscratch = c->d_qscratch; Hh.qstride = c->qstride; Hh.qnrm = c->d_qnrm;
  Hh.qstale = c->d_qstale; Hh.qstale_count = c->d_hcount + LQRO_HC_FACET0; Hh.qstale_cap = c->hull_cap;
  Hh.rowpend = P.rowpend; Hh.rowclaim = plan.early ? c->d_rowclaim : nullptr;
  Hh.row_lp = plan.row_lp;
  Hh.row_target = plan.row_target;
  Hh.lp_vgoal = d_vgoal; Hh.lp_newv = d_lpnv; Hh.lp_vmax = g.vmax_lp;
  Hh.hbuild = c->d_hbuild; Hh.hbuild_cap = LQRO_HBUILD_CAP;
  Hh.big_inline = plan.big_inline;
  Hh.qflags = c->knobs.qhull_flags;
  return Hh;
}

// the obstacle columns among a row's slots, for k_stale / k_stale_rows
static ObsSlots obs_slots(const lqro_ctx* c) {
  ObsSlots O{};
  if (c->nobs > 0) {
    O.resp = c->d_oresp;
    O.jj = c->cfg.n_agents - 1;
  }
  O.ix = ix_tab(c);
  if (c->nobs > 0 || O.ix) O.nbr_list = c->nbr_k > 0 ? c->d_nbrlist : nullptr;
  return O;
}

// speculative builds: the marks, and the ticket over the jobs k_prio_prev queued
static HullArgs with_spec(const lqro_ctx* c, HullArgs H) {
  H.spec_mark = c->d_hotmark; H.spec_n = c->d_hot2 + LQRO_H2_SPEC; H.spec_next = c->d_hot2 + LQRO_H2_SPEC_NEXT;
  return H;
}

// the full hull on the pairs k_lhull handed over instead of the main queue
static HullArgs handed_over(const lqro_ctx* c, HullArgs H) {
  H.queue = c->d_lq; H.count = c->d_hcount + LQRO_HC_LHAND; H.next = c->d_hcount + LQRO_HC_LHAND_NEXT;
  return H;
}

// One clearance measurement on s: the agents of d_x and the context's
// obstacles against the own rows, into `rows`; the totals folded.  The caller
// has ordered s behind the last step; the buffers exist.
static int enqueue_clear(lqro_ctx* c, const double* d_x, lqro_clearance_row* rows, hipStream_t s,
                         hipEvent_t* ev = nullptr) {
  const lqro_config& g = c->cfg;
  if (c->measured) HIPCHK(hipStreamWaitEvent(s, c->cev, 0));   // (the last measurement may be on another stream)
  ClearArgs A{};
  A.n_agents = g.n_agents; A.nobs = c->nobs; A.X = g.x_dim;
  A.nrows = c->nrows; A.row_begin = c->rb; A.row_stride = c->rs;
  A.x = d_x; A.obs = c->d_obs; A.ow = c->d_clow;
  const double a = g.xy_radius + g.xy_radius, b = g.z_radius + g.z_radius;   // createSpheres' 2 XYRADIUS, 2 ZRADIUS
  A.wxy = 1.0 / (a * a); A.wz = 1.0 / (b * b);
  A.pack = c->d_clpack;
  A.faces = c->nfence > 0 ? c->fence_faces : 0;
  for (int q = 0; q < 3; ++q) {
    A.lo[q] = c->fence_lo[q]; A.hi[q] = c->fence_hi[q]; A.m[q] = q < 2 ? g.xy_radius : g.z_radius;
  }
  A.rows = rows; A.tot = c->d_cltot;
  A.active = c->d_actsrc;   // (the caller's bytes: an explicit measurement runs without a step)
  LAUNCH(launch_clear(s, A, ev));
  HIPCHK(hipEventRecord(c->cev, s));
  c->measured = 1;
  c->cl_last = rows;
  return LQRO_OK;
}

// The step's first launches on the caller's stream: behind the last step, the
// counters and queues reset, the neighbour lists, the hot list.
static int enqueue_prologue(lqro_ctx* c, const StepPlan& plan, const PairArgs& P, const double* d_x, hipStream_t s) {
  const lqro_config& g = c->cfg;
  // the context's scratch (queues, counters, plane slots, tables) is reused by
  // every step: a step enqueued on another stream than the last one, or a
  // set_gains on c->stream, must not overlap the step still in flight
  if (c->stepped) HIPCHK(hipStreamWaitEvent(s, c->ev[3], 0));
  HIPCHK(hipEventRecord(c->ev[0], s));
  HIPCHK(hipMemsetAsync(c->d_hcount, 0, sizeof(int) * LQRO_HC_WORDS, s));
  HIPCHK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * LQRO_ST_WORDS, s));
  HIPCHK(hipMemsetAsync(c->d_hq, 0xFF, sizeof(int) * (size_t)c->hull_cap, s));
  // obstacles: this step's columns (P.x), the caller's agents then the obstacles
  if (c->nobs > 0)
    LAUNCH(launch_cols(s, d_x, (size_t)g.n_agents * g.x_dim, c->d_obs, (size_t)c->nobs * g.x_dim, c->d_cols));
  // Qhull order: the normal the last step's last eligible pair left enters this step
  if (c->qhull_order)
    HIPCHK(hipMemcpyAsync(c->d_carry, c->d_carry + 3, sizeof(double) * 3, hipMemcpyDeviceToDevice, s));
  // the activity mask and the interaction table: this step's bytes, its pairs counter, the carried-over list
  // without the pairs that left or are ignored now
  if (c->d_actsrc || c->d_ixsrc) {
    ActiveArgs Aa{};
    if (c->d_actsrc) { Aa.src = c->d_actsrc; Aa.act = c->d_act; }
    if (c->d_ixsrc) { Aa.clsrc = c->d_ixsrc; Aa.ix = reinterpret_cast<IxDev*>(c->d_ix); }
    Aa.n_agents = g.n_agents; Aa.n_obs = c->nobs; Aa.npr = c->npr;
    Aa.nrows = c->nrows; Aa.row_begin = c->rb; Aa.row_stride = c->rs;
    Aa.pairs = c->nbr_k > 0 ? nullptr : c->d_stats + LQRO_ST_PAIRS;
    if (c->qhull_order) { Aa.prev = c->d_prevq; Aa.prevn = c->d_hot2 + LQRO_H2_PREV; Aa.cap = c->hot_cap; }
    LAUNCH(hipLaunchKernelGGL(k_active, dim3(1), dim3(256), 0, s, Aa));
  }
  if (c->nbr_k > 0) {
    LAUNCH(hipLaunchKernelGGL(k_nbr, dim3((unsigned)c->nrows), dim3(64), 0, s, P.x, g.x_dim, g.n_agents + c->nobs, c->rb, c->rs,
                              c->npr, c->nbr_r2, c->nbr_k, plan.npr, c->d_nbrlist, c->d_stats, P.active, g.n_agents, P.ix));
  }
  if (plan.early) HIPCHK(hipMemsetAsync(c->d_rowpend, 0, sizeof(int) * 2 * (size_t)c->nrows, s));
  if (c->nfence > 0) {   // this step's fence planes, before any LP can start
    FenceArgs F{};
    F.nrows = c->nrows; F.row_begin = c->rb; F.row_stride = c->rs; F.X = g.x_dim;
    F.nfence = c->nfence; F.faces = c->fence_faces; F.tau = c->fence_tau;
    for (int a = 0; a < 3; ++a) {
      F.lo[a] = c->fence_lo[a]; F.hi[a] = c->fence_hi[a]; F.m[a] = a < 2 ? g.xy_radius : g.z_radius;
    }
    F.x = P.x; F.out = c->d_fence;
    LAUNCH(launch_fence(s, F));
  }
  // the monitor: this step's own columns, behind k_cols and k_fence; nothing in the step reads it
  if (c->monitor)
    if (int rc = enqueue_clear(c, d_x, c->d_clrows, s)) return rc;
  if (plan.hot) {
    const PrioArgs Q = prio_args(c, plan, P);
    if (plan.split) {
      HIPCHK(hipMemsetAsync(c->d_hot2 + LQRO_H2_HOT1, 0, sizeof(int) * (LQRO_H2_SPEC_NEXT - LQRO_H2_HOT1 + 1), s));
      LAUNCH(hipLaunchKernelGGL(k_prio_prev, dim3(1), dim3(256), 0, s, Q));
    }
    const long nb = std::min<long>((plan.slots + 255) / 256, 8L * c->n_cu);
    if (Q.act || Q.ix) LAUNCH(hipLaunchKernelGGL(k_prio<true>, dim3((unsigned)nb), dim3(256), 0, s, Q));
    else LAUNCH(hipLaunchKernelGGL(k_prio<false>, dim3((unsigned)nb), dim3(256), 0, s, Q));
  }
  return LQRO_OK;
}

// The side stream (plan.nwait workgroups, one a CU): the hot pairs, their
// hulls, then its share of the row sweep.
static int enqueue_side(lqro_ctx* c, const StepPlan& plan, const PairArgs& P, const HullArgs& Hh) {
  const int x_dim = c->cfg.x_dim, nwait = plan.nwait;
  const dim3 pair_block(P.waves * 64);
  if (!plan.spec) {   // (speculative builds: the side goes straight to k_qhull)
    LAUNCH(launch_pair(x_dim, dim3(nwait), pair_block, c->lds_bytes, c->side, hot_side(c, plan, P)));
  }
  if (c->qhull_order) {
    // the hot pairs' hulls in Qhull's order (k_qhull leaves when the queue
    // is empty), then the row sweep
    if (plan.qside) {
      PairArgs Pq = P;
      Pq.max_waves = plan.qside_waves;
      if (plan.nside == 0 || pair_masked(P)) Pq.nrows = 0;   // (under a mask or a table the main stream's row launch sweeps every row)
      LAUNCH(launch_qside(x_dim, dim3(std::min(nwait, c->qworkers)), c->side, Hh, Pq));
    } else {
      if (!c->knobs.qhull_big) {
        HullArgs Hs = plan.spec ? with_spec(c, Hh) : Hh;
        if (plan.split) { Hs.prod_done = c->d_hot2 + LQRO_H2_HOT2_DONE; Hs.prod_total = (int)plan.nblk; }
        LAUNCH(launch_qhull(dim3(std::min(nwait, c->qworkers)), c->side, Hs));
      }
      if (plan.nside > 0) LAUNCH(launch_pair(x_dim, dim3(nwait), pair_block, c->lds_bytes, c->side, P));
    }
  } else if (c->knobs.local_hull) {
    // the hot pairs' local hulls (k_lhull leaves when the queue is empty:
    // later jobs go to the k_lhull after the sweep), then the row sweep
    LAUNCH(launch_lhull(dim3(nwait), c->side, Hh));
    if (plan.lds_ok) {
      // the pairs it handed over (rare: near-coplanar input) in the full
      // hull right away, still beside the sweep (scratch blocks 0..nwait-1;
      // the k_hull after the sweep uses nwait.. and starts after the side)
      LAUNCH(launch_hull(dim3(nwait), c->side, handed_over(c, Hh)));
    }
    if (plan.nside > 0) LAUNCH(launch_pair(x_dim, dim3(nwait), pair_block, c->lds_bytes, c->side, P));
  } else {
    PairArgs Pt = P;
    Pt.max_waves = plan.side_waves;
    if (plan.nside == 0 || pair_masked(P)) Pt.nrows = 0;   // (as k_qside's tail)
    LAUNCH(launch_side(x_dim, dim3(nwait), dim3(HULL_CTHREADS), c->side, Hh, Pt));
  }
  return LQRO_OK;
}

// k_hull on H's queue beside the side's scratch blocks, then k_hull_big for
// what its LDS could not hold (or, without the LDS hull, for the whole queue)
static int enqueue_full_hulls(lqro_ctx* c, const StepPlan& plan, HullArgs H, hipStream_t s) {
  H.block_base = plan.nwait;
  H.big_main = plan.lds_ok ? 0 : 1;
  if (plan.lds_ok) LAUNCH(launch_hull(dim3(c->hull_blocks - plan.nwait), s, H));
  H.block_base = 0;
  LAUNCH(launch_hull_big(dim3(c->hull_big_blocks), s, H));
  return LQRO_OK;
}

// The main stream once the sweep and the side are done: every hull job left.
static int enqueue_hulls_after_sweep(lqro_ctx* c, const StepPlan& plan, const HullArgs& Hh, hipStream_t s, int phase) {
  const lqro_config& g = c->cfg;
  if (c->qhull_order) {
    // every hull job left, the ones beyond k_qhull's caps, then the facet-0
    // pairs' loop-carried normals
    HullArgs Hq = plan.spec ? with_spec(c, Hh) : Hh;   // (a speculative job not taken on the side)
    if (!c->knobs.qhull_big) LAUNCH(launch_qhull(dim3(c->qworkers), s, Hq));
    Hq.big_main = c->knobs.qhull_big;
    LAUNCH(launch_qhull_big(dim3(c->qworkers), s, Hq));
    // this step's inside-hull pairs head the next step's hot list
    LAUNCH(hipLaunchKernelGGL(k_prio_save, dim3(1), dim3(256), 0, s, c->d_hq, c->d_hcount + LQRO_HC_HULL, c->hull_cap,
                              c->d_prevq, c->d_hot2 + LQRO_H2_PREV, c->hot_cap,
                              plan.spec ? (const unsigned char*)c->d_hotmark : nullptr,
                              (const unsigned long long*)c->d_hbuild, (const unsigned long long*)(c->d_stats + LQRO_ST_NBUILD),
                              (int)LQRO_HBUILD_CAP, c->d_hotlist, c->d_hot2 + LQRO_H2_HOT1,
                              plan.split ? c->d_hotmark : nullptr, plan.slots));
    if (phase == 0) {
      LAUNCH(launch_stale(s, c->d_planes, c->d_qnrm, c->d_qstale, c->d_hcount + LQRO_HC_FACET0, c->hull_cap, Hh.x, g.x_dim,
                          plan.npr, c->rb, c->rs, c->d_carry, c->d_recs, plan.slots, obs_slots(c)));
    }
    return LQRO_OK;
  }
  if (c->knobs.local_hull) {
    // k_lhull takes the queue k_pair filled; k_hull / k_hull_big then take
    // the pairs it handed over (scratch: hull_blocks blocks of 6 H*NP doubles)
    LAUNCH(launch_lhull(dim3(c->hull_blocks), s, Hh));
    return enqueue_full_hulls(c, plan, handed_over(c, Hh), s);
  }
  return enqueue_full_hulls(c, plan, Hh, s);
}

// The step's second part (all of lqro_step_device_end): the facet-0 pairs of
// row shards against every rank's rows, the LP, the feedback for the schedule.
static int enqueue_tail(lqro_ctx* c, const double* d_x, const double* d_vgoal, double* d_newv, hipStream_t s,
                        const double* d_rowtab) {
  const lqro_config& g = c->cfg;
  const int npr = c->nbr_k > 0 ? std::min(c->nbr_k, c->npr) : c->npr;
  const long slots = (long)c->nrows * npr;
  const int slot = (int)(c->nstep & 1);
  if (d_rowtab && c->qhull_order) {
    LAUNCH(launch_stale_rows(s, c->d_planes, c->d_qnrm, c->d_qstale, c->d_hcount + LQRO_HC_FACET0, c->hull_cap, d_x, g.x_dim, npr,
                             c->rb, c->rs, d_rowtab, g.n_agents, c->d_carry, c->d_recs, slots, obs_slots(c)));
  }
  c->pending = 0;
  LpArgs La = lp_args(c, npr, d_vgoal, d_newv);
  if (c->early_step) {   // the rows the early LP ran are done
    La.rowclaim = c->d_rowclaim;
    La.mode = 2;
  }
  HIPCHK(launch_lp(La, s));
  if (c->early_step && c->early_internal && d_newv != c->d_newv) {   // the rows the early LP ran, into the caller's newV
    LAUNCH(launch_copy_claimed(s, c->d_rowclaim, c->nrows, c->rb, c->rs, c->d_newv, d_newv));
  }
  // the audit: this step's result against the lists its LP read; nothing in the step reads it
  c->au_vgoal = d_vgoal; c->au_newv = d_newv;
  if (c->lp_audit) {
    LAUNCH(launch_lp_audit(s, lp_args(c, npr, d_vgoal, d_newv), audit_args(c)));
    c->audited = 1;
  }
  // this step's work, for the schedule of the step two after it
  StepFeedback* fb = c->h_feedback + slot;
  static_assert(offsetof(StepFeedback, build_max) - offsetof(StepFeedback, sweep_work) ==
                    (LQRO_ST_BMAX - LQRO_ST_SWORK) * sizeof(unsigned long long),
                "LQRO_ST_SWORK, _BWORK, _BMAX in one copy");
  HIPCHK(hipMemcpyAsync(&fb->inside, c->d_stats + LQRO_ST_INSIDE, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&fb->sweep_work, c->d_stats + LQRO_ST_SWORK, 3 * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&fb->retried, c->d_stats + LQRO_ST_RETRY, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(c->iev[slot], s));
  HIPCHK(hipEventRecord(c->ev[3], s));
  c->stepped = 1;
  c->nstep++;
  return LQRO_OK;
}

// phase 0: the whole step.  Row shards in Qhull order split it around the
// exchange of the loop-carried normal (lqro_step_device_begin / _end):
// phase 1 runs the sweep and the hulls and writes each own row's last
// normal into d_rowtab; phase 2 (enqueue_tail) resolves the facet-0 pairs
// against every rank's rows and runs the LP.
//
// persistent: one workgroup per CU (LDS-bound), rows off a queue.
//   main:  k_prio -> k_pair(rows, n_cu - side blocks) -> [side done] -> k_hull -> k_hull_big -> k_lp
//   side:  [k_prio done] -> k_pair(hot, side blocks) -> k_side(hot hulls, then rows)
// The hot launch computes the pairs k_prio predicts to be inside-hull, so
// their hulls run on the side CUs while the row launch sweeps the rest on
// the others; each side workgroup joins the sweep as soon as the hull
// queue is drained.  No kernel waits on another running kernel (streams
// sharing a hardware queue just serialise), and the two concurrent grids
// add up to one workgroup per CU.  Hull jobs the prediction missed are
// taken by the hulls after the sweep.  Which of this a step does is
// plan_step's decision (lqro_plan.hpp).
static int enqueue_step(lqro_ctx* c, const double* d_x, const double* d_vgoal, double* d_newv,
                        hipStream_t s, int phase = 0, double* d_rowtab = nullptr) {
  const lqro_config& g = c->cfg;
  if (g.x_dim != 16 && g.x_dim != 12) return LQRO_E_ARG;
  // 1. the schedule, from the work of the step two before: its copy into the
  // pinned slot has completed once its event has (the host runs at most one
  // step ahead of the GPU here), so the schedule does not depend on host/GPU
  // timing
  const int slot = (int)(c->nstep & 1);
  StepFeedback fb = kNoFeedback;
  if (c->nstep >= 2) {
    HIPCHK(hipEventSynchronize(c->iev[slot]));
    fb = c->h_feedback[slot];
  }
  double* d_lpnv = d_newv != nullptr ? d_newv : (phase == 1 ? c->d_newv : nullptr);   // the early LP's newV
  const StepPlan plan = plan_step(step_shape(c, phase, d_lpnv, d_newv), c->knobs, fb, fb.inside != ~0ull);
  c->early_step = plan.early ? 1 : 0;
  c->act_step = c->d_actsrc || c->d_ixsrc ? 1 : 0;
  c->early_internal = plan.early_internal ? 1 : 0;
  // 2. the kernels' arguments
  const PairArgs P = pair_args(c, plan, c->nobs > 0 ? c->d_cols : d_x);   // (k_cols fills d_cols in the prologue)
  const HullArgs Hh = hull_args(c, plan, P, d_vgoal, d_lpnv);
  // 3. the launches
  if (int rc = enqueue_prologue(c, plan, P, d_x, s)) return rc;
  // the row launch is submitted before the side stream's work: should the two
  // streams land on one hardware queue (a second context in the process), the
  // main grid still runs first on its CUs instead of k_side's row tail
  // sweeping every row on the side CUs alone
  if (plan.nwait > 0) HIPCHK(hipEventRecord(c->xev[0], s));
  if (plan.split) LAUNCH(launch_pair(g.x_dim, dim3(plan.nblk), dim3(P.waves * 64), c->lds_bytes, s, hot_main(c, plan, P)));
  LAUNCH(launch_pair(g.x_dim, dim3(plan.nblk), dim3(P.waves * 64), c->lds_bytes, s, P));
  if (plan.early) {
    // the rows the main sweep closed (no open hull): their LP on its CUs
    // while the side stream's hulls run
    LpArgs Le = lp_args(c, plan.npr, d_vgoal, d_lpnv);
    Le.rowpend = c->d_rowpend; Le.rowclaim = c->d_rowclaim; Le.row_target = plan.row_target; Le.mode = 1;
    Le.lp4_list = nullptr;   // (its linearProgram4 inline)
    HIPCHK(launch_lp(Le, s, true));
  }
  if (plan.nwait > 0) {
    HIPCHK(hipStreamWaitEvent(c->side, c->xev[0], 0));
    if (int rc = enqueue_side(c, plan, P, Hh)) return rc;
    HIPCHK(hipEventRecord(c->xev[1], c->side));
    HIPCHK(hipStreamWaitEvent(s, c->xev[1], 0));
  }
  HIPCHK(hipEventRecord(c->ev[1], s));
  if (int rc = enqueue_hulls_after_sweep(c, plan, Hh, s, phase)) return rc;
  HIPCHK(hipEventRecord(c->ev[2], s));
  if (phase == 1) {
    // each own row's last normal (none without Qhull order)
    LAUNCH(launch_rowlast(s, c->qhull_order ? c->d_planes : nullptr, c->d_qnrm, plan.npr, c->nrows, c->rb, c->rs, d_rowtab));
    c->pend_x = d_x;
    c->pend_vgoal = d_vgoal;
    c->pend_stream = s;
    c->pending = 1;
    return LQRO_OK;
  }
  return enqueue_tail(c, d_x, d_vgoal, d_newv, s, nullptr);
}

// `stream` is the caller's HIP stream; NULL is the default (null) stream, as
// in lqro_dynamics_step_device, so the step is ordered with the work the
// caller (e.g. torch's default stream, RCCL's waits on it) has on it.
int lqro_step_device(lqro_ctx* c, const double* d_x, const double* d_vgoal, double* d_newv,
                     void* stream) {
  if (!c || !d_x || !d_vgoal || !d_newv) return LQRO_E_ARG;
  if (!c->have_gains || c->pending) return LQRO_E_STATE;
  HIPCHK(hipSetDevice(c->cfg.device));
  return enqueue_step(c, d_x, d_vgoal, d_newv, (hipStream_t)stream);
}

int lqro_step_device_begin(lqro_ctx* c, const double* d_x, const double* d_vgoal, double* d_rowtab, void* stream) {
  if (!c || !d_x || !d_vgoal || !d_rowtab) return LQRO_E_ARG;
  if (!c->have_gains || c->pending) return LQRO_E_STATE;
  HIPCHK(hipSetDevice(c->cfg.device));
  return enqueue_step(c, d_x, d_vgoal, nullptr, (hipStream_t)stream, 1, d_rowtab);
}

int lqro_step_device_end(lqro_ctx* c, const double* d_rowtab, double* d_newv, void* stream) {
  if (!c || !d_rowtab || !d_newv) return LQRO_E_ARG;
  if (!c->pending) return LQRO_E_STATE;
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  if (s != c->pend_stream) {   // the begin's work first
    HIPCHK(hipEventRecord(c->xev[0], c->pend_stream));
    HIPCHK(hipStreamWaitEvent(s, c->xev[0], 0));
  }
  return enqueue_tail(c, c->pend_x, c->pend_vgoal, d_newv, s, d_rowtab);
}

int lqro_step(lqro_ctx* c, const double* x, const double* vgoal, double* newv) {
  if (!c || !x || !vgoal || !newv) return LQRO_E_ARG;
  if (!c->have_gains || c->pending) return LQRO_E_STATE;
  const lqro_config& g = c->cfg;
  HIPCHK(hipSetDevice(g.device));
  const size_t N = g.n_agents, X = g.x_dim;
  HIPCHK(hipMemcpyAsync(c->d_x, x, sizeof(double) * N * X, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_vgoal, vgoal, sizeof(double) * N * 3, hipMemcpyHostToDevice, c->stream));
  int rc = enqueue_step(c, c->d_x, c->d_vgoal, c->d_newv, c->stream);
  if (rc) return rc;
  if (c->rs == 1) {
    HIPCHK(hipMemcpyAsync(newv + (size_t)c->rb * 3, c->d_newv + (size_t)c->rb * 3,
                          sizeof(double) * 3 * c->nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {   // cyclic rows: the whole array, then this context's rows
    std::vector<double> all(N * 3);
    HIPCHK(hipMemcpyAsync(all.data(), c->d_newv, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->nrows; ++r) {
      const size_t i = (size_t)c->rb + (size_t)r * c->rs;
      for (int q = 0; q < 3; ++q) newv[3 * i + q] = all[3 * i + q];
    }
  }
  int hc = 0;
  HIPCHK(hipMemcpy(&hc, c->d_hcount + LQRO_HC_HULL, sizeof(int), hipMemcpyDeviceToHost));
  if (hc > c->hull_cap) return LQRO_E_OVERFLOW;
  // a pair whose hull the kernels could not build has no half-plane: the
  // step says so (the reference always gets a hull from qconvex, LQRO:879-880)
  unsigned long long st[LQRO_ST_FAILS];
  HIPCHK(hipMemcpy(st, c->d_stats, sizeof st, hipMemcpyDeviceToHost));
  if (st[LQRO_ST_HULLFAIL]) return LQRO_E_HULL;
  // a pair whose winner qconvex may have merged (Qhull's pre-merge is not
  // restated): never a silent difference from the reference (LQRO:925-967)
  if (st[LQRO_ST_MWIN]) return LQRO_E_QHMERGE;
  return LQRO_OK;
}

// ---- clearance -----------------------------------------------------------
static const lqro_clearance_total kClearNone = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val(),
                                                -1, -1, -1, -1, -1, -1, 0, 0, 0, 0};

static bool clear_radii_ok(const lqro_ctx* c) {
  const double a = c->cfg.xy_radius, b = c->cfg.z_radius;
  return a > 0 && b > 0 && std::isfinite(a) && std::isfinite(b);
}

// the measurement's buffers, once; the caller has waited for the last step
static int clear_reserve(lqro_ctx* c) {
  if (c->d_cltot) return LQRO_OK;
  double* pack = nullptr;
  lqro_clearance_row* rows = nullptr;
  lqro_clearance_total* tot = nullptr;
  if (c->mem.get(pack, 5 * ((size_t)c->cfg.n_agents + c->nobs)) || c->mem.get(rows, (size_t)c->nrows) ||
      c->mem.get(tot, 2)) {
    c->mem.release(pack); c->mem.release(rows);
    return LQRO_E_NOMEM;
  }
  const lqro_clearance_total t[2] = {kClearNone, kClearNone};
  if (hipMemcpy(tot, t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) {
    c->mem.release(pack); c->mem.release(rows); c->mem.release(tot);
    return LQRO_E_HIP;
  }
  c->d_clpack = pack; c->d_clrows = rows; c->d_cltot = tot;
  return LQRO_OK;
}

int lqro_set_monitor(lqro_ctx* c, int32_t on) {
  if (!c || (on != 0 && on != 1)) return LQRO_E_ARG;
  if (on && !clear_radii_ok(c)) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step measured, or did not, as it was set
  if (int rc = ctx_enter(c, false)) return rc;
  if (on)
    if (int rc = clear_reserve(c)) return rc;
  c->monitor = on;
  return LQRO_OK;
}

int lqro_clearance_device(lqro_ctx* c, const double* d_x, lqro_clearance_row* d_rows, void* stream) {
  if (!c || !d_x || !clear_radii_ok(c)) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;
  HIPCHK(hipSetDevice(c->cfg.device));
  if (!c->d_cltot) {   // the first call that needs the buffers: after the last step; later calls never wait
    HIPCHK(wait_last_step(c));
    if (int rc = clear_reserve(c)) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  if (c->stepped) HIPCHK(hipStreamWaitEvent(s, c->ev[3], 0));   // behind the context's last step
  return enqueue_clear(c, d_x, d_rows ? d_rows : c->d_clrows, s);
}

int lqro_clearance(lqro_ctx* c, const double* x, lqro_clearance_row* rows, lqro_clearance_total* total) {
  if (!c || !x || !clear_radii_ok(c)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  if (int rc = clear_reserve(c)) return rc;
  const lqro_config& g = c->cfg;
  HIPCHK(hipMemcpyAsync(c->d_x, x, sizeof(double) * (size_t)g.n_agents * g.x_dim, hipMemcpyHostToDevice, c->stream));
  if (int rc = enqueue_clear(c, c->d_x, c->d_clrows, c->stream)) return rc;
  if (rows)
    HIPCHK(hipMemcpyAsync(rows, c->d_clrows, sizeof(lqro_clearance_row) * (size_t)c->nrows, hipMemcpyDeviceToHost,
                          c->stream));
  if (total) HIPCHK(hipMemcpyAsync(total, c->d_cltot, sizeof *total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return LQRO_OK;
}

// scripts/clearance_bench.py: one measurement of the device array d_x on the
// context's stream, a measurement like any other, with the three kernels'
// own times from HIP events (ms: k_clear_pack, k_clear, k_clear_total).
// Synchronous; declared where it is used, like the lqro_debug_* hooks.
int lqro_debug_clearance_times(lqro_ctx* c, const double* d_x, float* ms3) {
  if (!c || !d_x || !ms3 || !clear_radii_ok(c)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  if (int rc = clear_reserve(c)) return rc;
  hipEvent_t ev[4] = {};
  int rc = LQRO_OK;
  for (int k = 0; k < 4 && rc == LQRO_OK; ++k)
    if (hipEventCreate(&ev[k]) != hipSuccess) rc = LQRO_E_HIP;
  if (rc == LQRO_OK) rc = enqueue_clear(c, d_x, c->d_clrows, c->stream, ev);
  if (rc == LQRO_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = LQRO_E_HIP;
  for (int k = 0; k < 3 && rc == LQRO_OK; ++k)
    if (hipEventElapsedTime(&ms3[k], ev[k], ev[k + 1]) != hipSuccess) rc = LQRO_E_HIP;
  for (int k = 0; k < 4; ++k)
    if (ev[k]) (void)hipEventDestroy(ev[k]);
  return rc;
}

int lqro_get_monitor(lqro_ctx* c, lqro_clearance_total* last, lqro_clearance_total* since_reset, int32_t reset) {
  if (!c) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;   // (pending: the half-step's measurement is not ordered yet)
  lqro_clearance_total t[2] = {kClearNone, kClearNone};
  if (c->d_cltot) HIPCHK(hipMemcpy(t, c->d_cltot, sizeof t, hipMemcpyDeviceToHost));
  if (last) *last = t[0];
  if (since_reset) *since_reset = t[1];
  if (reset && c->d_cltot) HIPCHK(hipMemcpy(c->d_cltot + 1, &kClearNone, sizeof kClearNone, hipMemcpyHostToDevice));
  return LQRO_OK;
}

int lqro_get_monitor_rows(lqro_ctx* c, lqro_clearance_row* rows, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !rows)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  *n_out = 0;
  if (!c->cl_last) return LQRO_OK;
  if (cap < c->nrows) return LQRO_E_ARG;
  HIPCHK(hipMemcpy(rows, c->cl_last, sizeof(lqro_clearance_row) * (size_t)c->nrows, hipMemcpyDeviceToHost));
  *n_out = c->nrows;
  return LQRO_OK;
}

int lqro_get_monitor_pairs(lqro_ctx* c, int64_t* pairs, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !pairs)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  *n_out = 0;
  if (!c->cl_last) return LQRO_OK;
  std::vector<lqro_clearance_row> h((size_t)c->nrows);
  HIPCHK(hipMemcpy(h.data(), c->cl_last, sizeof(lqro_clearance_row) * h.size(), hipMemcpyDeviceToHost));
  int64_t n = 0;
  for (int r = 0; r < c->nrows && n < cap; ++r)
    for (int q = 0; q < 6 && h[r].hit[q] >= 0 && n < cap; ++q, ++n) {
      pairs[2 * n] = c->rb + (int64_t)r * c->rs;
      pairs[2 * n + 1] = h[r].hit[q];
    }
  *n_out = n;
  return LQRO_OK;
}

// ---- horizon conflict prediction ------------------------------------------
static const lqro_predict_total kPredNone = {__builtin_huge_val(), __builtin_huge_val(), -1, -1, -1, -1, -1, -1,
                                             -1, -1, -1, 0, 0, 0, 0};

// the measurement's buffers, once; the caller has waited for the last step
static int pred_reserve(lqro_ctx* c) {
  if (c->d_prtot) return LQRO_OK;
  const size_t N = c->cfg.n_agents, H = c->cfg.horizon;
  double *path = nullptr, *pv = nullptr;
  lqro_predict_row* rows = nullptr;
  lqro_predict_total* tot = nullptr;
  int rc = LQRO_OK;
  if (c->mem.get(path, 3 * H * (N + c->nobs)) || c->mem.get(pv, 3 * N) || c->mem.get(rows, (size_t)c->nrows) ||
      c->mem.get(tot, 2))
    rc = LQRO_E_NOMEM;
  const lqro_predict_total t[2] = {kPredNone, kPredNone};
  if (!rc && hipMemcpy(tot, t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) rc = LQRO_E_HIP;
  if (rc) {
    c->mem.release(path); c->mem.release(pv); c->mem.release(rows); c->mem.release(tot);
    return rc;
  }
  c->d_ppath = path; c->d_pv = pv; c->d_prrows = rows; c->d_prtot = tot;
  return LQRO_OK;
}

// the C G_k buffer for the gains as they are set; the caller has waited for the last step
static int pred_reserve_cg(lqro_ctx* c) {
  const int sets = c->per_agent ? c->cfg.n_agents : 1;
  if (c->d_pcg && c->pcg_sets == sets) return LQRO_OK;
  double* cg = nullptr;
  if (c->mem.get(cg, (size_t)sets * c->cfg.horizon * 9)) return LQRO_E_NOMEM;
  c->mem.release(c->d_pcg);
  c->d_pcg = cg; c->pcg_sets = sets; c->pcg_stale = 1;
  return LQRO_OK;
}

// One prediction on s: from (d_x, d_v), or over the given paths (d_given),
// the own rows against every column, into `rows`; the totals folded.  The
// caller has ordered s behind the last step; the buffers exist.
static int enqueue_predict(lqro_ctx* c, const double* d_x, const double* d_v, const double* d_given,
                           lqro_predict_row* rows, hipStream_t s, hipEvent_t* ev = nullptr) {
  const lqro_config& g = c->cfg;
  if (c->measured) HIPCHK(hipStreamWaitEvent(s, c->cev, 0));   // (the last measurement may be on another stream)
  PredArgs P{};
  P.n_agents = g.n_agents; P.nobs = c->nobs; P.X = g.x_dim; P.U = g.u_dim; P.H = g.horizon;
  P.nrows = c->nrows; P.row_begin = c->rb; P.row_stride = c->rs;
  P.nsets = c->per_agent ? g.n_agents : 1;
  P.nc = g.n_agents + c->nobs;
  P.ncols = d_given ? P.nc : g.n_agents;
  P.A = c->d_A; P.B = c->d_B; P.L = c->d_L; P.E = c->d_E; P.NCF = c->d_NCF; P.cg = c->d_pcg;
  P.x = d_x; P.v = d_v; P.obs = c->d_obs; P.ow = c->d_clow;
  const double a = g.xy_radius + g.xy_radius, b = g.z_radius + g.z_radius;   // as enqueue_clear
  P.wxy = 1.0 / (a * a); P.wz = 1.0 / (b * b);
  P.given = d_given; P.path = c->d_ppath;
  P.rows = rows; P.tot = c->d_prtot;
  P.active = c->d_actsrc;   // (the caller's bytes, as k_clear reads them)
  if (!d_given && c->pcg_stale) {
    LAUNCH(launch_predict_cg(s, P));
    c->pcg_stale = 0;
  }
  LAUNCH(launch_predict(s, P, ev));
  HIPCHK(hipEventRecord(c->cev, s));
  c->measured = 1;
  c->pr_last = rows;
  c->pr_kind = d_given ? 2 : 1;
  return LQRO_OK;
}

static int predict_device(lqro_ctx* c, const double* d_x, const double* d_v, const double* d_given,
                          lqro_predict_row* d_rows, void* stream) {
  if (c->pending) return LQRO_E_STATE;
  if (!d_given && !c->have_gains) return LQRO_E_STATE;
  HIPCHK(hipSetDevice(c->cfg.device));
  const int sets = c->per_agent ? c->cfg.n_agents : 1;
  if (!c->d_prtot || (!d_given && (!c->d_pcg || c->pcg_sets != sets))) {
    // the first call that needs the buffers: after the last step; later calls never wait
    HIPCHK(wait_last_step(c));
    if (int rc = pred_reserve(c)) return rc;
    if (!d_given)
      if (int rc = pred_reserve_cg(c)) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  if (c->stepped) HIPCHK(hipStreamWaitEvent(s, c->ev[3], 0));   // behind the context's last step
  return enqueue_predict(c, d_x, d_v, d_given, d_rows ? d_rows : c->d_prrows, s);
}

int lqro_predict_device(lqro_ctx* c, const double* d_x, const double* d_v, lqro_predict_row* d_rows, void* stream) {
  if (!c || !d_x || !d_v || !clear_radii_ok(c)) return LQRO_E_ARG;
  return predict_device(c, d_x, d_v, nullptr, d_rows, stream);
}

int lqro_predict_paths_device(lqro_ctx* c, const double* d_paths, lqro_predict_row* d_rows, void* stream) {
  if (!c || !d_paths || !clear_radii_ok(c)) return LQRO_E_ARG;
  return predict_device(c, nullptr, nullptr, d_paths, d_rows, stream);
}

// the host calls' tail: the rows and this measurement's total out, then the wait
static int predict_finish(lqro_ctx* c, lqro_predict_row* rows, lqro_predict_total* total) {
  if (rows)
    HIPCHK(hipMemcpyAsync(rows, c->d_prrows, sizeof(lqro_predict_row) * (size_t)c->nrows, hipMemcpyDeviceToHost,
                          c->stream));
  if (total) HIPCHK(hipMemcpyAsync(total, c->d_prtot, sizeof *total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return LQRO_OK;
}

int lqro_predict(lqro_ctx* c, const double* x, const double* v, lqro_predict_row* rows, lqro_predict_total* total) {
  if (!c || !x || !v || !clear_radii_ok(c)) return LQRO_E_ARG;
  if (c->pending || !c->have_gains) return LQRO_E_STATE;
  if (int rc = ctx_enter(c, true)) return rc;
  if (int rc = pred_reserve(c)) return rc;
  if (int rc = pred_reserve_cg(c)) return rc;
  const lqro_config& g = c->cfg;
  HIPCHK(hipMemcpyAsync(c->d_x, x, sizeof(double) * (size_t)g.n_agents * g.x_dim, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_pv, v, sizeof(double) * (size_t)g.n_agents * 3, hipMemcpyHostToDevice, c->stream));
  if (int rc = enqueue_predict(c, c->d_x, c->d_pv, nullptr, c->d_prrows, c->stream)) return rc;
  return predict_finish(c, rows, total);
}

int lqro_predict_paths(lqro_ctx* c, const double* paths, lqro_predict_row* rows, lqro_predict_total* total) {
  if (!c || !paths || !clear_radii_ok(c)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  if (int rc = pred_reserve(c)) return rc;
  const lqro_config& g = c->cfg;
  const size_t n = 3 * (size_t)g.horizon * ((size_t)g.n_agents + c->nobs);
  if (!c->d_pgiven && c->mem.get(c->d_pgiven, n)) return LQRO_E_NOMEM;
  HIPCHK(hipMemcpyAsync(c->d_pgiven, paths, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  if (int rc = enqueue_predict(c, nullptr, nullptr, c->d_pgiven, c->d_prrows, c->stream)) return rc;
  return predict_finish(c, rows, total);
}

// scripts/predict_bench.py: one prediction of the device arrays on the
// context's stream, a measurement like any other, with the launches' own
// times from HIP events (ms: paths, k_conf, k_conf_obs, k_conf_total).
// Synchronous; declared where it is used, like the lqro_debug_* hooks.
int lqro_debug_predict_times(lqro_ctx* c, const double* d_x, const double* d_v, float* ms4) {
  if (!c || !d_x || !d_v || !ms4 || !clear_radii_ok(c)) return LQRO_E_ARG;
  if (c->pending || !c->have_gains) return LQRO_E_STATE;
  if (int rc = ctx_enter(c, true)) return rc;
  if (int rc = pred_reserve(c)) return rc;
  if (int rc = pred_reserve_cg(c)) return rc;
  hipEvent_t ev[5] = {};
  int rc = LQRO_OK;
  for (int k = 0; k < 5 && rc == LQRO_OK; ++k)
    if (hipEventCreate(&ev[k]) != hipSuccess) rc = LQRO_E_HIP;
  if (rc == LQRO_OK) rc = enqueue_predict(c, d_x, d_v, nullptr, c->d_prrows, c->stream, ev);
  if (rc == LQRO_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = LQRO_E_HIP;
  for (int k = 0; k < 4 && rc == LQRO_OK; ++k)
    if (hipEventElapsedTime(&ms4[k], ev[k], ev[k + 1]) != hipSuccess) rc = LQRO_E_HIP;
  for (int k = 0; k < 5; ++k)
    if (ev[k]) (void)hipEventDestroy(ev[k]);
  return rc;
}

int lqro_get_prediction(lqro_ctx* c, lqro_predict_total* last, lqro_predict_total* since_reset, int32_t reset) {
  if (!c) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  lqro_predict_total t[2] = {kPredNone, kPredNone};
  if (c->d_prtot) HIPCHK(hipMemcpy(t, c->d_prtot, sizeof t, hipMemcpyDeviceToHost));
  if (last) *last = t[0];
  if (since_reset) *since_reset = t[1];
  if (reset && c->d_prtot) HIPCHK(hipMemcpy(c->d_prtot + 1, &kPredNone, sizeof kPredNone, hipMemcpyHostToDevice));
  return LQRO_OK;
}

int lqro_get_prediction_rows(lqro_ctx* c, lqro_predict_row* rows, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !rows)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  *n_out = 0;
  if (!c->pr_last) return LQRO_OK;
  if (cap < c->nrows) return LQRO_E_ARG;
  HIPCHK(hipMemcpy(rows, c->pr_last, sizeof(lqro_predict_row) * (size_t)c->nrows, hipMemcpyDeviceToHost));
  *n_out = c->nrows;
  return LQRO_OK;
}

int lqro_get_paths(lqro_ctx* c, double* out) {
  if (!c || !out) return LQRO_E_ARG;
  if (c->pending || c->pr_kind != 1) return LQRO_E_STATE;
  if (int rc = ctx_enter(c, true)) return rc;
  const size_t N = c->cfg.n_agents, H = c->cfg.horizon, nc = N + c->nobs;
  std::vector<double> h(3 * H * nc);   // [k][3][nc] -> [agent][k][3]
  HIPCHK(hipMemcpy(h.data(), c->d_ppath, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (size_t a = 0; a < N; ++a)
    for (size_t k = 0; k < H; ++k)
      for (size_t r = 0; r < 3; ++r) out[(a * H + k) * 3 + r] = h[(k * 3 + r) * nc + a];
  return LQRO_OK;
}

// ---- LP audit --------------------------------------------------------------
int lqro_set_lp_audit(lqro_ctx* c, int32_t on, float tol) {
  if (!c || (on != 0 && on != 1) || !(tol >= 0.0f) || !std::isfinite(tol)) return LQRO_E_ARG;
  if (c->pending) return LQRO_E_STATE;   // the pending half-step's tail audits, or does not, as it was set
  if (int rc = ctx_enter(c, false)) return rc;
  if (on && !c->d_autot) {   // the buffers, once: after the last step, never in a step
    lqro_lp_row* rows = nullptr;
    lqro_lp_total* tot = nullptr;
    if (c->mem.get(rows, (size_t)c->nrows) || c->mem.get(tot, 2)) {
      c->mem.release(rows);
      return LQRO_E_NOMEM;
    }
    const lqro_lp_total t[2] = {lp_total_none(), lp_total_none()};
    if (hipMemcpy(tot, t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) {
      c->mem.release(rows); c->mem.release(tot);
      return LQRO_E_HIP;
    }
    c->d_aurows = rows; c->d_autot = tot;
  }
  c->lp_audit = on;
  if (on) c->audit_tol = tol;
  return LQRO_OK;
}

int lqro_get_lp_audit(lqro_ctx* c, lqro_lp_total* last, lqro_lp_total* since_reset, int32_t reset) {
  if (!c) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;   // (pending: the half-step's audit comes with its _end)
  lqro_lp_total t[2] = {lp_total_none(), lp_total_none()};
  if (c->d_autot) HIPCHK(hipMemcpy(t, c->d_autot, sizeof t, hipMemcpyDeviceToHost));
  if (last) *last = t[0];
  if (since_reset) *since_reset = t[1];
  if (reset && c->d_autot) {
    const lqro_lp_total none = lp_total_none();
    HIPCHK(hipMemcpy(c->d_autot + 1, &none, sizeof none, hipMemcpyHostToDevice));
  }
  return LQRO_OK;
}

int lqro_get_lp_audit_rows(lqro_ctx* c, lqro_lp_row* rows, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !rows)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  *n_out = 0;
  if (!c->audited) return LQRO_OK;
  if (cap < c->nrows) return LQRO_E_ARG;
  HIPCHK(hipMemcpy(rows, c->d_aurows, sizeof(lqro_lp_row) * (size_t)c->nrows, hipMemcpyDeviceToHost));
  *n_out = c->nrows;
  return LQRO_OK;
}

// scripts/lp_audit_bench.py: the last step's audit once more on the context's
// stream, an audit like any other (it folds into the totals), with the two
// kernels' own times from HIP events (ms: k_lp_audit, k_lp_audit_total).
// Synchronous; declared where it is used, like the lqro_debug_* hooks.
int lqro_debug_lp_audit_times(lqro_ctx* c, float* ms2) {
  if (!c || !ms2) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  if (!c->lp_audit || !c->audited) return LQRO_E_STATE;
  const int npr = c->nbr_k > 0 ? std::min(c->nbr_k, c->npr) : c->npr;
  hipEvent_t ev[3] = {};
  int rc = LQRO_OK;
  for (int k = 0; k < 3 && rc == LQRO_OK; ++k)
    if (hipEventCreate(&ev[k]) != hipSuccess) rc = LQRO_E_HIP;
  if (rc == LQRO_OK) {
    launch_lp_audit(c->stream, lp_args(c, npr, c->au_vgoal, c->au_newv), audit_args(c), ev);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = LQRO_E_HIP;
  }
  for (int k = 0; k < 2 && rc == LQRO_OK; ++k)
    if (hipEventElapsedTime(&ms2[k], ev[k], ev[k + 1]) != hipSuccess) rc = LQRO_E_HIP;
  for (int k = 0; k < 3; ++k)
    if (ev[k]) (void)hipEventDestroy(ev[k]);
  return rc;
}

int lqro_set_carry_normal(lqro_ctx* c, const double* n3) {
  if (!c || !n3) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  const double v[6] = {n3[0], n3[1], n3[2], n3[0], n3[1], n3[2]};
  HIPCHK(hipMemcpy(c->d_carry, v, sizeof v, hipMemcpyHostToDevice));
  return LQRO_OK;
}

int lqro_get_carry_normal(lqro_ctx* c, double* n3) {
  if (!c || !n3) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  HIPCHK(hipMemcpy(n3, c->d_carry + 3, sizeof(double) * 3, hipMemcpyDeviceToHost));
  return LQRO_OK;
}

int lqro_get_records(lqro_ctx* c, lqro_pair_record* out, int64_t cap, int64_t* n_out) {
  if (!c || !out) return LQRO_E_ARG;
  if (!c->d_recs || c->pending) return LQRO_E_STATE;
  const int64_t n = (int64_t)c->nrows * (c->nbr_k > 0 ? std::min(c->nbr_k, c->npr) : c->npr);
  if (cap < n) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, false)) return rc;
  HIPCHK(hipMemcpy(out, c->d_recs, sizeof(lqro_pair_record) * (size_t)n, hipMemcpyDeviceToHost));
  if (n_out) *n_out = n;
  return LQRO_OK;
}

int lqro_get_stats_ex(lqro_ctx* c, int64_t* st, int32_t n) {
  if (!c || !st || n < 1) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;   // (pending: the half-step's counters are not final)
  unsigned long long h[LQRO_ST_FAILS];
  HIPCHK(hipMemcpy(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost));
  // (with culling k_nbr counted the kept pairs, under a mask k_active the slots visited)
  if (c->nbr_k <= 0 && !c->act_step) h[LQRO_ST_PAIRS] = (unsigned long long)c->nrows * c->npr;
  // [0..10] the device words; [11] LQRO_REC_QHMERGE_WIN pairs (device word
  // LQRO_ST_MWIN; word 11 counts the failures lqro_get_hull_failures names)
  for (int k = 0; k < n; ++k)
    st[k] = k < LQRO_ST_NFAIL ? (int64_t)h[k] : k == 11 ? (int64_t)h[LQRO_ST_MWIN] : 0;
  return LQRO_OK;
}

int lqro_get_hull_builds(lqro_ctx* c, lqro_hull_build* out, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !out)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  *n_out = 0;
  if (!c->d_hbuild) return LQRO_OK;   // not in Qhull order: no builds
  unsigned long long h[LQRO_ST_FAILS];
  HIPCHK(hipMemcpy(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost));
  const int64_t n = (int64_t)h[LQRO_ST_NBUILD];
  *n_out = n;
  const int64_t m = std::min<int64_t>(std::min<int64_t>(n, LQRO_HBUILD_CAP), cap);
  if (m <= 0) return LQRO_OK;
  std::vector<unsigned long long> r(4 * (size_t)m);
  HIPCHK(hipMemcpy(r.data(), c->d_hbuild, sizeof(unsigned long long) * r.size(), hipMemcpyDeviceToHost));
  SlotPairs sp;
  if (int rc = sp.load(c)) return rc;
  for (int64_t k = 0; k < m; ++k) {
    const unsigned long long* w = &r[4 * (size_t)k];
    lqro_hull_build& b = out[k];
    sp.pair((long)(w[0] & 0xFFFFFFFFFFull), b.i, b.j);
    b.kernel = (int32_t)(w[0] >> 40);
    b.t_start = w[1];
    b.t_end = w[2];
    b.n_points = (int32_t)(w[3] & 0xFFFFF);
    b.insertions = (int32_t)((w[3] >> 20) & 0xFFFFF);
    b.facet_slots = (int32_t)((w[3] >> 40) & 0xFFFFF);
  }
  return LQRO_OK;
}

int lqro_get_stats(lqro_ctx* c, int64_t* st) { return lqro_get_stats_ex(c, st, 8); }

// the pairs named in the step's counters: count word `wn`, slots from word `w0`
static int named_pairs(lqro_ctx* c, int wn, int w0, int64_t* pairs, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !pairs)) return LQRO_E_ARG;
  if (int rc = ctx_enter(c, true)) return rc;
  unsigned long long h[LQRO_ST_WORDS];
  HIPCHK(hipMemcpy(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost));
  const int64_t n = (int64_t)h[wn];
  *n_out = n;
  const int64_t m = std::min<int64_t>(std::min<int64_t>(n, LQRO_ST_FAILMAX), cap);
  if (m <= 0) return LQRO_OK;
  SlotPairs sp;
  if (int rc = sp.load(c)) return rc;
  for (int64_t k = 0; k < m; ++k) sp.pair((long)h[w0 + k], pairs[2 * k], pairs[2 * k + 1]);
  return LQRO_OK;
}

int lqro_get_hull_failures(lqro_ctx* c, int64_t* pairs, int64_t cap, int64_t* n_out) {
  return named_pairs(c, LQRO_ST_NFAIL, LQRO_ST_FAILS, pairs, cap, n_out);
}

int lqro_get_qhmerge_pairs(lqro_ctx* c, int64_t* pairs, int64_t cap, int64_t* n_out) {
  return named_pairs(c, LQRO_ST_MWIN, LQRO_ST_MWINS, pairs, cap, n_out);
}

int lqro_get_timings(lqro_ctx* c, float* ms) {
  if (!c || !ms) return LQRO_E_ARG;
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipEventSynchronize(c->ev[3]));
  HIPCHK(hipEventElapsedTime(&ms[0], c->ev[0], c->ev[1]));
  HIPCHK(hipEventElapsedTime(&ms[1], c->ev[1], c->ev[2]));
  HIPCHK(hipEventElapsedTime(&ms[2], c->ev[2], c->ev[3]));
  HIPCHK(hipEventElapsedTime(&ms[3], c->ev[0], c->ev[3]));
  return LQRO_OK;
}

}  // extern "C"
