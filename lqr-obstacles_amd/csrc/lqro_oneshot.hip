// lqro_oneshot.hip — the entry points of include/lqro.h that take no context:
// version and status text, the default configuration, gain synthesis, the
// agents' dynamics step and the stand-alone LP.  Their device buffers live in
// a DevPool on the stack (lqro_devmem.hpp), so every return frees them.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lqro_ctx.hpp"
#include "lqro_synth.hpp"
#include "lqro_dyn.hpp"
#include "lqro_kern.hpp"

using namespace lqro;

extern "C" {

int lqro_version(void) { return 5; }

const char* lqro_status_string(int s) {
  switch (s) {
    case LQRO_OK: return "ok";
    case LQRO_E_ARG: return "bad argument";
    case LQRO_E_HIP: return "HIP runtime error";
    case LQRO_E_NOMEM: return "out of memory";
    case LQRO_E_STATE: return "call order violated";
    case LQRO_E_SINGULAR: return "singular C*G_k";
    case LQRO_E_NODEVICE: return "no gfx950 device";
    case LQRO_E_OVERFLOW: return "work queue overflow";
    case LQRO_E_HULL: return "an inside-hull pair's hull could not be built (degenerate input or capacity; lqro_get_hull_failures)";
    case LQRO_E_QHMERGE:
      return "an inside-hull pair's winning facet may be one qconvex's pre-merge joins: its half-plane is not pinned "
             "to the reference (LQRO_REC_QHMERGE_WIN; lqro_get_qhmerge_pairs)";
  }
  return "unknown";
}

void lqro_config_default(lqro_config* c, int32_t n, int32_t h, int32_t np) {
  c->n_agents = n;
  c->x_dim = 16;
  c->u_dim = 4;
  c->horizon = h;
  c->n_points = np;
  c->min_reach = 4;
  c->xy_radius = 0.26;
  c->z_radius = 0.75;
  c->vmax_reach = 30.0;
  c->vmax_lp = 100.0;
  c->row_begin = 0;
  c->row_end = 0;
  c->row_stride = 0;
  c->device = 0;
  c->flags = LQRO_FLAG_QHULL_ORDER;   // the reference's own inside-hull rule (drop-in default)
}

// ---------------------------------------------------------------------------
// Gain synthesis (controlMatrices, LQRO:520-582): host for one agent type,
// device for heterogeneous swarms (one agent per lane; lqro_synth.hpp)
// ---------------------------------------------------------------------------
int lqro_synthesize_gains(const lqro_model* md, double* Ao, double* Bo, double* co, double* Lo,
                          double* Eo, double* Lho, double* Eho) {
  if (!md) return LQRO_E_ARG;
  synth::gains(md, Ao, Bo, co, Lo, Eo, Lho, Eho);
  return LQRO_OK;
}

int lqro_synthesize_gains_x(const lqro_model* md, int32_t x_dim, double* Ao, double* Bo, double* co,
                            double* Lo, double* Eo, double* lo, double* Lho, double* Eho) {
  if (!md) return LQRO_E_ARG;
  if (x_dim == 16) synth::gains_x<16>(md, Ao, Bo, co, Lo, Eo, Lho, Eho, lo);
  else if (x_dim == 12) synth::gains_x<12>(md, Ao, Bo, co, Lo, Eo, Lho, Eho, lo);
  else return LQRO_E_ARG;
  return LQRO_OK;
}

int lqro_synthesize_gains_batch_x(const lqro_model* models, int32_t n, int32_t x_dim, double* A, double* B,
                                  double* c, double* L, double* E, double* l, double* Lh, double* Eh,
                                  int32_t device) {
  if (!models || n <= 0 || (x_dim != 16 && x_dim != 12)) return LQRO_E_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return LQRO_E_NODEVICE;
  if (hipSetDevice(device) != hipSuccess) return LQRO_E_HIP;
  // per-agent output block, in doubles: A X*X, B X*4, c X, L 4*X, E 12, l 4, Lh 3*X, Eh 9
  const int X = x_dim, sz[8] = {X * X, X * 4, X, 4 * X, 12, 4, 3 * X, 9}, stride = X * X + 12 * X + 25;
  DevPool mem;
  lqro_model* d_m = nullptr;
  double* d_out = nullptr;
  if (mem.get(d_m, (size_t)n) || mem.get(d_out, stride * (size_t)n)) return LQRO_E_NOMEM;
  if (hipMemcpy(d_m, models, sizeof(lqro_model) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return LQRO_E_HIP;
  const char* lane_env = getenv("LQRO_SYNTH_LANE");
  launch_synth(x_dim, lane_env && atoi(lane_env) == 1, d_m, (int)n, d_out);
  std::vector<double> h((size_t)stride * n);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(h.data(), d_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return LQRO_E_HIP;
  double* outs[8] = {A, B, c, L, E, l, Lh, Eh};
  int off = 0;
  for (int k = 0; k < 8; ++k) {
    if (outs[k])
      for (int a = 0; a < n; ++a)
        memcpy(outs[k] + (size_t)a * sz[k], h.data() + (size_t)a * stride + off, sizeof(double) * sz[k]);
    off += sz[k];
  }
  return LQRO_OK;
}

int lqro_synthesize_gains_batch(const lqro_model* models, int32_t n, double* A, double* B, double* c,
                                double* L, double* E, double* Lh, double* Eh, int32_t device) {
  return lqro_synthesize_gains_batch_x(models, n, 16, A, B, c, L, E, nullptr, Lh, Eh, device);
}

static bool agents_complete(const lqro_agents* a) {
  return a && a->x && a->rot && a->x_true && a->rot_true && a->P && a->vgoal && a->u_goal && a->p_goal &&
         a->L && a->E && a->l && a->Lh && a->Eh && a->M && a->N && a->normals;
}

int lqro_dynamics_step_device(const lqro_model* models, int32_t n_models, int32_t n, int32_t per_agent_gains,
                              const lqro_agents* agents, void* stream) {
  if (!models || n <= 0 || (n_models != 1 && n_models != n) || !agents_complete(agents)) return LQRO_E_ARG;
  const char* lane = getenv("LQRO_DYN_LANE");
  launch_dyn(lane && atoi(lane) == 1, models, (int)n_models, (int)n, (int)(per_agent_gains != 0), *agents,
             (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? LQRO_OK : LQRO_E_HIP;
}

int lqro_dynamics_step(const lqro_model* models, int32_t n_models, int32_t n, int32_t per_agent_gains,
                       const lqro_agents* agents, int32_t device) {
  if (!models || n <= 0 || (n_models != 1 && n_models != n) || !agents_complete(agents)) return LQRO_E_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return LQRO_E_NODEVICE;
  if (hipSetDevice(device) != hipSuccess) return LQRO_E_HIP;
  const size_t G = per_agent_gains ? (size_t)n : 1, N = (size_t)n;
  using namespace dyn;
  // (host source, element count, written back)
  struct Buf { const double* h; double* out; size_t cnt; double* d; };
  Buf b[17] = {
      {agents->x, agents->x, N * kX, nullptr},            {agents->rot, agents->rot, N * 9, nullptr},
      {agents->x_true, agents->x_true, N * kX, nullptr},  {agents->rot_true, agents->rot_true, N * 9, nullptr},
      {agents->P, agents->P, N * kX * kX, nullptr},       {agents->vgoal, agents->vgoal, N * 3, nullptr},
      {nullptr, agents->u, agents->u ? N * kU : 0, nullptr},
      {agents->u_goal, nullptr, N * kU, nullptr},         {agents->p_goal, nullptr, N * 3, nullptr},
      {agents->L, nullptr, G * kU * kX, nullptr},         {agents->E, nullptr, G * kU * kV, nullptr},
      {agents->l, nullptr, G * kU, nullptr},              {agents->Lh, nullptr, G * kV * kX, nullptr},
      {agents->Eh, nullptr, G * kV * kV, nullptr},        {agents->M, nullptr, (size_t)kX * kX, nullptr},
      {agents->N, nullptr, (size_t)kZ * kZ, nullptr},     {agents->normals, nullptr, N * kNormals, nullptr}};
  DevPool mem;
  lqro_model* d_m = nullptr;
  float* d_kf = nullptr;
  if (mem.get(d_m, (size_t)n_models)) return LQRO_E_NOMEM;
  if (agents->keyframes && mem.get(d_kf, 8 * N)) return LQRO_E_NOMEM;
  for (auto& q : b)
    if (q.cnt && mem.get(q.d, q.cnt)) return LQRO_E_NOMEM;   // (no u: its buffer stays null)
  if (hipMemcpy(d_m, models, sizeof(lqro_model) * (size_t)n_models, hipMemcpyHostToDevice) != hipSuccess)
    return LQRO_E_HIP;
  for (auto& q : b)
    if (q.h && hipMemcpy(q.d, q.h, sizeof(double) * q.cnt, hipMemcpyHostToDevice) != hipSuccess) return LQRO_E_HIP;
  lqro_agents d;
  d.x = b[0].d; d.rot = b[1].d; d.x_true = b[2].d; d.rot_true = b[3].d; d.P = b[4].d; d.vgoal = b[5].d;
  d.u = b[6].d; d.u_goal = b[7].d; d.p_goal = b[8].d; d.L = b[9].d; d.E = b[10].d; d.l = b[11].d;
  d.Lh = b[12].d; d.Eh = b[13].d; d.M = b[14].d; d.N = b[15].d; d.normals = b[16].d;
  d.keyframes = d_kf; d.time = agents->time;
  if (int rc = lqro_dynamics_step_device(d_m, n_models, n, per_agent_gains, &d, nullptr)) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return LQRO_E_HIP;
  for (auto& q : b)
    if (q.out && hipMemcpy(q.out, q.d, sizeof(double) * q.cnt, hipMemcpyDeviceToHost) != hipSuccess)
      return LQRO_E_HIP;
  if (d_kf && hipMemcpy(agents->keyframes, d_kf, sizeof(float) * 8 * N, hipMemcpyDeviceToHost) != hipSuccess)
    return LQRO_E_HIP;
  return LQRO_OK;
}

// The stand-alone LP's and audit's slot layout: agent r's planes as k_pair's
// 32-byte slots ([6] = 1), every row at the pitch of the longest list (one
// slot at least).  LQRO_E_ARG for a list of negative length.
static int plane_slots(const float* planes, const int64_t* offsets, int n_agents, int64_t& mmax, std::vector<float>& h) {
  mmax = 1;
  for (int r = 0; r < n_agents; ++r) {
    const int64_t m = offsets[r + 1] - offsets[r];
    if (m < 0) return LQRO_E_ARG;
    if (m > mmax) mmax = m;
  }
  h.assign((size_t)n_agents * (size_t)mmax * 8, 0.0f);
  for (int r = 0; r < n_agents; ++r)
    for (int64_t k = offsets[r]; k < offsets[r + 1]; ++k) {
      float* d = &h[((size_t)r * mmax + (size_t)(k - offsets[r])) * 8];
      for (int q = 0; q < 6; ++q) d[q] = planes[6 * k + q];
      int one = 1;
      memcpy(&d[6], &one, 4);
    }
  return LQRO_OK;
}

int lqro_calculate_new_v(const float* planes, const int64_t* offsets, int32_t n_agents,
                         const double* vgoal, double vmax_lp, double* newv, int32_t device) {
  return lqro_calculate_new_v_hard(planes, offsets, nullptr, n_agents, vgoal, vmax_lp, newv, device);
}

int lqro_calculate_new_v_hard(const float* planes, const int64_t* offsets, const int32_t* n_hard,
                              int32_t n_agents, const double* vgoal, double vmax_lp, double* newv,
                              int32_t device) {
  if (!planes || !offsets || !vgoal || !newv || n_agents <= 0) return LQRO_E_ARG;
  if (n_hard)
    for (int r = 0; r < n_agents; ++r)
      if (n_hard[r] < 0) return LQRO_E_ARG;
  HIPCHK(hipSetDevice(device));
  int64_t mmax;
  std::vector<float> h;
  if (int rc = plane_slots(planes, offsets, n_agents, mmax, h)) return rc;
  const size_t slots = (size_t)n_agents * (size_t)mmax;
  DevPool mem;
  float *d_slots = nullptr, *d_compact = nullptr, *d_proj = nullptr;
  double *d_vg = nullptr, *d_nv = nullptr;
  int *d_l4 = nullptr, *d_l4c = nullptr, *d_nh = nullptr;
  if (mem.get(d_slots, 8 * slots) || mem.get(d_compact, 8 * slots) || mem.get(d_proj, 8 * slots) ||
      mem.get(d_vg, 3 * (size_t)n_agents) || mem.get(d_nv, 3 * (size_t)n_agents) ||
      mem.get(d_l4, 8 * (size_t)n_agents) || mem.get(d_l4c, 2, 0) || (n_hard && mem.get(d_nh, (size_t)n_agents)))
    return LQRO_E_NOMEM;
  if (n_hard && hipMemcpy(d_nh, n_hard, sizeof(int) * (size_t)n_agents, hipMemcpyHostToDevice) != hipSuccess)
    return LQRO_E_HIP;
  if (hipMemcpy(d_slots, h.data(), sizeof(float) * 8 * slots, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_vg, vgoal, sizeof(double) * 3 * n_agents, hipMemcpyHostToDevice) != hipSuccess)
    return LQRO_E_HIP;
  LpArgs La{};
  La.npr = (int)mmax; La.cap = (int)mmax; La.nrows = n_agents; La.row_begin = 0; La.row_stride = 1; La.vmax = vmax_lp;
  La.slots = d_slots; La.compact = d_compact; La.proj = d_proj; La.vgoal = d_vg; La.newv = d_nv; La.prof = nullptr;
  La.lp4_list = d_l4; La.lp4_count = d_l4c; La.lp4_next = d_l4c + 1;
  La.obs_first = -1; La.nhard_rows = d_nh;   // (the kernel clamps to the row's plane count)
  if (launch_lp(La, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(newv, d_nv, sizeof(double) * 3 * n_agents, hipMemcpyDeviceToHost) != hipSuccess)
    return LQRO_E_HIP;
  return LQRO_OK;
}

// lqro_calculate_new_v_hard's twin: the same slot layout and n_hard clamping
// (in the kernel), the audit's two kernels in place of the LP's
int lqro_audit_new_v(const float* planes, const int64_t* offsets, const int32_t* n_hard, int32_t n_agents,
                     const double* vgoal, const double* newv, float tol, lqro_lp_row* rows, lqro_lp_total* total,
                     int32_t device) {
  if (!planes || !offsets || !vgoal || !newv || n_agents <= 0 || !(tol >= 0.0f) || !std::isfinite(tol))
    return LQRO_E_ARG;
  if (n_hard)
    for (int r = 0; r < n_agents; ++r)
      if (n_hard[r] < 0) return LQRO_E_ARG;
  int64_t mmax;
  std::vector<float> h;
  if (int rc = plane_slots(planes, offsets, n_agents, mmax, h)) return rc;
  const size_t slots = (size_t)n_agents * (size_t)mmax;
  HIPCHK(hipSetDevice(device));
  DevPool mem;
  float* d_slots = nullptr;
  double *d_vg = nullptr, *d_nv = nullptr;
  int* d_nh = nullptr;
  lqro_lp_row* d_rows = nullptr;
  lqro_lp_total* d_tot = nullptr;
  if (mem.get(d_slots, 8 * slots) || mem.get(d_vg, 3 * (size_t)n_agents) || mem.get(d_nv, 3 * (size_t)n_agents) ||
      mem.get(d_rows, (size_t)n_agents) || mem.get(d_tot, 2) || (n_hard && mem.get(d_nh, (size_t)n_agents)))
    return LQRO_E_NOMEM;
  const lqro_lp_total none[2] = {lp_total_none(), lp_total_none()};
  if ((n_hard && hipMemcpy(d_nh, n_hard, sizeof(int) * (size_t)n_agents, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(d_slots, h.data(), sizeof(float) * 8 * slots, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_vg, vgoal, sizeof(double) * 3 * n_agents, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_nv, newv, sizeof(double) * 3 * n_agents, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_tot, none, sizeof none, hipMemcpyHostToDevice) != hipSuccess)
    return LQRO_E_HIP;
  LpArgs La{};
  La.npr = (int)mmax; La.cap = (int)mmax; La.nrows = n_agents; La.row_begin = 0; La.row_stride = 1;
  La.slots = d_slots; La.vgoal = d_vg; La.newv = d_nv;
  La.obs_first = -1; La.nhard_rows = d_nh;
  LpAuditArgs B{};
  B.tol = tol; B.plain = 1; B.rows = d_rows; B.tot = d_tot;
  launch_lp_audit(0, La, B);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      (rows && hipMemcpy(rows, d_rows, sizeof(lqro_lp_row) * (size_t)n_agents, hipMemcpyDeviceToHost) != hipSuccess) ||
      (total && hipMemcpy(total, d_tot, sizeof *total, hipMemcpyDeviceToHost) != hipSuccess))
    return LQRO_E_HIP;
  return LQRO_OK;
}

}  // extern "C"
