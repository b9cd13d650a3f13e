// lqro_kern.hpp — launch functions of the kernels compiled in their own
// objects (lqro_kern_hull.hip, lqro_kern_lp.hip, lqro_kern_synth.hip,
// lqro_kern_dyn.hip), so that liblqro.so's large kernels compile in parallel
// and a host edit recompiles none of them.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lqro.h"

// The arguments of the LP kernels (k_lp, k_lp_lds, k_lp4) and of k_fence.
// Both stay outside the namespace: they are part of the kernels' names.
struct LpArgs {
  int npr, nrows, row_begin, row_stride;
  // a row's plane list holds at most cap = npr + nfence + umax planes; npr
  // stays the number of pair slots to compact (no extras: cap == npr)
  int cap;
  double vmax;
  const float* slots;   // per row npr x 8 (flag in [6]: 1 = plane)
  float* compact;       // per row cap x 8: the row's planes in push order
  float* proj;          // per row cap x 8: linearProgram4's projected planes
  // the planes ahead of the pair planes (RVO2's obstacle-first order,
  // AGT:84-151): k_fence's, per own row nfence x 6 floats, then the user's,
  // per agent (global id) umax x 6 floats of which ucounts[i] are live
  // (null: all)
  const float* fence;
  const float* uplanes;
  const int* ucounts;
  int nfence, umax;
  const double* vgoal;
  double* newv;
  unsigned long long* prof;   // LQRO_LP_PROFILE: cycles per row
  // rows whose linearProgram3 fails go to k_lp4 (null: linearProgram4 inline)
  int* lp4_list;              // 8 ints per row: lrow, fail, m, nv.xyz (float bits), n_hard, 0
  int* lp4_count;
  int* lp4_next;
  // early LP (lqro_hull.hpp hull_row_done): mode 1 runs the rows whose
  // count reached row_target and that it claims; mode 2 (the tail) skips the
  // rows claimed earlier.  rowclaim null: every row.
  const int* rowpend;
  int* rowclaim;
  int row_target;
  int mode;
  // hard planes (lqro_set_hard_planes; linearProgram4 keeps a list's first
  // n_hard planes out of its relaxation, lqro_lp.hpp w_lp4h).  hard: the
  // level, LQRO_HARD_*: the row's fence planes (1), its live user planes too
  // (2), and at 3 its obstacle-column planes, which are then compacted ahead
  // of the agent planes.  A row's obstacle slots are [obs_first, npr),
  // obs_first = n_agents - 1; with culling (nbr: per row npr neighbour jj,
  // ascending, -1 padded) the slots whose jj >= obs_first, the suffix of its
  // live slots.  obs_first < 0 (no obstacles, or hard < 3): slot order as it is.
  // nhard_rows (lqro_calculate_new_v_hard): per row n_hard itself, clamped to
  // the row's plane count; null: from the level.
  int hard, obs_first;
  const int* nbr;
  const int* nhard_rows;
  // activity mask (lqro_set_active; k_active's byte per agent, null: none):
  // an inactive own row's LP is not run, its newV is +0.0; the audit gives it
  // the cleared record and leaves it out of the totals
  const unsigned char* active;
};

// The fence (lqro_set_fence): an axis-aligned box [lo, hi] the agents'
// ellipsoids (semi-axes m) should stay inside, as at most six half-planes per
// own row in absolute velocity space, ahead of the user and pair planes
// (RVO2 puts its obstacle lines first in the same LP, AGT:84-151).  Axis x,
// y, z, lower face then upper; a face at infinity is not emitted (`faces`).
// The bound is fp64 in the order written, rounded once.
struct FenceArgs {
  int nrows, row_begin, row_stride, X, nfence, faces;
  double lo[3], hi[3], m[3], tau;
  const double* x;
  float* out;
};

// The clearance measurement (lqro_clearance[_device], lqro_set_monitor;
// lqro_kern_clear.hip): own rows against every column, lqro.h's contract.
// pack: the columns as a structure of arrays, px py pz wxy wz, ncols each.
struct ClearArgs {
  int n_agents, nobs, X;
  int nrows, row_begin, row_stride;
  const double* x;      // n_agents x X: the agents' states
  const double* obs;    // nobs x X: the obstacles' states as the step reads them
  const double* ow;     // nobs x 2: the obstacles' wxy, wz
  double wxy, wz;       // the agent columns' weights
  double* pack;         // 5 x (n_agents + nobs)
  int faces;            // the fence: bit 2 a + side (0: no fence)
  double lo[3], hi[3], m[3];
  lqro_clearance_row* rows;     // nrows records, the own rows in row order
  lqro_clearance_total* tot;    // [0] last, [1] since reset
  // activity mask (lqro_set_active; null: none): the caller's n_agents bytes
  // as they are when the measurement runs (!= 0: takes part).  An inactive
  // agent is neither a measured row nor a column; its own row's record is the
  // cleared one, which adds nothing to the totals
  const unsigned char* active;
};

// The LP audit (lqro_set_lp_audit, lqro_audit_new_v; lqro_kern_audit.hip):
// the step's result against each own row's plane list, lqro.h's contract.  The
// list is read through the LpArgs the LP itself was launched with (newv: the
// result to audit).
struct LpAuditArgs {
  float tol;
  int faces;             // the fence: bit 2 a + side of the emitted faces, for a fence plane's id
  int plain;             // lqro_audit_new_v: every plane is LQRO_AUDIT_USER with id = k
  lqro_lp_row* rows;     // nrows records, the own rows in row order
  lqro_lp_total* tot;    // [0] last, [1] since reset
};

// The horizon conflict prediction (lqro_predict[_device],
// lqro_predict_paths[_device]; lqro_kern_predict.hip): own rows against every
// column at every slice, lqro.h's contract.  path: the bodies' paths as a
// structure of arrays [H][3][nc], nc = n_agents + nobs.
struct PredArgs {
  int n_agents, nobs, X, U, H;
  int nrows, row_begin, row_stride;
  int nsets;            // gains sets: 1, or n_agents
  int ncols;            // the columns k_conf streams: n_agents (the predicting calls: k_conf_obs takes the
                        // obstacles), n_agents + nobs (given paths)
  int nc;               // the path array's pitch, n_agents + nobs
  const double *A, *B, *L, *E;   // the gains (k_pred_cg)
  const double* NCF;    // k_tables': nsets x H x 3 x X
  double* cg;           // nsets x H x 9: C G_k
  const double* x;      // n_agents x X
  const double* v;      // n_agents x 3: the commanded velocities
  const double* obs;    // nobs x X: the obstacles' states as the step reads them
  const double* ow;     // nobs x 2: the obstacle columns' wxy, wz
  double wxy, wz;       // the agent columns' weights
  const double* given;  // null, or the caller's paths [(n_agents + nobs)][H][3]
  double* path;
  lqro_predict_row* rows;     // nrows records, the own rows in row order
  lqro_predict_total* tot;    // [0] last, [1] since reset
  const unsigned char* active;   // as ClearArgs::active
};

namespace lqro {
// k_pred_cg: the C G_k table of every gains set
void launch_predict_cg(hipStream_t s, const PredArgs& P);
// k_pred_paths or k_pred_tr, k_conf, k_conf_obs, k_conf_total: one measurement
// (ev: five timing events recorded around the four launches, scripts/predict_bench.py; else null)
void launch_predict(hipStream_t s, const PredArgs& P, hipEvent_t* ev = nullptr);
// k_conf's dynamic LDS: the tile's rows' paths
size_t predict_lds_bytes(int H);
// k_clear_pack, k_clear, k_clear_total: one measurement (ev: four timing
// events recorded around the three kernels, scripts/clearance_bench.py; else null)
void launch_clear(hipStream_t s, const ClearArgs& A, hipEvent_t* ev = nullptr);
// k_lp_audit, k_lp_audit_total: one audit (ev: three timing events recorded
// around the two kernels, scripts/lp_audit_bench.py; else null)
void launch_lp_audit(hipStream_t s, const LpArgs& La, const LpAuditArgs& B, hipEvent_t* ev = nullptr);
// a total that no audit has touched: maxima -inf, indices -1, counts 0
inline lqro_lp_total lp_total_none() {
  lqro_lp_total t{};
  t.viol_max = t.hard_viol_max = t.dv2_max = -__builtin_huge_valf();
  t.viol_i = t.viol_k = t.viol_kind = t.viol_id = -1;
  t.hard_i = t.hard_k = t.hard_kind = t.hard_id = -1;
  t.dv2_i = -1;
  return t;
}
struct HullArgs;
struct ObsSlots;   // (lqro_hull_job.hpp)
// k_tables: one workgroup per agent with gains of its own (n_gains: 1 or N)
void launch_tables(hipStream_t s, int n_gains, int X, int U, int H, const double* A, const double* B, const double* L,
                   const double* E, int per_agent, double* T, double* NCF, double* R, double* TF, double rad0,
                   double rad1, double rad2, double umax, int* err);
// k_obs_rtab: the obstacle classes' slice bounds (PairArgs::Ro: class, agent of n_agents, H) from the tables' T
// and each class's semi-axes and max |u_p| (osc), one launch over (class, agent, k)
void launch_obs_rtab(hipStream_t s, int n_cls, int n_gains, int n_agents, int H, const double* T, const double* osc,
                     double* Ro);
// k_cols: the step's columns, the agents' states then the obstacles'
void launch_cols(hipStream_t s, const double* x, size_t nx, const double* obs, size_t nobs, double* cols);
constexpr size_t kLpLdsMax = 160 * 1024;   // one CU's LDS: the longest plane list k_lp_lds holds
// the LP of every row: k_lp_lds (+ k_lp4 for the rows it lists) or, past
// kLpLdsMax, k_lp.  La.lp4_count / lp4_next must be zero (or lp4_list null).
// early (La.mode 1, no lp4_list; plan_step: La.cap fits): k_lp_lds at 32 B a
// plane whatever the length, of which it runs the rows it claims
hipError_t launch_lp(LpArgs La, hipStream_t s, bool early = false);
// k_copy_claimed: the rows the early LP ran (claim 1), from src into dst
void launch_copy_claimed(hipStream_t s, const int* rowclaim, int nrows, int row_begin, int row_stride,
                         const double* src, double* dst);
// k_fence: this step's fence planes of every own row
void launch_fence(hipStream_t s, const FenceArgs& F);
// k_hull: grid x 8 waves, topology in LDS
void launch_hull(dim3 grid, hipStream_t s, const HullArgs& A);
// k_hull_big: one inserting wave, topology in global memory
void launch_hull_big(dim3 grid, hipStream_t s, const HullArgs& A);
// k_lhull: grid x 4 waves, one inside-hull pair at a time from a local hull
// around vrel; the pairs it cannot decide go to A.lqueue (for k_hull)
void launch_lhull(dim3 grid, hipStream_t s, const HullArgs& A);
// k_qhull (LQRO_FLAG_QHULL_ORDER): grid x 1 wave, one inside-hull pair per
// wave (one wave per CU: its LDS) with Qhull's build order (lqro_qhull3.hpp); A.qscratch holds
// A.block_base + grid workers of qhull_worker_bytes(H*NP) bytes.  Pairs beyond
// its per-insertion caps go to A.rqueue for k_qhull_big (lqro_qhull.hpp),
// which with A.big_main takes the main queue instead.
void launch_qhull(dim3 grid, hipStream_t s, const HullArgs& A);
void launch_qhull_big(dim3 grid, hipStream_t s, const HullArgs& A);
size_t qhull_lds_doubles();   // k_qhull's LDS block (k_qside sweeps rows in it)
size_t qhull_worker_bytes(int hnp);
// k_stale: the facet-0 pairs' loop-carried normals, then the carry out
void launch_stale(hipStream_t s, float* planes, const double* qnrm, const int* list, const int* count, int cap,
                  const double* x, int X, int npr, int row_begin, int row_stride, double* carry,
                  lqro_pair_record* recs, long nslots, const ObsSlots& O);
void launch_rowlast(hipStream_t s, const float* planes, const double* qnrm, int npr, int nrows, int row_begin,
                    int row_stride, double* rowtab);
void launch_stale_rows(hipStream_t s, float* planes, const double* qnrm, const int* list, const int* count, int cap,
                       const double* x, int X, int npr, int row_begin, int row_stride, const double* rowtab, int N,
                       double* carry, lqro_pair_record* recs, long nslots, const ObsSlots& O);
// controlMatrices for n models into out (stride X*X + 12X + 25 doubles):
// k_synthw (one wave per agent) or, lane = true, k_synth (one agent per lane)
void launch_synth(int x_dim, bool lane, const lqro_model* d_models, int n, double* d_out);
// the agent loop LQRO:1437-1446: k_dynw or, lane = true, k_dyn
void launch_dyn(bool lane, const lqro_model* models, int n_models, int n, int per_agent, const lqro_agents& A,
                hipStream_t s);
}  // namespace lqro
