// lqro_ctx.hpp — the context behind lqro.h's lqro_ctx* and what the files
// that take one share (lqro_runtime.hip, lqro_debug.hip): the status macro,
// the way into an entry point, the decoding of a pair slot.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/lqro.h"
#include "lqro_device.hpp"
#include "lqro_devmem.hpp"
#include "lqro_plan.hpp"
#ifndef LQRO_RUNTIME_TU   // lqro_pair.hpp's non-template kernels: in lqro_runtime.hip's object alone
#define LQRO_PAIR_TU 1
#endif
#include "lqro_pair_launch.hpp"
#include "lqro_hull.hpp"

// (value-initialised by lqro_create: all zero; hidden: its C++ members are no part of the ABI)
struct __attribute__((visibility("hidden"))) lqro_ctx {
  lqro_config cfg;
  double *d_R, *d_TF, umax;
  unsigned long long* d_shash;
  int rb, re, rs, nrows, npr;   // rows rb, rb + rs, ... < re; npr: slots a row (n_agents - 1 + nobs)
  int have_gains, per_agent;
  hipStream_t stream;
  hipEvent_t ev[5];
  hipStream_t side;          // k_hull workers running beside k_pair
  hipEvent_t xev[2];         // cross-stream ordering (no timing)
  double *d_T, *d_NCF, *d_S, *d_x, *d_vgoal, *d_newv;
  double *d_A, *d_B, *d_L, *d_E;
  float *d_planes, *d_lpscratch, *d_lpcompact;
  lqro_pair_record* d_recs;
  int *d_hq, *d_hcount, *d_err, *d_rq;   // d_hcount: LQRO_HC_* (lqro_device.hpp)
  lqro::HullMemBig* d_hbig;
  lqro::HullWide* d_hwide;
  int* d_hbag;
  int* d_lp4;                // k_lp_lds -> k_lp4 row list (8 ints per row)
  int* d_hotlist;            // k_prio: likely inside-hull pairs (slots), computed first
  int* d_prevq;              // Qhull order: the last step's inside-hull pairs (k_prio_save), hot_cap
  int* d_hot2;               // the split hot launch's counters: LQRO_H2_* (lqro_device.hpp)
  lqro::StepKnobs knobs;           // the environment knobs (lqro_plan.hpp)
  unsigned char* d_hotmark;  // per slot: in the hot list
  int* d_nbrlist;            // culling on: per row K neighbour slots (lqro_set_neighbors)
  double nbr_r2;
  int nbr_k, nbr_cap;         // k; rows x nbr_cap ints allocated
  int hot_cap;
  int* d_lq;                 // k_lhull -> k_hull queue
  // what each step leaves for the schedule of the step two after it (pinned,
  // copied at the end of the step): step t writes slot t & 1
  lqro::StepFeedback* h_feedback;
  hipEvent_t iev[2];              // recorded after the copy into slot k
  long long nstep;                // steps enqueued
  int hull_big_blocks;
  int n_cu;
  double* d_hscratch;
  int* d_hiscratch;
  float* d_hfscratch;
  unsigned long long* d_hfbest;
  int *d_hvpid, *d_hstack;
  lqro::HullPt* d_hfaces;
  int hull_blocks, hull_cap;
  unsigned long long* d_stats;
  unsigned long long* d_prof;
  int lds_bytes;
  int stepped;               // a step was enqueued (ev[3] recorded)
  int pending;               // lqro_step_device_begin ran, _end not yet
  const double* pend_x;
  const double* pend_vgoal;
  hipStream_t pend_stream;
  // LQRO_FLAG_QHULL_ORDER: k_qhull workers, per-slot normals, facet-0 slots,
  // the loop-carried normal in [0..2], out [3..5]
  int qhull_order;
  int qworkers;
  size_t qstride;
  char* d_qscratch;
  double* d_qnrm;
  int* d_qstale;
  unsigned long long* d_hbuild;   // LQRO_HBUILD_CAP x 4 words: the builds' timing records
  double* d_carry;
  // early LP: per row open work and LP claim (lqro_hull.hpp hull_row_done)
  int early_step;            // the step being enqueued runs the early LP
  int early_internal;        // ... into d_newv (lqro_step_device_begin: the caller's buffer comes with _end)
  int* d_rowpend;
  int* d_rowclaim;
  // the planes ahead of a row's pair planes (lqro_set_fence,
  // lqro_set_user_planes[_device]); lp_cap: the pitch d_lpscratch and
  // d_lpcompact are allocated for (>= npr + nfence + uplane_max)
  int nfence, fence_faces;        // faces emitted; bit 2 a + side (side 1 = upper)
  double fence_lo[3], fence_hi[3], fence_tau;
  float* d_fence;                 // nrows x nfence x 6, k_fence's output
  const float* d_uplanes;         // the caller's, or d_uown
  const int* d_ucounts;           // the caller's, d_ucown, or null
  int uplane_max;
  float* d_uown;                  // lqro_set_user_planes's copies
  int* d_ucown;
  int lp_cap;
  int hard_level;                 // lqro_set_hard_planes: LQRO_HARD_* (0: every plane soft)
  // obstacle columns (lqro_set_obstacles[_device]): nobs states behind the
  // agents' in d_cols, the array the step's kernels then take for x (k_cols
  // fills it at the head of every step)
  int nobs;
  const double* d_obs;            // nobs x X: the caller's, or d_obsown
  double* d_obsown;               // lqro_set_obstacles's copy
  double* d_cols;                 // (n_agents + nobs) x X
  int n_ocls;                     // shape classes that are not the agents' (<= LQRO_OBS_SHAPES_MAX)
  double* d_oresp;                // nobs: each column's factor for the 0.5 of LQRO:1416
  int* d_ocls;                    // nobs: 0 the agents' shape, c >= 1 class c (n_ocls > 0 only)
  double *d_So, *d_Ro;            // n_ocls x (NP x 3), then n_ocls x 4 (semi-axes, max |u_p|: pa.osc);
                                  // n_ocls x n_agents x H (the row of agent 0 with shared gains)
  int lds_attr;                   // the dynamic LDS size the k_pair instantiations are set to
  // clearance (lqro_clearance[_device], lqro_set_monitor): allocated by the
  // first call that needs them, never in a step
  int monitor;                    // lqro_set_monitor: every step measures its own columns
  int measured;                   // a measurement was enqueued (cev recorded)
  hipEvent_t cev;                 // the last measurement's end, on whichever stream it ran
  double* d_clpack;               // 5 x (n_agents + nobs): px py pz wxy wz
  double* d_clow;                 // nobs x 2: the obstacle columns' wxy, wz (lqro_set_obstacles)
  lqro_clearance_row* d_clrows;   // nrows: the context's own row buffer
  const lqro_clearance_row* cl_last;   // the last measurement's rows: d_clrows or the caller's
  lqro_clearance_total* d_cltot;  // [0] last, [1] since reset
  // horizon conflict prediction (lqro_predict[_device], lqro_predict_paths[_device]):
  // allocated by the first call that needs them, never in a step; its
  // measurements share `measured` / `cev` with the clearance calls
  double* d_pcg;                  // gains sets x H x 9: C G_k (k_pred_cg)
  int pcg_sets;                   // the sets d_pcg is allocated for
  int pcg_stale;                  // lqro_set_gains ran since d_pcg was built
  double* d_ppath;                // [H][3][n_agents + nobs]: the bodies' paths
  double* d_pv;                   // n_agents x 3: lqro_predict's copy of v
  double* d_pgiven;               // (n_agents + nobs) x H x 3: lqro_predict_paths' copy
  lqro_predict_row* d_prrows;     // nrows: the context's own row buffer
  const lqro_predict_row* pr_last;   // the last prediction's rows: d_prrows or the caller's
  lqro_predict_total* d_prtot;    // [0] last, [1] since reset
  int pr_kind;                    // the last prediction: 0 none, 1 predicted paths, 2 given paths
  // LP audit (lqro_set_lp_audit): allocated by the call that turns it on, never in a step
  int lp_audit;                   // every step audits its own rows at the end of its tail
  float audit_tol;
  int audited;                    // d_aurows holds an audit's rows
  lqro_lp_row* d_aurows;          // nrows
  lqro_lp_total* d_autot;         // [0] last, [1] since reset
  const double* au_vgoal;         // the last tail's vgoal and newV (lqro_debug_lp_audit_times)
  double* au_newv;
  // activity mask (lqro_set_active[_device]): allocated by the setter, never in a step
  const unsigned char* d_actsrc;  // n_agents bytes: the caller's, or d_actown (null: no mask)
  unsigned char* d_actown;        // lqro_set_active's copy
  unsigned char* d_act;           // k_active's 0 / 1 bytes, padded to a multiple of 4: what the step's kernels read
  int act_step;                   // the last step ran under a mask or a table (its pairs counter is k_active's)
  // interaction classes (lqro_set_interaction[_device]): allocated by the setter, never in a step
  const unsigned char* d_ixsrc;   // n_agents class bytes: the caller's, or d_ixown (null: no table)
  unsigned char* d_ixown;         // lqro_set_interaction's copy
  unsigned char* d_ix;            // an lqro::IxDev: the table, then k_active's clamped bytes: what the step's kernels read
  lqro::PairArgs pa;
  lqro::DevPool mem;              // owns every d_* buffer above that is not the caller's
};

namespace lqro {
void sphere_axes(int np, double axy, double az, double* out);   // (lqro_synth.cpp)
}

// the last step's final event was recorded on whichever stream it was
// enqueued on (the caller's for lqro_step_device): wait on that, not on
// c->stream; a context that never stepped has nothing to wait for
static inline hipError_t wait_last_step(lqro_ctx* c) {
  if (c->measured) {   // ... and the last clearance measurement, wherever it was enqueued
    const hipError_t e = hipEventSynchronize(c->cev);
    if (e != hipSuccess) return e;
  }
  if (!c->stepped) return hipStreamSynchronize(c->stream);
  return hipEventSynchronize(c->ev[3]);
}

#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "liblqro: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, \
              __LINE__);                                                                 \
      return LQRO_E_HIP;                                                                 \
    }                                                                                    \
  } while (0)

// The way into an entry point once its arguments are checked: a pending
// half-step (a _begin without its _end) is refused before any HIP call where
// the caller says so, then the context's device, then the last step's end.
// (Where argument checks follow the pending test, the entry point makes that
// test itself and passes false.)
static inline int ctx_enter(lqro_ctx* c, bool pending_is_error) {
  if (pending_is_error && c->pending) return LQRO_E_STATE;
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(wait_last_step(c));
  return LQRO_OK;
}

// The last step's slot -> ordered pair (i, j).  With culling on, a slot names
// an entry of its row's neighbour list, which load() downloads.
struct __attribute__((visibility("hidden"))) SlotPairs {
  const lqro_ctx* c;
  int npr;
  std::vector<int> nbr;
  int load(const lqro_ctx* ctx) {
    c = ctx;
    npr = c->nbr_k > 0 ? std::min(c->nbr_k, c->npr) : c->npr;
    if (c->nbr_k > 0) {
      nbr.resize((size_t)c->nrows * npr);
      HIPCHK(hipMemcpy(nbr.data(), c->d_nbrlist, sizeof(int) * nbr.size(), hipMemcpyDeviceToHost));
    }
    return LQRO_OK;
  }
  template <class I>
  void pair(long slot, I& i, I& j) const {
    const int jj = nbr.empty() ? (int)(slot % npr) : nbr[slot], row = c->rb + (int)(slot / npr) * c->rs;
    i = row;
    j = jj < row ? jj : jj + 1;
  }
};
