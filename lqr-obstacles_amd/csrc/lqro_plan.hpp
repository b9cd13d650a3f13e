// lqro_plan.hpp — one step's schedule as a pure host function.
//
// plan_step decides whether the step overlaps the hulls with the sweep (`hot`),
// how many CUs the side stream takes and which of the Qhull-order refinements
// (split hot launch, speculative builds, early LP, k_qside) are on, from the
// context's sizes, the environment knobs and the work measured two steps
// before.  It is plain host arithmetic: no HIP include, no device type, so it
// compiles with g++ alone and tests/test_step_plan.py pins it on a CPU
// (tests/golden/step_plan.json).  lqro_runtime.hip fills the inputs, the
// kernel headers' limits among them, and turns the plan into launches.
// Every schedule gives bit-identical results; only the step's time depends on
// what is decided here.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace lqro {

// The environment knobs, read once per context (knobs_from_env).
struct StepKnobs {
  int hot_on;                // LQRO_HOT (default 1)
  int hot_split;             // LQRO_HOT_SPLIT (default 1): the split hot launch in Qhull order
  int hot_spec;              // LQRO_HOT_SPEC (default 1): with the split, the last step's inside pairs are built speculatively from the step's start
  long hot_max_inside;       // LQRO_HOT_MAX_INSIDE (-1: 4 x the side CUs)
  double hot_t, hot_r;       // k_prio horizon (s) and radius (m): LQRO_HOT_T, LQRO_HOT_R
  int qside;                 // LQRO_QSIDE=1: k_qhull side workers sweep rows after their builds (default off)
  int qside_pct;             // LQRO_QHULL_SIDE_PCT: side CUs per 100 of the last step's inside-hull pairs (default 100)
  int qspare;                // LQRO_QHULL_SPARE: side CUs beyond the last step's inside-hull count (default 4; -1: count/16 + 4)
  int qbalance;              // LQRO_QHULL_BALANCE: the side's width from the measured work (default 1)
  int qhull_inline;          // LQRO_QHULL_INLINE_BIG: k_qhull rebuilds a capped build in place (default 1)
  int qhull_big;             // LQRO_QHULL_BIG=1: every pair in k_qhull_big (A/B runs)
  int qhull_flags;           // LQRO_QHULL_FLAGS: k_qhull's helper waves (1), emit lane state (2), queue pre-scan (4),
                             // a long emit over the waves (16), no event for a trigger without sharp new
                             // facets (32), helpers posted under the state a sharp trigger leads to (64);
                             // default 119
  int hull_big_only;         // LQRO_HULL_BIG: skip the LDS hull (A/B)
  int local_hull;            // LQRO_LOCAL_HULL (default 1): k_lhull first, k_hull for what it hands over
  int lhull_prof;            // LQRO_LHULL_PROFILE: k_lhull writes its per-job words
  int side_cus;              // CUs running k_hull beside k_pair (LQRO_SIDE_HULL_CUS)
  int lside_cus;             // side CUs with the local hull (LQRO_LOCAL_SIDE_CUS, default 3/16 of the CUs)
  int early_lp;              // LQRO_EARLY_LP (default 1): per row open work and LP claim (lqro_hull.hpp hull_row_done)
};

inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
inline long env_long(const char* name, long dflt) {
  const char* e = std::getenv(name);
  return e ? std::atol(e) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* e = std::getenv(name);
  return e ? std::atof(e) : dflt;
}

inline StepKnobs knobs_from_env(int n_cu) {
  StepKnobs k{};
  k.qhull_big = env_int("LQRO_QHULL_BIG", 0) != 0;
  // CUs running k_hull workers beside k_pair (the hot-pair hulls); default 3/8
  k.side_cus = std::max(0, std::min(n_cu / 2, env_int("LQRO_SIDE_HULL_CUS", (3 * n_cu) / 8)));
  k.hull_big_only = env_int("LQRO_HULL_BIG", 0) != 0;   // every hull job in k_hull_big (A/B runs)
  k.local_hull = env_int("LQRO_LOCAL_HULL", 1) != 0;
  k.lside_cus = std::max(0, std::min(n_cu / 2, env_int("LQRO_LOCAL_SIDE_CUS", (3 * n_cu) / 16)));
  k.hot_on = env_int("LQRO_HOT", 1) != 0;
  k.hot_t = env_double("LQRO_HOT_T", 3.0);
  k.hot_r = env_double("LQRO_HOT_R", 3.0);
  k.lhull_prof = env_int("LQRO_LHULL_PROFILE", 0) != 0;
  k.hot_max_inside = env_long("LQRO_HOT_MAX_INSIDE", -1L);
  k.early_lp = env_int("LQRO_EARLY_LP", 1) != 0;
  // Qhull order: the last step's inside-hull pairs in a hot launch of their
  // own on the side stream, so the builds start when they are found rather
  // than behind the other hot pairs' stragglers (which go to the main stream)
  k.hot_split = env_int("LQRO_HOT_SPLIT", 1) != 0;
  k.hot_spec = env_int("LQRO_HOT_SPEC", 1) != 0;
  k.qspare = env_int("LQRO_QHULL_SPARE", 4);
  k.qside_pct = std::max(1, std::min(100, env_int("LQRO_QHULL_SIDE_PCT", 100)));
  // off by default: with 3 waves a CU the side workers sweep rows at ~1/5 of a
  // 16-wave workgroup's rate, so where the sweep outlasts the builds (C4:
  // 227 vs 114 ms per step) it loses; at C3 it ties (22.0 ms either way)
  k.qside = env_int("LQRO_QSIDE", 0) != 0;
  // a build past k_qhull's caps rebuilt at once on its CU (q3_big_inline)
  // instead of in the k_qhull_big launch after the sweep
  k.qhull_inline = env_int("LQRO_QHULL_INLINE_BIG", 1) != 0;
  k.qhull_flags = env_int("LQRO_QHULL_FLAGS", 119);
  // the side's width from the measured work of the step two before (the
  // sweep's CU time, the builds' total and longest): no wider than leaves
  // the sweep no longer than the builds (LQRO_QHULL_BALANCE=0: one CU per
  // expected build, round 5's rule)
  k.qbalance = env_int("LQRO_QHULL_BALANCE", 1) != 0;
  return k;
}

// What a step leaves for the schedule of the step two after it: one pinned
// slot of 8 words, copied from the step's counters at its end (enqueue_tail).
struct StepFeedback {
  unsigned long long inside;       // inside-hull pairs; ~0: none yet
  unsigned long long sweep_work;   // LQRO_ST_SWORK, _BWORK, _BMAX (100 MHz ticks): the sweep's workgroup time
  unsigned long long build_work;   //   summed, the Qhull-order builds' time summed
  unsigned long long build_max;    //   and the longest build (one copy: the three stay adjacent)
  unsigned long long retried;      // LQRO_ST_RETRY (builds past k_qhull's caps)
  unsigned long long unused[3];
};
static_assert(sizeof(StepFeedback) == 8 * sizeof(unsigned long long), "one slot is 8 words");
constexpr StepFeedback kNoFeedback = {~0ull, 0ull, 0ull, 0ull, 0ull, {0ull, 0ull, 0ull}};

// Everything else the decision reads: the context's sizes and flags, k_pair's
// LDS layout and the limits the kernels' headers set (filled by the runtime).
struct StepShape {
  int n_cu, nrows;
  int npr;                   // pairs per row before culling (N - 1)
  int nbr_k;                 // culling on: neighbours per row (lqro_set_neighbors), else <= 0
  size_t hnp;                // horizon * n_points
  int per_agent, qhull_order;
  int phase;                 // 0 the whole step, 1 lqro_step_device_begin, 2 the tail
  bool has_newv;             // the early LP has a newV to write (the caller's, or in phase 1 the context's)
  bool newv_is_callers;      // ... and it is the caller's buffer
  int waves, lds_wave, wave_doubles;   // PairArgs: k_pair's waves, its LDS before the wave regions, one region
  size_t hull_lds_max_hnp;   // kHullLdsMaxHNP
  size_t hull_lds_doubles;   // sizeof(HullMemC) / 8
  int hull_cwaves;           // HULL_CWAVES
  size_t qhull_lds_doubles;  // qhull_lds_doubles()
  size_t lp_lds_max;         // kLpLdsMax
  int early_lp_max_npr;      // LQRO_EARLY_LP_MAX_NPR
  int row_big;               // LQRO_ROW_BIG
  int extra_planes = 0;      // fence + user planes a row's LP may get ahead of its pair planes (capacity per row)
  int n_obs = 0;             // obstacle columns behind the npr agent columns of every row (lqro_set_obstacles):
                             //   a row has npr + n_obs slots, whatever the number of rows
  int hard_obs = 0;          // lqro_set_hard_planes at LQRO_HARD_OBSTACLES with obstacles set: the row's LP takes
                             //   its obstacle slots ahead of its agent slots
};

struct StepPlan {
  int npr;                   // pairs per row after culling
  long slots;                // nrows * npr
  bool lds_ok;               // the LDS hull (k_hull) can hold the step's hulls
  int side_waves;            // k_side's waves that sweep rows
  int qside_waves;           // k_qside's
  bool hot;                  // hulls on the side stream beside the sweep
  int side;                  // the side's width (CUs) were it hot
  int nwait;                 // the side's workgroups: hot ? side : 0
  bool split, spec, qside;
  bool early, early_internal;
  int row_split;
  unsigned nblk, nside;      // the row launch's workgroups on the main and on the side stream
  int big_inline, row_lp, row_target;
};

// LDS layout of k_pair, in doubles: the block tables (T, N, S, R, TF, the
// slice hashes), one block per obstacle shape class that is not the agents'
// (lqro_set_obstacles_ex: S_c 3 NP SoA, Ro_c H, the three semi-axes and max
// |u_p|), then one region per wave.  n_cls = 0 is the layout a context is
// created with.
struct PairLayout {
  int XP, PW;
  int lds_T, lds_N, lds_S, lds_R, lds_TF, lds_H;
  int lds_cls, cls_doubles;   // class c >= 1 at lds_cls + (c - 1) * cls_doubles
  int lds_wave, wave_doubles, waves;
  int lds_bytes;
};
constexpr int kPairLdsBudget = 160 * 1024 / 8;

// False when no wave keeps a region.  max_waves: LQRO_PAIR_LB / 64.
inline bool pair_layout(int H, int NP, int X, int n_cls, PairLayout& L, int max_waves = 16) {
  const int XP = X + 1;
  int off = 0;
  L.XP = XP;
  L.PW = (NP + 63) / 64;
  L.lds_T = off; off += H * 9;
  L.lds_N = off; off += H * 3 * XP;
  L.lds_S = off; off += 3 * NP;
  L.lds_R = off; off += H;
  L.lds_TF = off; off += H;
  L.lds_H = off; off += H;
  L.lds_cls = off;
  L.cls_doubles = 3 * NP + H + 4;
  off += n_cls * L.cls_doubles;
  L.lds_wave = off;
  // tr 3H, sc H, mask H*PW (u64), cls/cnt/mixed 3H ints (mixed padded to
  // even), GJK simplex 18, statistics 5
  L.wave_doubles = 4 * H + H * L.PW + H + (H + (H & 1)) / 2 + 18 + 5;
  int waves = off <= kPairLdsBudget ? (kPairLdsBudget - off) / L.wave_doubles : 0;
  if (waves > max_waves) waves = max_waves;
  L.waves = waves;
  L.lds_bytes = (off + (waves > 0 ? waves : 0) * L.wave_doubles) * 8;
  return waves >= 1;
}

// The side's width in Qhull order from the work measured two steps before:
// with k side CUs the builds end no sooner than max(b_max, 1.15 w_build / k)
// (LPT packing of chains, 15 % margin) and the sweep's rows no sooner than
// w_sweep / (n - k).  The widest k within 2 % of the best such bound: where
// the builds bound the step (C3: the slowest build) every build keeps a CU
// of its own as long as the sweep stays shorter; where the sweep does (C5: its
// 2048-row shard is ~86 CU-s of sweep against ~21 CU-s of builds) the side
// shrinks to what the builds need (224 -> ~60 CUs: 4.7 s -> ~0.6 s a step).
inline int qhull_side_balance(int n, double w_sweep, double w_build, double b_max) {
  const int kmax = n - n / 8;
  double best = 1e300;
  std::vector<double> t((size_t)kmax + 1, 0.0);
  for (int k = 1; k <= kmax; ++k) {
    t[k] = std::max(std::max(b_max, 1.15 * w_build / k), w_sweep / (double)(n - k));
    best = std::min(best, t[k]);
  }
  for (int k = kmax; k >= 1; --k)
    if (t[k] <= 1.02 * best) return k;
  return kmax;
}

// `known`: a step's feedback has arrived (false for a context's first two
// steps, and F is then kNoFeedback).  The caller has waited for the copy into
// F, so the schedule does not depend on host/GPU timing.
inline StepPlan plan_step(const StepShape& S, const StepKnobs& K, const StepFeedback& F, bool known) {
  StepPlan p{};
  // culling on: each row's slots are its K neighbours (k_nbr), not its N-1 pairs
  // (columns that are not rows: the obstacles' slots count like pair slots everywhere below)
  const int cols = S.npr + S.n_obs;
  const int npr = S.nbr_k > 0 ? std::min(S.nbr_k, cols) : cols;
  p.npr = npr;
  // the LDS hull variant packs outside-set extents in 32 bits (lqro_hull.hpp
  // seg_put: 15-bit count, 17-bit offset / 4 into HULL_SBMULT * H*NP entries)
  const bool lds_ok = S.hnp <= S.hull_lds_max_hnp && !K.hull_big_only;
  const long slots = (long)S.nrows * npr;
  // k_side sweeps rows in the hull's LDS (HullMemC) after its hulls: as many
  // of its waves take pairs as per-wave regions fit beside the row tables
  const long side_room = (long)S.hull_lds_doubles - S.lds_wave;
  const int side_waves = side_room > 0 ? (int)std::min<long>(std::min(S.hull_cwaves, S.waves),
                                                              side_room / S.wave_doubles) : 0;
  // the overlap pays where the hot pairs' hulls fit k_side's LDS topology
  // (C3: 177 hulls of <= 1,700 vertices); at H*NP > 16,383 (C5: 40 % of the
  // hulls outgrow its 2,048 vertices and retry in k_hull_big) the plain
  // schedule is faster (516 vs 1,150 ms per C5 shard step, scripts/c5_once.py)
  // crowded swarms (many inside-hull pairs in an earlier step) take the plain
  // schedule
  // The inside-hull count that picks the schedule is step t-2's, read after
  // that step's copy completed (the host runs at most one step ahead of the
  // GPU here).
  const unsigned long long inside_prev = F.inside;
  const double w_sweep = 1e-5 * (double)F.sweep_work;   // CU-ms, ms (the step two before)
  const double w_build = 1e-5 * (double)F.build_work;
  const double b_max = 1e-5 * (double)F.build_max;
  const unsigned long long retried_prev = F.retried;
  const bool lhull = K.local_hull || S.qhull_order;   // k_lhull or k_qhull on the side
  int side = lhull ? K.lside_cus : K.side_cus;
  const unsigned long long qspare =
      !known ? 0ull : K.qspare >= 0 ? (unsigned long long)K.qspare : inside_prev / 16 + 4;
  // the side's builds (workers): the last step's inside-hull count, or a
  // share of it (LQRO_QHULL_SIDE_PCT: the longest builds first, k_prio_save)
  unsigned long long qwant =
      known ? (inside_prev * (unsigned long long)K.qside_pct + 99ull) / 100ull + qspare : 0ull;
  if (S.qhull_order && K.qbalance && known && w_sweep > 0.0 && b_max > 0.0)
    qwant = std::min(qwant, (unsigned long long)qhull_side_balance(S.n_cu, w_sweep, w_build, b_max));
  if (S.qhull_order) {
    // Qhull's build is one long dependent chain per pair (one wave per CU):
    // the side takes one CU per expected hull, so every hot hull starts at
    // once, plus a few for pairs new this step (LQRO_QHULL_SPARE, default 4:
    // a pair beyond them waits for the first build to end), leaving at least
    // an eighth of the CUs to the sweep (unknown count: half the CUs).  With
    // speculative builds the main stream's sweep is as long as the slowest
    // build: each CU given back to it shortens the step (C3: 192 -> 181 side
    // CUs, 19.85 -> 19.35 ms, profiles/r5ak_ab_qhull_spare.txt)
    const unsigned long long want = known ? qwant : (unsigned long long)(S.n_cu / 2);
    side = (int)std::min<unsigned long long>((unsigned long long)(S.n_cu - S.n_cu / 8),
                                             std::max<unsigned long long>((unsigned long long)side, want));
  } else if (lhull) {
    // local hulls: at most ~3.7 inside-hull pairs per side CU (C3: 177 on
    // 48 CUs), widening up to half the CUs as the swarm gets denser
    if (known)
      side = (int)std::max<unsigned long long>(
          (unsigned long long)side,
          std::min<unsigned long long>(S.n_cu / 2, (inside_prev * 10ull + 36ull) / 37ull));
  } else if (known && inside_prev > 2ull * (unsigned long long)side) {
    // the LDS hull: beyond 2 inside-hull pairs per side CU the side widens by
    // a third (at most half the CUs)
    side = std::min(S.n_cu / 2, (4 * side) / 3);
  }
  // local hulls: the overlap pays up to ~16 inside-hull pairs per CU of the
  // widest side (1,067 at 22 m: 15.5 vs 18.0 ms plain; 2,496 at 16 m: a tie)
  // (Qhull's order: the overlap always pays, the hulls outlast the sweep)
  // (the LDS hull: beyond 4 per (widened) side CU the side CUs cannot keep up
  // with the hulls and the plain schedule — every CU on the hulls after the
  // sweep — is faster, scripts/crowded.py)
  const long max_inside = K.hot_max_inside >= 0 ? K.hot_max_inside
                          : S.qhull_order     ? LONG_MAX
                          : (lhull ? 16L * std::max(side, S.n_cu / 2) : 4L * side);
  const bool crowded = known && inside_prev > (unsigned long long)max_inside;
  // with the local hull the side stream is k_pair(hot) -> k_lhull -> k_pair
  // (rows, the same row queue): no LDS-topology condition
  // (Qhull order: until the work of a step is known — a context's first two
  // steps — the plain schedule: every CU sweeps, then the builds.  A side
  // guessed at half the CUs starved the sweep where it outweighs the builds:
  // C5's whole swarm took 11.7 s per unknown step against 3.4 s plain)
  const bool hot = K.hot_on && S.n_cu >= 64 && slots >= 65536 && S.nbr_k <= 0 && !crowded && side >= 1 &&
                   (known || !S.qhull_order) &&
                   (lhull || (lds_ok && S.hnp <= 16383 && side_waves >= 1));
  const int nwait = hot ? side : 0;
  p.row_split = std::max(1, std::min(16, (2 * S.n_cu + S.nrows - 1) / S.nrows));
  // Qhull order: the side's k_qhull workers sweep rows in their build's LDS
  // once the hot builds are taken (k_qside, 3 waves a CU): rows in units of
  // ~128 pairs, so a 3-wave worker's last unit ends soon after the 16-wave
  // workgroups' (shared gains: the tables are staged once per workgroup)
  const long qside_room = (long)S.qhull_lds_doubles - S.lds_wave;
  const int qside_waves = qside_room > 0 ? (int)std::min<long>(3, qside_room / S.wave_doubles) : 0;
  const bool qside = hot && K.qside && S.qhull_order && !K.qhull_big && qside_waves >= 1;
  if (qside && !S.per_agent) p.row_split = std::max(p.row_split, std::min(16, std::max(1, npr / 128)));
  // early LP (Qhull order, beside the hulls): a row whose planes are all
  // final runs its LP at once — in a k_lp_lds after the main sweep, or in the
  // k_qhull job that completes it (lqro_hull.hpp hull_row_done; rows of at
  // most LQRO_EARLY_LP_MAX_NPR pairs, longer ones go to the tail) — and the
  // tail only runs the rest (rows waiting on k_stale, rows closed late)
  // (the split step, lqro_step_device_begin / _end: the early rows' newV go
  // to the context's own buffer, copied into the caller's by _end; rows with
  // a facet-0 pair wait for the row-normal exchange in the tail as before)
  const bool early = hot && K.early_lp && S.qhull_order && !K.qhull_big && S.phase != 2 && S.nbr_k <= 0 &&
                     ((size_t)npr + (size_t)S.extra_planes) * 32 <= S.lp_lds_max && S.has_newv;
  p.early = early;
  p.early_internal = early && !S.newv_is_callers;
  const int units = S.nrows * p.row_split;
  const unsigned nblk = (unsigned)std::min(units, S.n_cu - nwait);
  const unsigned nside = (unsigned)std::max(0, std::min(units - (int)nblk, nwait));
  // Qhull order, split hot launch (every pair of the last step's list gets a
  // side CU of its own): side: the last step's inside-hull pairs, then
  // k_qhull; main: k_prio's other hot pairs, then the rows.  k_qhull's workers
  // wait for the main hot launch before leaving an empty queue.
  const bool split = hot && S.qhull_order && K.hot_split && !qside && !K.qhull_big && known &&
                     qwant <= (unsigned long long)nwait;
  // speculative builds (with the split): the last step's inside-hull pairs go
  // straight into the hull queue, so the side's k_qhull workers start building
  // them at once instead of after their evaluation (~0.5 ms at C3); the main
  // stream's hot launch evaluates them first, and each build commits only if
  // its pair is inside (PairArgs::spec_mark)
  const bool spec = split && K.hot_spec;
  p.slots = slots; p.lds_ok = lds_ok; p.side_waves = side_waves; p.qside_waves = qside_waves;
  p.hot = hot; p.side = side; p.nwait = nwait;
  p.split = split; p.spec = spec; p.qside = qside;
  p.nblk = nblk; p.nside = nside;
  // (k_qhull's in-place rebuild of capped builds where they happen: hulls of
  // more than 10,000 points (C5's ~19,000), or builds capped two steps before)
  p.big_inline = K.qhull_inline && !K.qhull_big && (S.hnp > 10000 || retried_prev > 0) ? 1 : 0;
  // (a row with fence or user planes: k_qhull's in-job LP knows the pair
  // planes only, so the job that closes the row leaves it to the tail; so
  // does one whose LP takes the obstacle slots first: the in-job LP compacts
  // in slot order)
  p.row_lp = npr <= S.early_lp_max_npr && S.extra_planes <= 0 && !S.hard_obs ? 1 : 0;
  p.row_target = p.row_split * S.row_big;
  return p;
}

}  // namespace lqro
