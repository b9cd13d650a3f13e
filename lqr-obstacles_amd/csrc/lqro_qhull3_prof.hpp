// lqro_qhull3_prof.hpp — k_qhull's diagnostics (lqro_qhull3.hpp), in one
// place: the profile-only state of a build (Q3Prof, a member of Q3S; empty in
// the plain build), the stamp macros the hot functions use (Q3T, W1T, Q3C,
// W1C), the diagnostic locals of an insertion, a wait and a queue scan
// (Q3InsProf, Q3WaitProf, Q3ScanProf, the stamps Q3Cy / Q3Rt) and the named
// hooks the hot functions call: a hook's body is behind the #ifdef here, its
// call site in lqro_qhull3.hpp is not, so the algorithm reads without them
// and the plain build compiles to the same kernels.  Two diagnostic
// builds (scripts/build_variant.sh): LQRO_QHULL_PROFILE (cycles per phase,
// scripts/qhull_prof.py; with LQRO_QHULL_PROF_LIGHT the stamps do not drain
// the memory queue) and LQRO_QHULL_LONGPROF (the long partitions of each
// build, scripts/qhull_long.py).  Everything here is empty without them.
#pragma once
#include "lqro_hull_job.hpp"

namespace lqro {

#define Q3_PROF_RETRY (LQRO_PROF_PAIR + 16)   // profile words: builds handed to k_qhull_big (16)
#ifdef LQRO_QHULL_PROFILE
#define Q3_CAPBIT(b) (b)   // which cap sent a build to k_qhull_big (scripts/qhull_prof.py)
#else
#define Q3_CAPBIT(b) 0
#endif

// wave 0's profile-only words of one build
struct Q3Prof {
#if defined(LQRO_QHULL_PROFILE) || defined(LQRO_QHULL_LONGPROF)
  unsigned long long tph[32];   // LQRO_QHULL_PROFILE: phase cycles 0..20, counters 21..28
  unsigned long long tq;         // LQRO_QHULL_PROFILE: the last stamp
  unsigned long long tjob;       // LQRO_QHULL_PROFILE: the job's start (after its points)
  unsigned long long tw, nw;     // LQRO_QHULL_PROFILE: waiting for wave 1's speculation
  unsigned long long tdl;        // LQRO_QHULL_PROFILE: its end until wave 0 sees it
  unsigned long long tw1, nw1;   // LQRO_QHULL_PROFILE: the waits after one-chunk insertions
  unsigned long long tse, tsn;   // LQRO_QHULL_PROFILE: publication -> speculation end, -> wave 0 past the wait
  unsigned long long tfr, nsp;   // LQRO_QHULL_PROFILE: the wait's first read, its spins
  unsigned long long tfr2, trel;
  unsigned long long r_start, r_done, r_seen, r_gseen;
  unsigned long long tseen, tpre, npre, tstart;
  int prev1;
  unsigned long long tps[24], nps;   // LQRO_QHULL_PROFILE: phases of the one-chunk insertions
  unsigned long long lp_n, lp_pts, lp_t, lp_all, lp_tloc, lp_wait, lp_adopt, lp_tail, lp_tw;   // LQRO_QHULL_LONGPROF
  unsigned long long lp_own, lp_got, lp_hwait, lp_stop, lp_ev, lp_posts;
#endif
};

#if defined(LQRO_QHULL_PROFILE) && defined(LQRO_QHULL_PROF_LIGHT)
// (light: no drain — a phase is charged the waits the build itself makes
// there, so the phases add up to the undisturbed critical path)
#define Q3T(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); S.pf.tph[k] += t_ - S.pf.tq; S.pf.tq = t_; } while (0)
#elif defined(LQRO_QHULL_PROFILE)
// (every outstanding load and store drained first: a phase is charged its own memory waits)
#define Q3T(k) do { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); S.pf.tph[k] += t_ - S.pf.tq; S.pf.tq = t_; } while (0)
#else
#define Q3T(k) do {} while (0)
#endif
// LQRO_QHULL_PROFILE counters: 21 insertions, 22 partitioned points, 23 located
// chunks, 24 sequence events, 25 emitted destination groups, 31 adopted speculations
// Wave 1's own phases and wave 0's wait for it (LQRO_QHULL_PROFILE): prof words
// Q3_PROF_W1 + k: 0 speculation total, 1 the adopted cone's vertex records,
// 2 queue scan, 3 horizon, 4 cone, 5 match / checkzero / sharp, 6 serving
// chunks, 7 speculations, 8 chunks served, 9 wave 0 waiting for a speculation,
// 10 waits; 16 + k: wave 0's phase k (Q3T) over the insertions whose partition
// sequence fits one chunk (np <= 64), 40 their number; cycles summed over the
// step's hulls (lqro_debug_prof_words)
#define Q3_PROF_W1 LQRO_PROF_QW1
// LQRO_QHULL_LONGPROF (a diagnostic build, scripts/build_variant.sh): per
// build record k (lqro_get_hull_builds order, k < 1024), prof words
// Q3_PROF_LONG + 24 k: insertions whose partition sequence is longer than one
// chunk, their points, their ticks (100 MHz, from the publication to the end
// of the emit), the ticks of all the build's partitions, the long ones' ticks
// to the end of their locate; wave 0's ticks waiting for the speculation,
// from the wait to the publication, from the emit's end to the next wait;
// chunks of helped sequences wave 0 located, chunks the helpers did, ticks
// waiting for them, ticks stopping them, events, posts; helper chunks and
// their ticks; wave 1's speculations, publication -> seen and seen -> done
// ticks; wave 0's waits and their speculation-end -> seen ticks
#define Q3_PROF_LONG LQRO_PROF_QLONG
// wave 1's profile-only words of one job
struct Q3P {
  unsigned long long tq2 = 0;   // LQRO_QHULL_PROFILE: the last speculation's end (this wave's clock)
  unsigned long long t[16];
  unsigned long long tq;
};
#if defined(LQRO_QHULL_PROFILE) && defined(LQRO_QHULL_PROF_LIGHT)
#define W1T(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); P.t[k] += t_ - P.tq; P.tq = t_; } while (0)
#elif defined(LQRO_QHULL_PROFILE)
#define W1T(k) do { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); P.t[k] += t_ - P.tq; P.tq = t_; } while (0)
#else
#define W1T(k) do {} while (0)
#endif
#ifdef LQRO_QHULL_PROFILE
#define Q3C(k, v) do { S.pf.tph[k] += (unsigned long long)(v); } while (0)
#define W1C(k, v) do { P.t[k] += (unsigned long long)(v); } while (0)   // wave 1's counters (11: horizon levels)
#else
#define Q3C(k, v) do {} while (0)
#define W1C(k, v) do {} while (0)
#endif

// a stamp a hook below takes and a later one reads: cycles (LQRO_QHULL_PROFILE)
// and the 100 MHz real time (LQRO_QHULL_LONGPROF)
struct Q3Cy {
#ifdef LQRO_QHULL_PROFILE
  unsigned long long t;
#endif
};
struct Q3Rt {
#ifdef LQRO_QHULL_LONGPROF
  unsigned long long t;
#endif
};
__device__ __forceinline__ void q3_cy_now(Q3Cy& c) {
#ifdef LQRO_QHULL_PROFILE
  c.t = __builtin_amdgcn_s_memtime();
#endif
}
__device__ __forceinline__ void q3_rt_now(Q3Rt& r) {
#ifdef LQRO_QHULL_LONGPROF
  r.t = __builtin_amdgcn_s_memrealtime();
#endif
}

// q3_wait's probe, for wave 0's wait for a speculation: the time of the
// first read back and the reads after it
struct Q3WaitProf {
#ifdef LQRO_QHULL_PROFILE
  unsigned long long tf;
  int spins;
#endif
  __device__ __forceinline__ void first() {
#ifdef LQRO_QHULL_PROFILE
    tf = __builtin_amdgcn_s_memtime();
#endif
  }
  __device__ __forceinline__ void spin() {
#ifdef LQRO_QHULL_PROFILE
    ++spins;
#endif
  }
};

// wave 0's profile-only words of one insertion (q3_build's loop)
struct Q3InsProf {
#ifdef LQRO_QHULL_PROFILE
  unsigned long long snap[21];   // Q3Prof::tph at its start
  unsigned long long tins;       // its start (for the long-sequence split)
#endif
  Q3Cy tw;         // the wait for the speculation begins
  Q3WaitProf wp;
  Q3Rt ta, t0;     // its start, its publication
};

// wave 1's profile-only words of one queue scan and horizon (q3_spec)
struct Q3ScanProf {
  Q3Rt t0, t1;     // the scan's start and end
#ifdef LQRO_QHULL_LONGPROF
  int reloads;     // queue-window reloads
#endif
};

// wave 0, before a job's build: its words zeroed
__device__ __forceinline__ void q3_prof_begin(Q3Prof& F) {
#if defined(LQRO_QHULL_PROFILE) || defined(LQRO_QHULL_LONGPROF)
  F.lp_n = F.lp_pts = F.lp_t = F.lp_all = F.lp_tloc = F.lp_wait = F.lp_adopt = F.lp_tail = F.lp_tw = 0;
  F.lp_own = F.lp_got = F.lp_hwait = F.lp_stop = F.lp_ev = F.lp_posts = 0;
#endif
#ifdef LQRO_QHULL_PROFILE
  for (int k = 0; k < 32; k++) F.tph[k] = 0;
  F.tw = F.nw = 0;
  F.tdl = 0;
  F.tw1 = F.nw1 = 0;
  F.tse = F.tsn = 0;
  F.tfr = F.nsp = 0;
  F.tfr2 = 0;
  F.trel = 0;
  F.r_start = F.r_done = F.r_seen = F.r_gseen = 0;
  F.tseen = F.tpre = F.npre = F.tstart = 0;
  F.prev1 = 0;
  for (int k = 0; k < 24; k++) F.tps[k] = 0;
  F.nps = 0;
  F.tjob = __builtin_amdgcn_s_memtime();
#endif
}

// wave 0, at q3_build's start and before the selection: the stamp the next
// Q3T, or phase 10 (q3_prof_flush), counts from
__device__ __forceinline__ void q3_prof_stamp(Q3Prof& F) {
#ifdef LQRO_QHULL_PROFILE
  F.tq = __builtin_amdgcn_s_memtime();
#endif
}

// wave 0, a job committed (n points, nalloc facet slots): its words added to
// the step's (A.prof)
__device__ __forceinline__ void q3_prof_flush(const HullArgs& A, Q3Prof& F, int n, int nalloc, int lane) {
#ifdef LQRO_QHULL_PROFILE
  F.tph[10] = __builtin_amdgcn_s_memtime() - F.tq;
  F.tph[27] = __builtin_amdgcn_s_memtime() - F.tjob;   // the whole job (26: its max over jobs)
  F.tph[28] = (unsigned long long)n;
  if (A.prof && lane == 0) {
    for (int k = 0; k < 32; k++)
      if (k != 26 && k != 11) atomicAdd(&A.prof[k], F.tph[k]);
    atomicAdd(&A.prof[Q3_PROF_W1 + 9], F.tw);
    atomicAdd(&A.prof[Q3_PROF_W1 + 10], F.nw);
    for (int k = 0; k < 24; k++) atomicAdd(&A.prof[Q3_PROF_W1 + 16 + k], F.tps[k]);
    atomicAdd(&A.prof[Q3_PROF_W1 + 40], F.nps);
    atomicAdd(&A.prof[Q3_PROF_W1 + 41], F.tdl);
    atomicAdd(&A.prof[Q3_PROF_W1 + 42], F.tw1);
    atomicAdd(&A.prof[Q3_PROF_W1 + 43], F.nw1);
    atomicAdd(&A.prof[Q3_PROF_W1 + 44], F.tse);
    atomicAdd(&A.prof[Q3_PROF_W1 + 45], F.tsn);
    atomicAdd(&A.prof[Q3_PROF_W1 + 46], F.tfr);
    atomicAdd(&A.prof[Q3_PROF_W1 + 47], F.nsp);
    atomicAdd(&A.prof[Q3_PROF_W1 + 48], F.tfr2);
    atomicAdd(&A.prof[Q3_PROF_W1 + 49], F.trel);
    atomicAdd(&A.prof[Q3_PROF_W1 + 50], F.r_start);
    atomicAdd(&A.prof[Q3_PROF_W1 + 51], F.r_done);
    atomicAdd(&A.prof[Q3_PROF_W1 + 52], F.r_seen);
    atomicAdd(&A.prof[Q3_PROF_W1 + 53], F.r_gseen);
    atomicAdd(&A.prof[Q3_PROF_W1 + 54], F.tpre);
    atomicAdd(&A.prof[Q3_PROF_W1 + 55], F.npre);
    atomicAdd(&A.prof[Q3_PROF_W1 + 56], F.tstart);
    atomicMax(&A.prof[26], F.tph[27]);
    // per job (words 32 + 2j): cycles; insertions | points << 20 | facet slots << 40
    const unsigned long long j = atomicAdd(&A.prof[11], 1ull);
    if (j < 4096) {
      A.prof[32 + 2 * j] = F.tph[27];
      A.prof[33 + 2 * j] = F.tph[21] | ((unsigned long long)n << 20) | ((unsigned long long)nalloc << 40);
    }
  }
#endif
}

// lane 0 of wave 0, a build handed to k_qhull_big: counted, the caps it hit, its slot
__device__ __forceinline__ void q3_prof_retry(const HullArgs& A, int status, int slot) {
#ifdef LQRO_QHULL_PROFILE
  if (A.prof) {
    const unsigned long long k = atomicAdd(&A.prof[Q3_PROF_RETRY], 1ull);
    atomicOr(&A.prof[Q3_PROF_RETRY + 1], (unsigned long long)status);
    if (k < 14) A.prof[Q3_PROF_RETRY + 2 + k] = (unsigned long long)slot | ((unsigned long long)status << 32);
  }
#endif
}

// wave 1, its job over: its words added to the step's
__device__ __forceinline__ void q3_prof_w1_flush(const HullArgs& A, const Q3P& P, int lane) {
#ifdef LQRO_QHULL_PROFILE
  if (A.prof && lane == 0)
    for (int k = 0; k < 16; k++) atomicAdd(&A.prof[Q3_PROF_W1 + k], P.t[k]);
#endif
}

// LQRO_QHULL_LONGPROF, thread 0 at a job's start: the helpers' words (LT: Q3L)
template <class LT>
__device__ __forceinline__ void q3_longprof_begin(LT& L) {
#ifdef LQRO_QHULL_LONGPROF
  for (int k = 0; k < 12; k++) L.hprof[k] = 0ull;
  L.lp_pubr = L.lp_doner = 0ull;
#endif
}

// LQRO_QHULL_LONGPROF, lane 0 of wave 0: the record of build k (hull_build_note's index)
template <class LT>
__device__ __forceinline__ void q3_longprof_flush(const HullArgs& A, int k, const Q3Prof& F, const LT& L) {
#ifdef LQRO_QHULL_LONGPROF
  if (A.prof && k >= 0 && k < 1024) {
    unsigned long long* r = A.prof + Q3_PROF_LONG + 24 * k;
    r[0] = F.lp_n; r[1] = F.lp_pts; r[2] = F.lp_t; r[3] = F.lp_all;
    r[4] = F.lp_tloc; r[5] = F.lp_wait; r[6] = F.lp_adopt - F.lp_wait; r[7] = F.lp_tail;
    r[8] = F.lp_own; r[9] = F.lp_got; r[10] = F.lp_hwait; r[11] = F.lp_stop; r[12] = F.lp_ev; r[13] = F.lp_posts;
    r[14] = L.hprof[0]; r[15] = L.hprof[1] | (L.hprof[2] << 32);
    for (int q = 3; q < 11; q++) r[13 + q] = L.hprof[q];   // r[16..23]
  }
#endif
}

// ---- the hooks of the hot functions, in the order they are met ----
// (LT: Q3L, defined after this header; its diagnostic members are read from
// LDS by name of the address space, as q3_lds does)
#define Q3_PROF_LDS(r) (*(const __attribute__((address_space(3))) unsigned long long*)(&(r)))

// q3_help, lane 0, its chunk released: claimed at t0, located by t1
template <class LT>
__device__ __forceinline__ void q3_lp_helped(LT& L, const Q3Rt& t0, const Q3Rt& t1) {
#ifdef LQRO_QHULL_LONGPROF
  const unsigned long long th2 = __builtin_amdgcn_s_memrealtime();
  atomicAdd(&L.hprof[0], 1ull);
  atomicAdd(&L.hprof[1], t1.t - t0.t);
  atomicAdd(&L.hprof[2], th2 - t0.t);
#endif
}

// q3_locate_seq: wave 0 waited (or not) since tw0 for a helper's chunk
__device__ __forceinline__ void q3_lp_hwait(Q3Prof& F, const Q3Rt& tw0, bool waited) {
#ifdef LQRO_QHULL_LONGPROF
  if (waited) F.lp_hwait += __builtin_amdgcn_s_memrealtime() - tw0.t;
#endif
}
// a chunk of a helped sequence: located by wave 0 (mine) or taken from a helper
__device__ __forceinline__ void q3_lp_chunk(Q3Prof& F, bool mine) {
#ifdef LQRO_QHULL_LONGPROF
  if (mine) F.lp_own++; else F.lp_got++;
#endif
}
// a helped sequence's helpers stopped (since ts0) after a post; ev: by an event
__device__ __forceinline__ void q3_lp_stopped(Q3Prof& F, const Q3Rt& ts0, bool help, bool ev) {
#ifdef LQRO_QHULL_LONGPROF
  if (help) {
    F.lp_stop += __builtin_amdgcn_s_memrealtime() - ts0.t;
    F.lp_posts++;
    if (ev) F.lp_ev++;
  }
#endif
}

// q3_spec: the queue scan begins, reloads its window, ends; the horizon ends
__device__ __forceinline__ void q3_lp_scan_begin(Q3ScanProf& C) {
  q3_rt_now(C.t0);
#ifdef LQRO_QHULL_LONGPROF
  C.reloads = 0;
#endif
}
__device__ __forceinline__ void q3_lp_scan_reload(Q3ScanProf& C) {
#ifdef LQRO_QHULL_LONGPROF
  ++C.reloads;
#endif
}
template <class LT>
__device__ __forceinline__ void q3_lp_scan_end(LT& L, Q3ScanProf& C, int lane) {
  q3_rt_now(C.t1);
#ifdef LQRO_QHULL_LONGPROF
  if (lane == 0) { L.hprof[8] += (unsigned long long)C.reloads; L.hprof[9] += C.t1.t - C.t0.t; }
#endif
}
template <class LT>
__device__ __forceinline__ void q3_lp_horizon_end(LT& L, const Q3ScanProf& C, int lane) {
#ifdef LQRO_QHULL_LONGPROF
  if (lane == 0) L.hprof[10] += __builtin_amdgcn_s_memrealtime() - C.t1.t;
#endif
}

// q3_build, an insertion begins: the phases so far; the tail since the last partition
__device__ __forceinline__ void q3_prof_ins_begin(Q3Prof& F, Q3InsProf& I) {
#ifdef LQRO_QHULL_PROFILE
  for (int k = 0; k < 21; k++) I.snap[k] = F.tph[k];
#endif
  q3_rt_now(I.ta);
#ifdef LQRO_QHULL_LONGPROF
  F.lp_tail += F.lp_tw ? I.ta.t - F.lp_tw : 0ull;
#endif
}
// before wave 0's wait for the speculation (q3_wait with I.wp)
__device__ __forceinline__ void q3_prof_wait_begin(Q3InsProf& I) {
  q3_cy_now(I.tw);
#ifdef LQRO_QHULL_PROFILE
  I.wp.spins = 0;
#endif
}
// and after it
template <class LT>
__device__ __forceinline__ void q3_prof_wait_end(Q3Prof& F, LT& L, const Q3InsProf& I, int lane) {
#ifdef LQRO_QHULL_PROFILE
  if (F.prev1) { F.tfr += I.wp.tf - I.tw.t; F.nsp += (unsigned long long)I.wp.spins; }
#endif
#ifdef LQRO_QHULL_LONGPROF
  {   // (wave 0 waited: the speculation's end -> seen here)
    const unsigned long long tn = __builtin_amdgcn_s_memrealtime();
    const unsigned long long de = Q3_PROF_LDS(L.lp_doner);
    if (tn - I.ta.t > 20 && tn > de && lane == 0) { L.hprof[6] += tn - de; L.hprof[7] += 1; }
  }
#endif
#ifdef LQRO_QHULL_PROFILE
  {
    const unsigned long long tn_ = __builtin_amdgcn_s_memtime();
    F.tw += tn_ - I.tw.t;
    F.nw += 1;
    if (tn_ - I.tw.t > 200) F.tdl += tn_ - L.done_t;   // (waited) speculation end -> seen here
    F.tseen = tn_;
    if (F.prev1) {   // after a one-chunk insertion: its wait, publication -> speculation end / -> seen
      F.tw1 += tn_ - I.tw.t; F.nw1 += 1;
      F.tse += L.done_t - L.pub_t; F.tsn += tn_ - L.pub_t;
      F.tfr2 += L.done_t2 - L.pub_t;
      const unsigned long long nr_ = __builtin_amdgcn_s_memrealtime();
      F.r_start += L.start_r - L.pub_r; F.r_done += L.done_r - L.pub_r; F.r_seen += nr_ - L.pub_r;
    }
  }
#endif
#ifdef LQRO_QHULL_LONGPROF
  F.lp_wait += __builtin_amdgcn_s_memrealtime() - I.ta.t;
#endif
}
// the insertion's point is chosen (after Q3T(1))
__device__ __forceinline__ void q3_prof_ins_chosen(const Q3Prof& F, Q3InsProf& I) {
#ifdef LQRO_QHULL_PROFILE
  I.tins = F.tq;
#endif
}
// before the publication to wave 1 (the release of L.ph) ...
template <class LT>
__device__ __forceinline__ void q3_prof_publish(Q3Prof& F, LT& L, Q3InsProf& I, int lane) {
#ifdef LQRO_QHULL_PROFILE
  if (lane == 0) { L.pub_t = __builtin_amdgcn_s_memtime(); L.pub_r = __builtin_amdgcn_s_memrealtime(); }
  // (this wave's clock) seen -> publication
  if (F.tseen) { F.tpre += __builtin_amdgcn_s_memtime() - F.tseen; F.npre += 1; }
#endif
  q3_rt_now(I.t0);
#ifdef LQRO_QHULL_LONGPROF
  F.lp_adopt += I.t0.t - I.ta.t;   // (less the wait, in lp_wait)
  if (lane == 0) L.lp_pubr = I.t0.t;
#endif
}
// ... and after it: the release's own cost
template <class LT>
__device__ __forceinline__ void q3_prof_published(Q3Prof& F, const LT& L, int lane) {
#ifdef LQRO_QHULL_PROFILE
  if (lane == 0) F.trel += __builtin_amdgcn_s_memtime() - L.pub_t;
#endif
}
// the partition sequence (np points) is located
__device__ __forceinline__ void q3_lp_located(Q3Prof& F, const Q3InsProf& I, int np) {
#ifdef LQRO_QHULL_LONGPROF
  if (np > 64) F.lp_tloc += __builtin_amdgcn_s_memrealtime() - I.t0.t;
#endif
}
// and emitted (or empty)
__device__ __forceinline__ void q3_lp_partitioned(Q3Prof& F, const Q3InsProf& I, int np) {
#ifdef LQRO_QHULL_LONGPROF
  const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - I.t0.t;
  F.lp_all += dt;
  if (np > 64) { F.lp_n += 1; F.lp_pts += (unsigned long long)np; F.lp_t += dt; }
  F.lp_tw = I.t0.t + dt;
#endif
}
// the insertion is over: those whose partition sequence is longer than one
// chunk (29 cycles, 30 count) apart from the one-chunk ones (tps, nps)
__device__ __forceinline__ void q3_prof_ins_end(Q3Prof& F, const Q3InsProf& I, int np) {
#ifdef LQRO_QHULL_PROFILE
  F.prev1 = np <= 64;
  if (np > 64) { F.tph[29] += F.tq - I.tins; F.tph[30] += 1; }
  else {
    for (int k = 0; k < 21; k++) F.tps[k] += F.tph[k] - I.snap[k];
    F.nps += 1;
  }
#endif
}

// q3_body, wave 1: a speculation begins (t0, ts: for the hooks after it)
template <class LT>
__device__ __forceinline__ void q3_prof_spec_begin(LT& L, Q3P& P, Q3Cy& t0, Q3Rt& ts, int lane) {
  q3_cy_now(t0);
#ifdef LQRO_QHULL_PROFILE
  P.tq = t0.t;
  P.t[14] += t0.t - L.pub_t;   // publication -> speculation start
  if (P.tq2) P.t[15] += t0.t - P.tq2;   // (this wave's clock) its last speculation's end -> this start
  if (lane == 0) L.start_r = __builtin_amdgcn_s_memrealtime();
#endif
  q3_rt_now(ts);
}
// it is over, before its results are released
template <class LT>
__device__ __forceinline__ void q3_prof_spec_done(LT& L, const Q3Rt& ts, int lane) {
#ifdef LQRO_QHULL_LONGPROF
  if (lane == 0) {
    const unsigned long long te_ = __builtin_amdgcn_s_memrealtime();
    L.hprof[3] += 1; L.hprof[4] += ts.t - Q3_PROF_LDS(L.lp_pubr); L.hprof[5] += te_ - ts.t;
    L.lp_doner = te_;
  }
#endif
#ifdef LQRO_QHULL_PROFILE
  if (lane == 0) L.done_t = __builtin_amdgcn_s_memtime();
#endif
}
// and after the release and the prescan
template <class LT>
__device__ __forceinline__ void q3_prof_spec_end(LT& L, Q3P& P, const Q3Cy& t0, int lane) {
#ifdef LQRO_QHULL_PROFILE
  if (lane == 0) { L.done_t2 = __builtin_amdgcn_s_memtime(); L.done_r = __builtin_amdgcn_s_memrealtime(); }
  P.tq2 = __builtin_amdgcn_s_memtime();
  P.t[0] += __builtin_amdgcn_s_memtime() - t0.t;
  P.t[7] += 1;
#endif
}
// wave 1 located a posted chunk (since t0)
__device__ __forceinline__ void q3_prof_w1_helped(Q3P& P, const Q3Cy& t0) {
#ifdef LQRO_QHULL_PROFILE
  P.t[6] += __builtin_amdgcn_s_memtime() - t0.t;
  P.t[8] += 1;
#endif
}

}  // namespace lqro
