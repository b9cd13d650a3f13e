// lqro_qhull3_prof.hpp — k_qhull's diagnostics (lqro_qhull3.hpp), in one
// place: the profile-only state of a build (Q3Prof, a member of Q3S; empty in
// the plain build), the stamp macros the hot functions use (Q3T, W1T, Q3C)
// and what q3_body does with them at a job's start and end.  Two diagnostic
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
#else
#define Q3C(k, v) do {} while (0)
#endif

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

// wave 0, before the selection: the stamp phase 10 (q3_prof_flush) counts from
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

}  // namespace lqro
