// lqro_hull_job.hpp — what every hull kernel (k_hull, k_hull_big, k_lhull,
// k_qhull, k_qhull_big) shares: the launch arguments (HullArgs), taking a job
// from the hull queue (hull_take_job), the job's pair (hull_job) and its
// reachable points (hull_points), the row counter of the early LP
// (hull_row_done), the notes a job leaves (hull_fail_note, qhmerge_note,
// hull_build_note) and the hl_* wave / workgroup helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lqro.h"
#include "lqro_device.hpp"

namespace lqro {

// an outside-set entry: the point and its (rounded) coordinates, so that
// re-distributing it needs one load
struct HullPt {
  double x, y, z;
  int q, pad;
};

struct HullWide;

struct HullArgs {
  int N, X, H, NP;
  int row_begin, npr, per_agent;
  int row_stride;                   // local row r is agent row_begin + r * row_stride
  const int* nbr_list;   // culling on: slot -> neighbour jj (see PairArgs), else null
  double r2, r2_lo, r2_hi;
  const double* T;
  const double* NCF;
  const double* S;
  const double* x;
  float* planes;
  lqro_pair_record* recs;
  const int* queue;
  const int* count;
  int cap;
  int* next;
  double* scratch;                  // per block: H*NP*6 doubles (rounded, full)
  int* iscratch;                    // per block: 2*H*NP*HULL_SCR_WAVES ints
  float* fscratch;                  // per block: H*NP floats (distance beyond the target)
  HullPt* sb;                       // per block: HULL_SBMULT*H*NP entries (outside-set segments)
  unsigned long long* fbest;        // per block: HULL_FB_STRIDE furthest-point keys
  int* vpid;                        // per block: HULL_VG_STRIDE vertex -> point ids
  int* stack;                       // per block: HULL_STKMULT*H*NP faces
  int* rqueue;                      // pairs that overflowed the LDS variant
  int* rcount;
  int* rnext;
  void* bigmem;                     // per block of k_hull_big: one HullMemBig
  HullWide* wide;                   // per block of k_hull: HULL_CWAVES wide-insertion lists
  int* bag;                         // per block of k_hull: HULL_BAGCAP overflow face ids (-1: empty)
  int block_base;                   // scratch index of this launch's block 0
  int big_main;                     // k_hull_big takes the main queue (H*NP too large for LDS)
  int big_inline;                   // k_qhull rebuilds a build past its caps in place (q3_big_inline)
  int qflags;                       // k_qhull: 1 helper waves locate long sequences, 2 the emit's lane state,
                                    // 4 wave 1 pre-scans the next speculation's queue entry, 16 a long
                                    // emit split over the waves, 32 no event for a not-sharp trigger,
                                    // 64 the helpers posted under the state a sharp trigger leads to
  int* lqueue;                      // k_lhull: pairs the local hull hands to the full hull
  int* lcount;
  int* ldone;                       // k_lhull: pairs it decided
  unsigned long long* lfail;        // k_lhull: hand-over reasons (16 counters, cumulative)
  unsigned long long* ljobs;        // k_lhull: per job (< 4096) 4 words: point / loop ticks (100 MHz), counts
  // lqro_debug_hull_points (test hook): the job's points given (already
  // rounded: P = P_rounded), k_hull's facets written out
  const double* ext_pts;
  int ext_n, ext_max;
  int ext_full;                     // ext_pts also holds the full-precision points (k_qhull hook)
  int* ext_facets;                  // ext_max x 3 point ids
  int* ext_nf;
  unsigned long long* stats;
  unsigned long long* prof;          // LQRO_HULL_PROFILE: per-phase cycles
  // k_qhull (LQRO_FLAG_QHULL_ORDER): per-worker scratch, per-slot normal and
  // distance, the slots whose facet 0 won (resolved by k_stale)
  char* qscratch;
  size_t qstride;
  double* qnrm;
  int* qstale;
  int* qstale_count;
  int qstale_cap;
  // early LP (lqro_runtime.hip, LQRO_ROW_BIG): rowpend counts each row's
  // open work down, rowclaim says who runs its LP (0 free, 1 claimed, 2 late:
  // a facet-0 pair waits for k_stale); the k_qhull job that completes a row
  // runs calculateNewV for it (lp_vgoal -> lp_newv).  Null: off.
  int* rowpend;
  int* rowclaim;
  int row_target;
  const double* lp_vgoal;
  double* lp_newv;
  double lp_vmax;
  // Qhull order: one timing record per build (hull_build_note), null: off
  unsigned long long* hbuild;
  int hbuild_cap;
  // jobs still being produced by a concurrent hot launch: a worker that finds
  // the queue empty waits until *prod_done reaches prod_total (its workgroups
  // finished) before it leaves; null: leave at once
  const int* prod_done;
  int prod_total;
  // Qhull order, speculative builds (PairArgs::spec_mark): a job whose slot
  // is marked >= 2 was queued before its pair was evaluated; the build
  // commits only once the mark is 3.  null: off
  const unsigned char* spec_mark;
  // ... and their queue entries 0 .. *spec_n - 1 are handed out by a plain
  // counter (*spec_next, one atomicAdd a worker: at the step's start every
  // side worker asks at once, and the head's compare-and-swap would hand
  // them out one round trip at a time); the queue's own head starts at
  // *spec_n.  null: off
  const int* spec_n;
  int* spec_next;
  // early LP: 1 when a k_qhull job that closes a row may run its LP in its
  // own LDS (rows of at most LQRO_EARLY_LP_MAX_NPR pairs); 0: such rows are
  // left to the tail
  int row_lp;
  // obstacle columns (lqro_set_obstacles[_ex]; oresp null: none): x holds the
  // agents' states, then the obstacles'; a row's slots jj >= obs_jj (= agents
  // - 1) are the obstacles'.  Obstacle o takes oresp[o] for the 0.5 of
  // LQRO:1416 and the point set of its class ocls[o] (null: every class 0):
  // 0 the agents' S, c >= 1 So + (c - 1) * NP * 3
  const double* So;
  const int* ocls;
  const double* oresp;
  int obs_jj;
  // interaction classes (lqro_set_interaction; null: none): an agent
  // column's factor is the table's (hull_factor)
  const IxDev* ix;
};

// Which of a row's slots are obstacle columns, for the kernels that finish a
// half-plane outside the hull kernels (k_stale, k_stale_rows): slot jj >= jj
// (through nbr_list with culling on) takes resp[jj - jj0].  resp null: no
// obstacles.  ix: the interaction table (null: none) an agent slot
// takes its factor from; nbr_list is set with either.
struct ObsSlots {
  const double* resp;
  const int* nbr_list;
  int jj;
  const IxDev* ix;
};

// the factor of LQRO:1416 for a slot's half-plane: 0.5 between agents, or the
// share of the row's class against the column's (lqro_set_interaction); the
// obstacle's own responsibility for an obstacle column (LQRO:1434: 1.0)
__device__ __forceinline__ double slot_factor(const int* nbr_list, int npr, long slot, const double* oresp,
                                              int obs_jj, const IxDev* ix, int row_begin, int row_stride) {
  if (!oresp && !ix) return 0.5;
  const int jj = nbr_list ? nbr_list[slot] : (int)(slot % npr);
  if (oresp && jj >= obs_jj) return oresp[jj - obs_jj];
  if (!ix) return 0.5;
  const int i = row_begin + (int)(slot / npr) * row_stride;
  return ix_share(ix, i, jj < i ? jj : jj + 1);
}
__device__ __forceinline__ double hull_factor(const HullArgs& A, int slot) {
  return slot_factor(A.nbr_list, A.npr, slot, A.oresp, A.obs_jj, A.ix, A.row_begin, A.row_stride);
}
// the point set of the column whose state is xj (x's rows past the agents'
// are the obstacles'): its class's
__device__ __forceinline__ const double* hull_col_sphere(const HullArgs& A, const double* xj) {
  if (!A.ocls) return A.S;
  const double* x0 = A.x + ((size_t)A.obs_jj + 1) * A.X;
  if (xj < x0) return A.S;
  const int cl = A.ocls[(xj - x0) / A.X];
  return cl > 0 ? A.So + (size_t)(cl - 1) * A.NP * 3 : A.S;
}

// (LQRO_ROW_BIG, lqro_device.hpp: the row counter's protocol; the early LP
// runs in k_qhull's facet-plane LDS: rows of at most LQRO_EARLY_LP_MAX_NPR
// pairs, planes and projections 32 B each)
#define LQRO_EARLY_LP_MAX_NPR 1024
// lane 0, after the job's plane (or its pending / failed flag) is written:
// count the row down; true when this job closed the row and claimed its LP
// (can_run: the caller will run it)
__device__ inline bool hull_row_done(const HullArgs& A, int slot, bool stale, bool can_run) {
  if (!A.rowpend) return false;
  const int lrow = slot / A.npr;
  if (stale) atomicExch(&A.rowclaim[lrow], 2);
  __threadfence();
  const int old = atomicSub(&A.rowpend[lrow], 1);
  const bool go = can_run && old - 1 == A.row_target && atomicCAS(&A.rowclaim[lrow], 0, 1) == 0;
  __threadfence();
  return go;
}

// (the step's counters, LQRO_ST_*: lqro_device.hpp)
#define LQRO_QHMERGE_K 1024.0   // the merge-suspect test's reach, x qh DISTround (q3_merge_suspect)
#define LQRO_HBUILD_CAP 16384

// an inside-hull pair left without its half-plane (a hull capacity): counted
// in LQRO_ST_HULLFAIL and named, so the step reports it (LQRO_E_HULL) instead of
// dropping the constraint silently
__device__ __forceinline__ void hull_fail_note(unsigned long long* stats, int slot) {
  atomicAdd(&stats[LQRO_ST_HULLFAIL], 1ull);
  const unsigned long long k = atomicAdd(&stats[LQRO_ST_NFAIL], 1ull);
  if (k < LQRO_ST_FAILMAX) stats[LQRO_ST_FAILS + k] = (unsigned long long)slot;
}

// a pair flagged LQRO_REC_QHMERGE_WIN: counted and named, so that lqro_step
// returns LQRO_E_QHMERGE instead of a silent difference from qconvex's merged
// facet (LQRO:925-967)
__device__ __forceinline__ void qhmerge_note(unsigned long long* stats, int slot) {
  const unsigned long long k = atomicAdd(&stats[LQRO_ST_MWIN], 1ull);
  if (k < LQRO_ST_FAILMAX) stats[LQRO_ST_MWINS + k] = (unsigned long long)slot;
}

// lane 0: a Qhull-order build's timing record (lqro_get_hull_builds):
// slot | kernel << 40, start, end (s_memrealtime, 100 MHz), points |
// insertions << 20 | facet slots << 40
__device__ __forceinline__ int hull_build_note(const HullArgs& A, int slot, int kernel, unsigned long long t0,
                                                int n, int nins, int nfac) {
  if (!A.hbuild) return -1;
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  atomicAdd(&A.stats[LQRO_ST_BWORK], t1 - t0);   // (the next steps' side width)
  atomicMax(&A.stats[LQRO_ST_BMAX], t1 - t0);
  const unsigned long long k = atomicAdd(&A.stats[LQRO_ST_NBUILD], 1ull);
  if (k >= (unsigned long long)A.hbuild_cap) return -1;
  unsigned long long* r = A.hbuild + 4 * k;
  r[0] = (unsigned long long)(unsigned)slot | ((unsigned long long)kernel << 40);
  r[1] = t0;
  r[2] = t1;
  r[3] = (unsigned long long)(n & 0xFFFFF) | ((unsigned long long)(nins & 0xFFFFF) << 20) |
         ((unsigned long long)(nfac & 0xFFFFF) << 40);
  return (int)k;
}

// Ordering point between the lanes of one wave.  A wave
// executes its LDS and its global memory operations in issue order, so only
// the compiler has to be kept from moving memory operations across this
// point; no s_waitcnt / s_barrier is needed (a workgroup fence would stall on
// every outstanding global store).
__device__ __forceinline__ void hl_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// compiler-only ordering of memory operations (LDS executes a wave's
// operations in issue order)
__device__ __forceinline__ void hl_cfence() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ int hl_ld(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void hl_st(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ double hl_rl(double v, int k) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, k);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), k);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Barrier across the workgroup's waves.
__device__ __forceinline__ void hl_bar() { __syncthreads(); }

// block-wide argmax of (key, idx), lowest idx on ties; result in every thread
template <class LT>
__device__ __forceinline__ void hl_argmax(LT& L, double& key, int& idx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ok = __shfl_xor(key, off);
    const int oi = __shfl_xor(idx, off);
    if (ok > key || (ok == key && oi < idx)) { key = ok; idx = oi; }
  }
  if (lane == 0) { L.rk[wave] = key; L.ri[wave] = idx; }
  hl_bar();
  key = L.rk[0]; idx = L.ri[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
    if (L.rk[w] > key || (L.rk[w] == key && L.ri[w] < idx)) { key = L.rk[w]; idx = L.ri[w]; }
  hl_bar();
}

// exclusive block scan of v (0/1); total in *tot
template <class LT>
__device__ __forceinline__ int hl_scan(LT& L, int v, int* tot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long b = __ballot(v != 0);
  const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) L.scan[wave] = __popcll(b);
  hl_bar();
  int base = 0, t = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
    if (w < wave) base += L.scan[w];
    t += L.scan[w];
  }
  *tot = t;
  hl_bar();
  return base + in_wave;
}

// ---------------------------------------------------------------------------
// A job's phases, the same in every hull kernel
// ---------------------------------------------------------------------------

// The pair of a job (a slot of the plane table): agents i and j, their states,
// i's tables and the relative velocity the facets are measured from.
struct HullJob {
  int i, j;
  const double* xi;
  const double* xj;
  const double* Ti;
  const double* Ni;
  double vrel[3];
};

__device__ __forceinline__ HullJob hull_job(const HullArgs& A, int slot) {
  HullJob J;
  const int lrow = slot / A.npr, jj = A.nbr_list ? A.nbr_list[slot] : slot % A.npr;
  J.i = A.row_begin + lrow * A.row_stride;
  J.j = jj < J.i ? jj : jj + 1;
  J.xi = A.x + (size_t)J.i * A.X;
  J.xj = A.x + (size_t)J.j * A.X;
  J.Ti = A.T + (A.per_agent ? (size_t)J.i * A.H * 9 : 0);
  J.Ni = A.NCF + (A.per_agent ? (size_t)J.i * A.H * 3 * A.X : 0);
  for (int k = 0; k < 3; k++) J.vrel[k] = J.xi[3 + k] - J.xj[3 + k];
  return J;
}

// Take the next job (pair slot), or -1 when the queue holds no untaken entry.
template <class LT>
__device__ __forceinline__ int hull_take_job(const HullArgs& A, LT& L, bool retryq) {
  const int* queue = retryq ? A.rqueue : A.queue;
  const int* qcount = retryq ? A.rcount : A.count;
  int* qnext = retryq ? A.rnext : A.next;
  if (threadIdx.x == 0) {
    // take an entry only if it is there (CAS on the head): a workgroup that
    // finds the queue empty consumes no index, so entries a concurrent k_pair
    // launch appends later are still taken (by the k_hull after the sweep)
    int job = -1, slot = -1;
    long waited = 0;
    if (A.spec_next && !retryq) {
      const int m = __hip_atomic_load(A.spec_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int j = m > 0 ? atomicAdd(A.spec_next, 1) : m;
      if (j < m) {   // (written by k_prio_prev, a kernel before this one)
        job = j;
        slot = queue[j];
      }
    }
    for (; job < 0;) {
      // (the producers' count first: once it is complete, every job they
      // appended is in qcount)
      const int pd = (A.prod_done && !retryq) ? __hip_atomic_load(A.prod_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
                                              : A.prod_total;
      const int nx = __hip_atomic_load(qnext, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      const int cnt = min(__hip_atomic_load(qcount, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT), A.cap);
      if (nx >= cnt) {
        // bounded: a worker that gives up leaves later jobs to the k_qhull
        // after the sweep (results do not depend on who builds)
        if (pd < A.prod_total && ++waited < (1l << 22)) {
          __builtin_amdgcn_s_sleep(4);
          continue;
        }
        break;
      }
      if (atomicCAS(qnext, nx, nx + 1) != nx) continue;
      job = nx;
      // counted before published: wait for k_pair's release store
      int v = __hip_atomic_load(queue + job, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      for (long w = 0; v < 0 && w < (1l << 26); ++w) {
        __builtin_amdgcn_s_sleep(2);
        v = __hip_atomic_load(queue + job, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      }
      slot = v;
      break;
    }
    L.job = job;
    L.slot = slot;
  }
  hl_bar();
  return L.slot;
}

// 1. The pair's reachable points in reference order, full precision (Pf)
// and %g-rounded (Pr); returns their number.  2. The tolerance eps, as the
// oracle's hull: 1e-13 (max|coord| + 1), in L.eps.
template <class LT>
__device__ __forceinline__ int hull_points(const HullArgs& A, LT& L, const double* Ti, const double* Ni,
                                           const double* xi, const double* xj, const double* vrel,
                                           double* Pr, double* Pf) {
  const int tid = threadIdx.x;
  const double* Sj = hull_col_sphere(A, xj);
  if (tid == 0) { L.n = A.ext_pts ? A.ext_n : 0; L.fail = 0; }
  hl_bar();
  if (A.ext_pts)
    for (int q = tid; q < 3 * A.ext_n; q += blockDim.x) {
      Pr[q] = A.ext_pts[q];
      Pf[q] = A.ext_full ? A.ext_pts[3 * A.ext_n + q] : A.ext_pts[q];
    }
  for (int k0 = 0; k0 < (A.ext_pts ? 0 : A.H); k0 += 128) {
    for (int it = tid; it < 3 * 128; it += blockDim.x) {
      const int k = k0 + it / 3, r = it % 3;
      if (k < A.H) {
        double d = 0.0;
        for (int c = 0; c < A.X; ++c) d += Ni[((size_t)k * 3 + r) * A.X + c] * (xi[c] - xj[c]);
        L.tr[it] = d;
      }
    }
    hl_bar();
    const int kend = min(A.H, k0 + 128);
    for (int q0 = k0 * A.NP; q0 < kend * A.NP; q0 += blockDim.x) {
      const int q = q0 + tid;
      bool ok = false;
      double p0 = 0, p1 = 0, p2 = 0;
      if (q < kend * A.NP) {
        const int k = q / A.NP, p = q % A.NP;
        const double* Tk = Ti + (size_t)k * 9;
        const double* tk = L.tr + (k - k0) * 3;
        const double u0 = Sj[3 * p] + tk[0], u1 = Sj[3 * p + 1] + tk[1], u2 = Sj[3 * p + 2] + tk[2];
        p0 = ((0.0 + Tk[0] * u0) + Tk[1] * u1) + Tk[2] * u2;
        p1 = ((0.0 + Tk[3] * u0) + Tk[4] * u1) + Tk[5] * u2;
        p2 = ((0.0 + Tk[6] * u0) + Tk[7] * u1) + Tk[8] * u2;
        const double a = p0 - vrel[0], b = p1 - vrel[1], c = p2 - vrel[2];
        const double t = a * a + b * b + c * c;
        if (t < A.r2_lo) ok = true;
        else if (t > A.r2_hi) ok = false;
        else ok = (a * a) / A.r2 + (b * b) / A.r2 + (c * c) / A.r2 < 1.0;
      }
      int tot;
      const int pos = L.n + hl_scan(L, ok ? 1 : 0, &tot);
      if (ok) {
        int oor = 0;
        Pf[3 * pos] = p0; Pf[3 * pos + 1] = p1; Pf[3 * pos + 2] = p2;
        Pr[3 * pos] = round6(p0, &oor);
        Pr[3 * pos + 1] = round6(p1, &oor);
        Pr[3 * pos + 2] = round6(p2, &oor);
        if (oor) L.fail = 7;
      }
      hl_bar();
      if (tid == 0) L.n += tot;
      hl_bar();
    }
  }
  const int n = L.n;
  double mx = 0.0;
  int dummy = 0;
  for (int q = tid; q < 3 * n; q += blockDim.x) mx = fmax(mx, fabs(Pr[q]));
  hl_argmax(L, mx, dummy);
  if (tid == 0) {
    L.eps = 1e-13 * (mx + 1.0);
    if (n < 4) L.fail = 8;
  }
  hl_bar();
  return n;
}

}  // namespace lqro
