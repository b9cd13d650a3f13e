// lqro_device.hpp — device-side fixed-size math shared by the lqro kernels.
//
// Exactness contract: liblqro.so is compiled with -ffp-contract=off, so each
// +, -, *, / below rounds once, exactly like the reference's x86-64 build.
// fp64 division and sqrt are IEEE correctly rounded on gfx950 (the default
// HIP lowering); fp32 division/sqrt use -fhip-fp32-correctly-rounded-divide-sqrt
// (hipcc's default).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lqro {

constexpr int kWave = 64;

// A row's LP may run as soon as every one of its planes is final.  rowpend
// (zeroed per step) adds LQRO_ROW_BIG for each finished row unit of the
// sweep, +1 for each hot pair (k_prio) and each inside-hull pair the sweep
// queues, -1 for each hot pair done without a hull and each hull job done:
// it equals row_split * LQRO_ROW_BIG exactly when the row has nothing open.
#define LQRO_ROW_BIG (1 << 20)

// ---------------------------------------------------------------------------
// The words of the counter blocks that the kernels and the runtime share
// ---------------------------------------------------------------------------
// The step's counters (the context's d_stats, zeroed per step): [0..7]
// lqro_get_stats' words, [8..11] lqro_get_stats_ex's:
#define LQRO_ST_PAIRS 0     // pairs (culling on: k_nbr counts the kept ones)
#define LQRO_ST_PLANES 1    // half-planes emitted
#define LQRO_ST_INSIDE 2    // inside-hull pairs (the next steps' schedule reads it, StepFeedback)
#define LQRO_ST_HULLOK 3    // inside-hull pairs whose hull gave the plane
#define LQRO_ST_HULLFAIL 4  // ... left without their half-plane (LQRO_E_HULL)
#define LQRO_ST_BACKUP 5    // GJK backup procedures
#define LQRO_ST_NREACH 6    // sum of n_reach
#define LQRO_ST_GTESTS 7    // sum of G-tests (GJK iterations)
#define LQRO_ST_MERGED 8    // Qhull-order hulls Qhull would merge facets in (LQRO_REC_QHMERGE)
#define LQRO_ST_RETRY 9     // builds k_qhull's caps handed to k_qhull_big
#define LQRO_ST_TIMEOUT 10  // k_qhull wave-handshake timeouts (the build went to k_qhull_big)
#define LQRO_ST_NFAIL 11    // pairs left without their half-plane, the first LQRO_ST_FAILMAX of their slots in [16 ..]
#define LQRO_ST_MWIN 12     // pairs flagged LQRO_REC_QHMERGE_WIN (lqro_get_stats_ex [11])
#define LQRO_ST_NBUILD 13   // Qhull-order build records written (HullArgs::hbuild)
#define LQRO_ST_FAILS 16
#define LQRO_ST_FAILMAX 64
#define LQRO_ST_MWINS (LQRO_ST_FAILS + LQRO_ST_FAILMAX)   // the first LQRO_ST_FAILMAX MWIN slots
// The step's work, for the next steps' schedule (the side's width): the
// sweep's workgroup time summed over k_pair's workgroups (one a CU), the
// Qhull-order builds' time summed and their maximum, on the 100 MHz clock
// (s_memrealtime)
#define LQRO_ST_SWORK (LQRO_ST_MWINS + LQRO_ST_FAILMAX)   // 144: the work words follow the named pairs
#define LQRO_ST_BWORK (LQRO_ST_SWORK + 1)
#define LQRO_ST_BMAX (LQRO_ST_SWORK + 2)
#define LQRO_ST_WORDS (LQRO_ST_SWORK + 4)

// The queue counters (the context's d_hcount, 16 ints zeroed per step): each
// queue's count, and the head its consumers advance
enum : int {
  LQRO_HC_HULL = 0,       // the hull queue (PairArgs::hull_count, HullArgs::count); k_prio_prev presets
  LQRO_HC_HULL_NEXT = 1,  //   both for the speculative builds
  LQRO_HC_RETRY = 2,      // jobs past the LDS hull's / k_qhull's caps (HullArgs::rcount)
  LQRO_HC_RETRY_NEXT = 3,
  LQRO_HC_ROW = 4,        // k_pair's row queue (PairArgs::row_counter)
  LQRO_HC_UNUSED5 = 5,
  LQRO_HC_HOT = 6,        // k_prio's hot list
  LQRO_HC_HOT_NEXT = 7,
  LQRO_HC_UNUSED8 = 8,
  LQRO_HC_LP4 = 9,        // k_lp_lds -> k_lp4 row list
  LQRO_HC_LP4_NEXT = 10,
  LQRO_HC_LHAND = 11,     // pairs k_lhull handed to the full hull (HullArgs::lcount)
  LQRO_HC_LHAND_NEXT = 12,
  LQRO_HC_LDONE = 13,     // pairs k_lhull decided
  LQRO_HC_UNUSED14 = 14,
  LQRO_HC_FACET0 = 15,    // Qhull order: slots whose facet 0 won (k_stale's list, HullArgs::qstale_count)
  LQRO_HC_WORDS = 16
};

// Qhull order, the split hot launch's counters (the context's d_hot2;
// [1..6] zeroed per split step, [0] carried from step to step)
enum : int {
  LQRO_H2_PREV = 0,        // the last step's inside-hull pairs (k_prio_save -> k_prio_prev)
  LQRO_H2_HOT1 = 1,        // the first hot launch's pair count
  LQRO_H2_HOT1_NEXT = 2,   // ... and its head
  LQRO_H2_HOT2_NEXT = 3,   // the second (main stream) hot launch's head
  LQRO_H2_HOT2_DONE = 4,   // ... and its finished workgroups (PairArgs::hot_done)
  LQRO_H2_SPEC = 5,        // speculative builds queued at the step's start
  LQRO_H2_SPEC_NEXT = 6,   // ... and the ticket that hands them out
  LQRO_H2_UNUSED7 = 7,
  LQRO_H2_WORDS = 8
};

// The profile words (the context's d_prof, cumulative; the lqro_debug_*
// calls read them): each region's first word
enum : int {
  LQRO_PROF_HULL = 0,                               // 32 hull counters
  LQRO_PROF_HJOBS = LQRO_PROF_HULL + 32,            // 2 words per hull job (< 4096)
  LQRO_PROF_PAIR = LQRO_PROF_HJOBS + 2 * 4096,      // k_pair's 16 phase words, then 16 hull wave phases
  LQRO_PROF_LFAIL = LQRO_PROF_PAIR + 16 + 16,       // k_lhull's 16 hand-over reasons
  LQRO_PROF_LJOBS = LQRO_PROF_LFAIL + 16,           // k_lhull's 4 words per job (< 4096)
  LQRO_PROF_QW1 = LQRO_PROF_LJOBS + 4 * 4096,       // k_qhull's wave 1 (Q3_PROF_W1), 64 words
  LQRO_PROF_QLONG = LQRO_PROF_QW1 + 64,             // LQRO_QHULL_LONGPROF: 24 x 1024
  LQRO_PROF_WORDS = LQRO_PROF_QLONG + 24 * 1024,
  LQRO_PROF_HULL_WORDS = LQRO_PROF_LFAIL            // what lqro_debug_hull_profile returns
};

// Workgroup-scope fence pair: orders this wave's LDS writes before other
// lanes' later reads (LDS executes a wave's instructions in order; this keeps
// the compiler from reordering and waits for lgkmcnt).
// x, opaque to the optimiser: values derived from it are recomputed after
// this point instead of being hoisted out of loops (each hoisted lane
// constant holds a VGPR for the whole kernel)
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// a double every lane holds alike, moved to scalar registers
__device__ __forceinline__ double uniform(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)b);
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// The activity mask (lqro_set_active) as the step's kernels read it: k_active's
// 0 / 1 bytes, the array padded to whole words.  agent_on_u is for an agent id
// every lane holds alike (k_pair: a wave takes one pair): one scalar load of
// the byte's word (the bytes do not change while the step's kernels run).
__device__ __forceinline__ bool agent_on_u(const unsigned char* act, int agent) {
  typedef const unsigned int __attribute__((address_space(4))) cword;
  const int a = __builtin_amdgcn_readfirstlane(agent);
  const unsigned int w = ((cword*)(const void*)act)[a >> 2];
  return ((w >> (8 * (a & 3))) & 0xFFu) != 0u;
}

// Interaction classes (lqro_set_interaction) as the step's kernels read them,
// one device block behind one pointer (null: no table, every agent column
// takes the 0.5 of LQRO:1416; a kernel's argument block and its scalar
// registers grow by that pointer alone): the C x C share table the setter
// copied and k_active's clamped class byte per agent, padded to whole words.
// share[cls[i] * C + cls[j]] is the factor row i applies against agent column
// j; exactly 0.0: row i ignores j (the slot is dead, as an inactive column's).
struct IxDev {
  double share[256];        // (LQRO_CLASSES_MAX squared)
  int C;
  int pad[3];
  unsigned char cls[4];     // (n_agents + 3) & ~3 bytes
};
__device__ __forceinline__ double ix_share(const IxDev* T, int i, int j) {
  return T->share[(int)T->cls[i] * T->C + (int)T->cls[j]];
}
// ... for a pair every lane holds alike (k_pair: a wave takes one pair): the
// two bytes' words and the entry by scalar loads, as agent_on_u
__device__ __forceinline__ double ix_share_u(const IxDev* T, int i, int j) {
  typedef const IxDev __attribute__((address_space(4))) cix;
  typedef const unsigned int __attribute__((address_space(4))) cword;
  cix* t = (cix*)(const void*)T;
  const int a = __builtin_amdgcn_readfirstlane(i), b = __builtin_amdgcn_readfirstlane(j);
  const unsigned int wa = ((cword*)t->cls)[a >> 2], wb = ((cword*)t->cls)[b >> 2];
  const int ca = (int)((wa >> (8 * (a & 3))) & 0xFFu), cb = (int)((wb >> (8 * (b & 3))) & 0xFFu);
  return t->share[ca * t->C + cb];
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// DPP lane moves (VALU, a few cycles) instead of ds_bpermute shuffles (LDS
// crossbar round trips) for wave reductions and scans.
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_i(int old, int x) {
  return __builtin_amdgcn_update_dpp(old, x, CTRL, ROWS, 0xF, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_d(double old, double x) {
  const long long o = __double_as_longlong(old), v = __double_as_longlong(x);
  const int lo = dpp_i<CTRL, ROWS>((int)o, (int)v);
  const int hi = dpp_i<CTRL, ROWS>((int)(o >> 32), (int)(v >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// inclusive prefix sum over the 64 lanes (all lanes active): row_shr steps
// inside each 16-lane row, then row_bcast:15 / row_bcast:31 across rows
__device__ __forceinline__ int wave_incl_scan(int x) {
  x += dpp_i<0x111, 0xF>(0, x);
  x += dpp_i<0x112, 0xF>(0, x);
  x += dpp_i<0x114, 0xF>(0, x);
  x += dpp_i<0x118, 0xF>(0, x);
  x += dpp_i<0x142, 0xA>(0, x);
  x += dpp_i<0x143, 0xC>(0, x);
  return x;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// operator! of include/matrix.h:603-671 for a 3x3: full pivoting, first
// strict maximum in (row, col) scan order, then back substitution and the
// column reshuffle.  Fully unrolled so the permutation stays in registers.
__device__ inline void inverse3(const double* q, double* out) {
  double m[9], inv[9];
  int rp[3] = {0, 1, 2}, cp[3] = {0, 1, 2};
#pragma unroll
  for (int i = 0; i < 9; ++i) { m[i] = q[i]; inv[i] = (i % 4 == 0) ? 1.0 : 0.0; }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double best = 0.0; int br = k, bc = k;
#pragma unroll
    for (int i = k; i < 3; ++i)
#pragma unroll
      for (int j = k; j < 3; ++j) {
        double a = fabs(m[rp[i] * 3 + cp[j]]);
        if (a > best) { best = a; br = i; bc = j; }
      }
    int t = rp[k]; rp[k] = rp[br]; rp[br] = t;
    t = cp[k]; cp[k] = cp[bc]; cp[bc] = t;
#pragma unroll
    for (int i = k + 1; i < 3; ++i) {
      double f = m[rp[i] * 3 + cp[k]] / m[rp[k] * 3 + cp[k]];
#pragma unroll
      for (int j = k + 1; j < 3; ++j) m[rp[i] * 3 + cp[j]] -= f * m[rp[k] * 3 + cp[j]];
#pragma unroll
      for (int j = 0; j < k; ++j) inv[rp[i] * 3 + rp[j]] -= f * inv[rp[k] * 3 + rp[j]];
      inv[rp[i] * 3 + rp[k]] = -f;
    }
  }
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    double qk = m[rp[k] * 3 + cp[k]];
#pragma unroll
    for (int j = 0; j < 3; ++j) inv[rp[k] * 3 + j] /= qk;
#pragma unroll
    for (int i = 0; i < k; ++i) {
      double f = m[rp[i] * 3 + cp[k]];
#pragma unroll
      for (int j = 0; j < 3; ++j) inv[rp[i] * 3 + j] -= f * inv[rp[k] * 3 + j];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[cp[i] * 3 + j] = inv[rp[i] * 3 + j];
}

// Exact emulation of what qconvex reads back from pointList.txt: the value
// printed by ostream's default format (%g, 6 significant digits, round half
// to even on the exact binary value, LQRObstacles.cpp:871-873) and parsed
// back with correct rounding.  Exact for 1e-15 <= |v| < 1e21 (two-product /
// exact-remainder arithmetic decides the rounding); outside that range
// *out_of_range is set.
__device__ inline double round6(double v, int* out_of_range) {
  if (v == 0.0 || !isfinite(v)) return v;
  const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                          1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  double a = fabs(v);
  if (!(a >= 1e-15 && a < 1e21)) { *out_of_range = 1; return v; }
  int e = (int)floor(log10(a));
  double m = 0.0;
  for (int iter = 0; iter < 3; ++iter) {
    int k = 5 - e;                 // scale a by 10^k into [1e5, 1e6)
    double y, lo;                  // exact value = y + lo (lo tiny)
    int dir;                       // sign of the exact residual: -1, 0, +1
    if (k >= 0) {
      double s = p10[k];
      y = a * s;
      lo = fma(a, s, -y);
      dir = (lo > 0) - (lo < 0);
    } else {
      double d = p10[-k];
      y = a / d;
      double r = fma(-y, d, a);    // a - y*d exactly
      lo = r;
      dir = (r > 0) - (r < 0);
    }
    (void)lo;
    // make sure 1e5 <= exact < 1e6
    if (y < 1e5 || (y == 1e5 && dir < 0)) { e -= 1; continue; }
    if (y > 1e6 || (y == 1e6 && dir >= 0)) { e += 1; continue; }
    double m0 = rint(y);           // half-even on y
    double t = y - m0;             // exact
    if (t == 0.5) {                // y = m0 + 0.5, m0 even
      if (dir > 0) m0 += 1.0;
    } else if (t == -0.5) {        // y = m0 - 0.5, m0 even
      if (dir < 0) m0 -= 1.0;
    }
    m = m0;
    break;
  }
  double r;
  int k = e - 5;
  if (k >= 0) r = m * p10[k];
  else r = m / p10[-k];
  return v < 0 ? -r : r;
}

}  // namespace lqro
