// lqro_kern_clear.hip — the clearance measurement's kernels (lqro.h:
// lqro_clearance[_device], lqro_set_monitor): k_clear_pack,
// k_clear, k_clear_total.  An object of its own beside the step's kernels: it
// shares no header with k_pair or the hull kernels, and nothing in a step
// reads what it writes.
// Exactness: every + - * below rounds once (-ffp-contract=off), in the order
// lqro.h states, so tests/clearance_ref.py's numpy restatement matches bit
// for bit; minima are (value, index) keys, counts are integers.
#include <hip/hip_runtime.h>

#include <climits>

#include "lqro_kern.hpp"

// a pair is a hit when s2 < 1.0, strictly (a variant build with <= is what
// the exact-border test must catch: DESIGN §6.14)
#ifdef LQRO_CLEAR_HIT_LE
#define CL_HIT(s2) ((s2) <= 1.0)
#else
#define CL_HIT(s2) ((s2) < 1.0)
#endif

constexpr int CL_TR = 16;       // own rows a workgroup
constexpr int CL_BLOCK = 256;   // threads a workgroup = columns a pass
constexpr int CL_WAVES = CL_BLOCK / 64;

// the columns as a structure of arrays: px py pz wxy wz, ncols each; the
// agents from the given x, the obstacles from the context's obstacle array
// (never from the step's column array: the explicit call works without a step)
__global__ void __launch_bounds__(256) k_clear_pack(ClearArgs A) {
  const int ncols = A.n_agents + A.nobs;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  const double* p;
  double wxy, wz;
  if (c < A.n_agents) {
    p = A.x + (size_t)c * A.X;
    wxy = A.wxy; wz = A.wz;
  } else {
    const int o = c - A.n_agents;
    p = A.obs + (size_t)o * A.X;
    wxy = A.ow[2 * o]; wz = A.ow[2 * o + 1];
  }
  A.pack[c] = p[0];
  A.pack[(size_t)ncols + c] = p[1];
  A.pack[2 * (size_t)ncols + c] = p[2];
  A.pack[3 * (size_t)ncols + c] = wxy;
  A.pack[4 * (size_t)ncols + c] = wz;
}

__device__ __forceinline__ bool cl_less(double v, int j, double bv, int bj) {
  return v < bv || (v == bv && j < bj);
}

// A workgroup owns CL_TR own rows and streams the columns CL_BLOCK at a time:
// each lane loads one column (coalesced), then visits the tile's rows, whose
// positions are wave-uniform LDS reads, keeping a running (s2, j), (d2, j) and
// hit count per row in registers.  A lane's columns ascend, so its strict <
// keeps the smallest column of equal values; the lanes and the four waves are
// then joined over (value, column) keys.  The hit list is a second pass over
// the rows that have a hit, one wave a row, ballot-compacted in ascending
// column order until six are found.
__global__ void __launch_bounds__(CL_BLOCK) k_clear(ClearArgs A) {
  __shared__ double sp[3][CL_TR];
  __shared__ int si[CL_TR], s_on[CL_TR];   // s_on: the row takes part (lqro_set_active)
  __shared__ double w_s2[CL_WAVES][CL_TR], w_d2[CL_WAVES][CL_TR];
  __shared__ int w_js[CL_WAVES][CL_TR], w_jd[CL_WAVES][CL_TR], w_nh[CL_WAVES][CL_TR];
  __shared__ double f_s2[CL_TR], f_d2[CL_TR];
  __shared__ int f_js[CL_TR], f_jd[CL_TR], f_nh[CL_TR], f_hit[CL_TR][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncols = A.n_agents + A.nobs;
  const double* __restrict__ px = A.pack;
  const double* __restrict__ py = A.pack + (size_t)ncols;
  const double* __restrict__ pz = A.pack + 2 * (size_t)ncols;
  const double* __restrict__ pwxy = A.pack + 3 * (size_t)ncols;
  const double* __restrict__ pwz = A.pack + 4 * (size_t)ncols;
  const int row0 = blockIdx.x * CL_TR;
  if (tid < CL_TR) {
    const int lrow = row0 + tid;
    const int i = lrow < A.nrows ? A.row_begin + lrow * A.row_stride : -1;   // (-1: no such row; nothing is written)
    si[tid] = i;
    s_on[tid] = i >= 0 && (A.active == nullptr || A.active[i] != 0);
    sp[0][tid] = i >= 0 ? px[i] : 0.0;
    sp[1][tid] = i >= 0 ? py[i] : 0.0;
    sp[2][tid] = i >= 0 ? pz[i] : 0.0;
  }
  __syncthreads();
  const double inf = __builtin_huge_val();
  double bs[CL_TR], bd[CL_TR];
  int js[CL_TR], jd[CL_TR], nh[CL_TR];
#pragma unroll
  for (int r = 0; r < CL_TR; ++r) { bs[r] = inf; bd[r] = inf; js[r] = INT_MAX; jd[r] = INT_MAX; nh[r] = 0; }
  for (int c0 = 0; c0 < ncols; c0 += CL_BLOCK) {
    const int c = c0 + tid;
    // (an inactive agent is no column; the obstacle columns are not masked)
    if (c < ncols && (A.active == nullptr || c >= A.n_agents || A.active[c] != 0)) {
      const double cx = px[c], cy = py[c], cz = pz[c], cwxy = pwxy[c], cwz = pwz[c];
#pragma unroll
      for (int r = 0; r < CL_TR; ++r) {
        const double dx = sp[0][r] - cx, dy = sp[1][r] - cy, dz = sp[2][r] - cz;
        const double q = dx * dx + dy * dy;
        const double zz = dz * dz;
        const double d2 = q + zz;
        const double s2 = q * cwxy + zz * cwz;
        if (c != si[r]) {   // self by index, never by distance
          if (s2 < bs[r]) { bs[r] = s2; js[r] = c; }
          if (d2 < bd[r]) { bd[r] = d2; jd[r] = c; }
          nh[r] += CL_HIT(s2) ? 1 : 0;
        }
      }
    }
  }
  // the lanes of a wave, then the waves
#pragma unroll
  for (int r = 0; r < CL_TR; ++r) {
    double vs = bs[r], vd = bd[r];
    int cs = js[r], cd = jd[r], n = nh[r];
    for (int off = 32; off >= 1; off >>= 1) {
      const double os = __shfl_xor(vs, off), od = __shfl_xor(vd, off);
      const int ocs = __shfl_xor(cs, off), ocd = __shfl_xor(cd, off);
      n += __shfl_xor(n, off);
      if (cl_less(os, ocs, vs, cs)) { vs = os; cs = ocs; }
      if (cl_less(od, ocd, vd, cd)) { vd = od; cd = ocd; }
    }
    if (lane == 0) { w_s2[wave][r] = vs; w_js[wave][r] = cs; w_d2[wave][r] = vd; w_jd[wave][r] = cd; w_nh[wave][r] = n; }
  }
  __syncthreads();
  if (tid < CL_TR) {
    double vs = w_s2[0][tid], vd = w_d2[0][tid];
    int cs = w_js[0][tid], cd = w_jd[0][tid], n = w_nh[0][tid];
    for (int w = 1; w < CL_WAVES; ++w) {
      if (cl_less(w_s2[w][tid], w_js[w][tid], vs, cs)) { vs = w_s2[w][tid]; cs = w_js[w][tid]; }
      if (cl_less(w_d2[w][tid], w_jd[w][tid], vd, cd)) { vd = w_d2[w][tid]; cd = w_jd[w][tid]; }
      n += w_nh[w][tid];
    }
    f_s2[tid] = vs; f_js[tid] = cs == INT_MAX ? -1 : cs;
    f_d2[tid] = vd; f_jd[tid] = cd == INT_MAX ? -1 : cd;
    f_nh[tid] = n;
    for (int q = 0; q < 6; ++q) f_hit[tid][q] = -1;
  }
  __syncthreads();
  // the hit lists: the rows with a hit only, one wave a row
  for (int r = wave; r < CL_TR; r += CL_WAVES) {
    const int i = si[r];
    if (i < 0 || f_nh[r] == 0 || !s_on[r]) continue;   // (wave-uniform)
    const double rx = sp[0][r], ry = sp[1][r], rz = sp[2][r];
    int cnt = 0;
    for (int c0 = 0; c0 < ncols && cnt < 6; c0 += 64) {
      const int c = c0 + lane;
      bool h = false;
      if (c < ncols && c != i && (A.active == nullptr || c >= A.n_agents || A.active[c] != 0)) {
        const double dx = rx - px[c], dy = ry - py[c], dz = rz - pz[c];
        const double q = dx * dx + dy * dy;
        const double zz = dz * dz;
        const double s2 = q * pwxy[c] + zz * pwz[c];
        h = CL_HIT(s2);
      }
      const unsigned long long b = __ballot(h);
      if (h) {
        const int pos = cnt + __popcll(b & ((1ull << lane) - 1ull));
        if (pos < 6) f_hit[r][pos] = c;
      }
      cnt += __popcll(b);
    }
  }
  __syncthreads();
  if (tid < CL_TR && si[tid] >= 0) {
    lqro_clearance_row R;
    R.s2_min = f_s2[tid]; R.d2_min = f_d2[tid];
    R.j_s2 = f_js[tid]; R.j_d2 = f_jd[tid];
    R.n_hit = f_nh[tid];
    // the fence margin: k_fence's bound without the division by tau, the sign
    // turned; the lowest face index wins a tie
    double fm = inf;
    int ff = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double p = sp[a][tid];
      if ((A.faces >> (2 * a)) & 1) {
        const double g = p - (A.lo[a] + A.m[a]);
        if (g < fm) { fm = g; ff = 2 * a; }
      }
      if ((A.faces >> (2 * a + 1)) & 1) {
        const double g = (A.hi[a] - A.m[a]) - p;
        if (g < fm) { fm = g; ff = 2 * a + 1; }
      }
    }
    R.fence_min = fm; R.fence_face = ff;
    for (int q = 0; q < 6; ++q) R.hit[q] = f_hit[tid][q];
    if (!s_on[tid]) {   // not a measured row: the cleared record
      R.s2_min = R.d2_min = R.fence_min = inf;
      R.j_s2 = R.j_d2 = R.fence_face = -1;
      R.n_hit = 0;
      for (int q = 0; q < 6; ++q) R.hit[q] = -1;
    }
    A.rows[row0 + tid] = R;
  }
}

// the smaller (value, i, j) key
struct ClKey {
  double v;
  int i, j;
};
__device__ __forceinline__ bool cl_key_less(const ClKey& a, const ClKey& b) {
  return a.v < b.v || (a.v == b.v && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

// One workgroup over the rows: the last total with lqro.h's tie rules, then
// folded into the since-reset total (a strictly smaller minimum replaces the
// kept one, so its (i, j) are those of the earliest measurement attaining it).
__global__ void __launch_bounds__(256) k_clear_total(ClearArgs A) {
  __shared__ ClKey k_s[256], k_d[256], k_f[256];
  __shared__ long long n_h[256], n_r[256], n_o[256];
  const int tid = threadIdx.x;
  const double inf = __builtin_huge_val();
  ClKey ks{inf, INT_MAX, INT_MAX}, kd = ks, kf = ks;
  long long nh = 0, nr = 0, no = 0;
  for (int lrow = tid; lrow < A.nrows; lrow += 256) {
    const lqro_clearance_row R = A.rows[lrow];
    const int i = A.row_begin + lrow * A.row_stride;
    const ClKey a{R.s2_min, i, R.j_s2}, b{R.d2_min, i, R.j_d2}, f{R.fence_min, i, R.fence_face};
    if (cl_key_less(a, ks)) ks = a;
    if (cl_key_less(b, kd)) kd = b;
    if (R.fence_face >= 0 && cl_key_less(f, kf)) kf = f;
    nh += R.n_hit;
    nr += R.n_hit > 0 ? 1 : 0;
    no += R.fence_min < 0.0 ? 1 : 0;
  }
  k_s[tid] = ks; k_d[tid] = kd; k_f[tid] = kf;
  n_h[tid] = nh; n_r[tid] = nr; n_o[tid] = no;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
      if (cl_key_less(k_s[tid + w], k_s[tid])) k_s[tid] = k_s[tid + w];
      if (cl_key_less(k_d[tid + w], k_d[tid])) k_d[tid] = k_d[tid + w];
      if (cl_key_less(k_f[tid + w], k_f[tid])) k_f[tid] = k_f[tid + w];
      n_h[tid] += n_h[tid + w]; n_r[tid] += n_r[tid + w]; n_o[tid] += n_o[tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  lqro_clearance_total L;
  ks = k_s[0]; kd = k_d[0]; kf = k_f[0];
  if (!(ks.v < inf)) ks.i = ks.j = -1;   // (a minimum of +inf names no pair)
  if (!(kd.v < inf)) kd.i = kd.j = -1;
  if (!(kf.v < inf)) kf.i = kf.j = -1;
  L.s2_min = ks.v; L.s2_i = ks.i; L.s2_j = ks.j;
  L.d2_min = kd.v; L.d2_i = kd.i; L.d2_j = kd.j;
  L.fence_min = kf.v; L.fence_i = kf.i; L.fence_face = kf.j;
  L.n_hit = n_h[0]; L.n_rows_hit = n_r[0]; L.n_fence_out = n_o[0];
  L.n_measured = 1;
  lqro_clearance_total S = A.tot[1];
  if (L.s2_min < S.s2_min) { S.s2_min = L.s2_min; S.s2_i = L.s2_i; S.s2_j = L.s2_j; }
  if (L.d2_min < S.d2_min) { S.d2_min = L.d2_min; S.d2_i = L.d2_i; S.d2_j = L.d2_j; }
  if (L.fence_min < S.fence_min) { S.fence_min = L.fence_min; S.fence_i = L.fence_i; S.fence_face = L.fence_face; }
  S.n_hit += L.n_hit; S.n_rows_hit += L.n_rows_hit; S.n_fence_out += L.n_fence_out;
  S.n_measured += 1;
  A.tot[0] = L;
  A.tot[1] = S;
}

namespace lqro {

void launch_clear(hipStream_t s, const ClearArgs& A, hipEvent_t* ev) {
  const int ncols = A.n_agents + A.nobs;
  if (ev) (void)hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(k_clear_pack, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, A);
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(k_clear, dim3((unsigned)((A.nrows + CL_TR - 1) / CL_TR)), dim3(CL_BLOCK), 0, s, A);
  if (ev) (void)hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(k_clear_total, dim3(1), dim3(256), 0, s, A);
  if (ev) (void)hipEventRecord(ev[3], s);
}

}  // namespace lqro
