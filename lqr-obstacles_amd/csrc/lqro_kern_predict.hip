// lqro_kern_predict.hip — the horizon conflict prediction's kernels (lqro.h:
// lqro_predict[_device], lqro_predict_paths[_device]):
// k_pred_cg, k_pred_paths, k_pred_tr, k_conf, k_conf_obs, k_conf_total.  An
// object of its own beside the step's kernels, as the clearance monitor's: it
// shares no header with k_pair, the hull kernels or the LP, and nothing in a
// step reads what it writes.
// Exactness: every + - * below rounds once (-ffp-contract=off), sums ascend
// from 0.0 in the order lqro.h states, so tests/predict_ref.py's numpy
// restatement matches bit for bit; minima are (value, index) keys, counts are
// integers.  No division, no sqrt.
#include <hip/hip_runtime.h>

#include <climits>

#include "lqro_kern.hpp"

// a pair-slice is a hit when s2 < 1.0, strictly (a variant build with <= is
// what the exact-border test must catch: DESIGN §6.17)
#ifdef LQRO_PREDICT_HIT_LE
#define PR_HIT(s2) ((s2) <= 1.0)
#else
#define PR_HIT(s2) ((s2) < 1.0)
#endif

constexpr int PR_TR = LQRO_PREDICT_TILE;   // own rows a workgroup
constexpr int PR_BLOCK = 256;              // threads a workgroup = columns a pass
constexpr int PR_WAVES = PR_BLOCK / 64;
#define PR_MAXX 16

// Per gains set: k_tables' own G recursion in its order (lqro_kern_lp.hip),
// whose rows 0..2 after update k + 1 are CG_k.  One workgroup a set; thread
// (r, c) owns entry (r, c).
__global__ void __launch_bounds__(256) k_pred_cg(PredArgs P) {
  __shared__ double sAt[PR_MAXX * PR_MAXX], sBt[PR_MAXX * 3], sG[PR_MAXX * 3];
  const int X = P.X, U = P.U, set = blockIdx.x, t = threadIdx.x;
  const double* Li = P.L + (P.nsets > 1 ? (size_t)set * U * X : 0);
  const double* Ei = P.E + (P.nsets > 1 ? (size_t)set * U * 3 : 0);
  if (t < X * X) {
    const int r = t / X, c = t % X;
    double bl = 0.0;
    for (int k = 0; k < U; ++k) bl += P.B[r * U + k] * Li[k * X + c];
    sAt[r * X + c] = P.A[r * X + c] + bl;
  }
  const bool own = t < X * 3;
  const int r = own ? t / 3 : 0, c = own ? t % 3 : 0;
  if (own) {
    double be = 0.0;
    for (int k = 0; k < U; ++k) be += P.B[r * U + k] * Ei[k * 3 + c];
    sBt[r * 3 + c] = be;
    sG[r * 3 + c] = 0.0;
  }
  __syncthreads();
  double* out = P.cg + (size_t)set * P.H * 9;
  for (int k = 0; k < P.H; ++k) {   // (every thread runs the loop: the barriers are the workgroup's)
    double g = 0.0;
    if (own)
      for (int m = 0; m < X; ++m) g += sAt[r * X + m] * sG[m * 3 + c];
    const double gn = g + sBt[r * 3 + c];
    __syncthreads();
    if (own) {
      sG[r * 3 + c] = gn;
      if (r < 3) out[(size_t)k * 9 + r * 3 + c] = gn;
    }
    __syncthreads();
  }
}

// Per agent and slice: P = (CG_k v) - (NCF_k x) with the agent's own set, into
// the structure of arrays path[k][3][nc] (the agent index fastest, so k_conf's
// column loads coalesce).
__global__ void __launch_bounds__(256) k_pred_paths(PredArgs P) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)P.n_agents * P.H) return;
  const int a = (int)(idx % P.n_agents), k = (int)(idx / P.n_agents), X = P.X;
  const size_t set = P.nsets > 1 ? (size_t)a : 0;
  const double* cg = P.cg + (set * P.H + k) * 9;
  const double* ncf = P.NCF + (set * P.H + k) * 3 * X;
  const double* x = P.x + (size_t)a * X;
  const double* v = P.v + (size_t)a * 3;
  for (int r = 0; r < 3; ++r) {
    double s = 0.0, f = 0.0;
    for (int c = 0; c < 3; ++c) s += cg[r * 3 + c] * v[c];
    for (int m = 0; m < X; ++m) f += ncf[r * X + m] * x[m];
    P.path[((size_t)k * 3 + r) * P.nc + a] = s - f;
  }
}

// The given-paths calls: the caller's [column][k][3] into the same layout.
__global__ void __launch_bounds__(256) k_pred_tr(PredArgs P) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)P.nc * P.H) return;
  const int c = (int)(idx % P.nc), k = (int)(idx / P.nc);
  const double* g = P.given + ((size_t)c * P.H + k) * 3;
  for (int r = 0; r < 3; ++r) P.path[((size_t)k * 3 + r) * P.nc + c] = g[r];
}

__device__ __forceinline__ bool pr_less(double v, int j, int k, double bv, int bj, int bk) {
  return v < bv || (v == bv && (j < bj || (j == bj && k < bk)));
}
__device__ __forceinline__ bool pr_first_less(int k, int j, int bk, int bj) { return k < bk || (k == bk && j < bj); }

// A workgroup owns PR_TR own rows, whose paths sit in LDS as [k][row][3], and
// streams the columns PR_BLOCK at a time: each lane takes one column
// (coalesced loads, slice by slice) and visits the tile's rows at every slice
// (wave-uniform LDS reads), keeping per row a running (s2, j, k), (d2, j, k),
// first hit (k, j) and conflict count in registers.  A lane's columns ascend
// and a column's slices ascend, so its strict < keeps the smallest (column,
// slice) of equal values and the smallest column of an equal first slice; the
// lanes and the four waves are then joined over the keys.  Every loop's trip
// count is the same in all lanes (a lane without a column works on column 0
// and keeps nothing).  The conflict list is a second pass over the rows that
// have one, one wave a row, ballot-compacted in ascending column order until
// four are found.
__global__ void __launch_bounds__(PR_BLOCK) k_conf(PredArgs P) {
  extern __shared__ double sp[];   // [H][PR_TR][3]
  __shared__ int si[PR_TR], s_on[PR_TR];
  __shared__ double w_s2[PR_WAVES][PR_TR], w_d2[PR_WAVES][PR_TR];
  __shared__ int w_js[PR_WAVES][PR_TR], w_ks[PR_WAVES][PR_TR], w_jd[PR_WAVES][PR_TR], w_kd[PR_WAVES][PR_TR];
  __shared__ int w_kf[PR_WAVES][PR_TR], w_jf[PR_WAVES][PR_TR], w_nc[PR_WAVES][PR_TR];
  __shared__ int f_nc[PR_TR], f_conf[PR_TR][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = P.H, ncols = P.ncols;
  const size_t nc = (size_t)P.nc;
  const double* __restrict__ path = P.path;
  const int row0 = blockIdx.x * PR_TR;
  if (tid < PR_TR) {
    const int lrow = row0 + tid;
    const int i = lrow < P.nrows ? P.row_begin + lrow * P.row_stride : -1;   // (-1: no such row; nothing is written)
    si[tid] = i;
    s_on[tid] = i >= 0 && (P.active == nullptr || P.active[i] != 0);
  }
  __syncthreads();
  for (int q = tid; q < H * PR_TR * 3; q += PR_BLOCK) {
    const int k = q / (PR_TR * 3), r = (q / 3) % PR_TR, a = q % 3, i = si[r];
    sp[q] = i >= 0 ? path[((size_t)k * 3 + a) * nc + i] : 0.0;
  }
  __syncthreads();
  const double inf = __builtin_huge_val();
  double bs[PR_TR], bd[PR_TR];
  int js[PR_TR], ks[PR_TR], jd[PR_TR], kd[PR_TR], kf[PR_TR], jf[PR_TR], ncf[PR_TR];
#pragma unroll
  for (int r = 0; r < PR_TR; ++r) {
    bs[r] = inf; bd[r] = inf;
    js[r] = ks[r] = jd[r] = kd[r] = kf[r] = jf[r] = INT_MAX;
    ncf[r] = 0;
  }
  for (int c0 = 0; c0 < ncols; c0 += PR_BLOCK) {
    const int c = c0 + tid;
    // (an inactive agent is no column; obstacle columns are not masked)
    const bool ok = c < ncols && (P.active == nullptr || c >= P.n_agents || P.active[c] != 0);
    const int cl = c < ncols ? c : 0;
    const double cwxy = cl < P.n_agents ? P.wxy : P.ow[2 * (cl - P.n_agents)];
    const double cwz = cl < P.n_agents ? P.wz : P.ow[2 * (cl - P.n_agents) + 1];
    unsigned take = 0, hit = 0;   // bit r: row r measures this column (self by index, never by distance); it has a hit
#pragma unroll
    for (int r = 0; r < PR_TR; ++r) take |= (ok && c != si[r]) ? 1u << r : 0u;
    for (int k = 0; k < H; ++k) {
      const double cx = path[((size_t)k * 3) * nc + cl], cy = path[((size_t)k * 3 + 1) * nc + cl],
                   cz = path[((size_t)k * 3 + 2) * nc + cl];
      const double* rp = sp + (size_t)k * (PR_TR * 3);
#pragma unroll
      for (int r = 0; r < PR_TR; ++r) {
        const double dx = rp[r * 3] - cx, dy = rp[r * 3 + 1] - cy, dz = rp[r * 3 + 2] - cz;
        const double q = dx * dx + dy * dy;
        const double zz = dz * dz;
        const double d2 = q + zz;
        const double s2 = q * cwxy + zz * cwz;
        const bool t = (take >> r) & 1u;
        if (t && s2 < bs[r]) { bs[r] = s2; js[r] = c; ks[r] = k; }
        if (t && d2 < bd[r]) { bd[r] = d2; jd[r] = c; kd[r] = k; }
        const bool h = t && PR_HIT(s2);
        if (h && k < kf[r]) { kf[r] = k; jf[r] = c; }
        hit |= h ? 1u << r : 0u;
      }
    }
#pragma unroll
    for (int r = 0; r < PR_TR; ++r) ncf[r] += (hit >> r) & 1u;
  }
  // the lanes of a wave, then the waves
#pragma unroll
  for (int r = 0; r < PR_TR; ++r) {
    double vs = bs[r], vd = bd[r];
    int cs = js[r], xs = ks[r], cd = jd[r], xd = kd[r], fk = kf[r], fj = jf[r], n = ncf[r];
    for (int off = 32; off >= 1; off >>= 1) {
      const double os = __shfl_xor(vs, off), od = __shfl_xor(vd, off);
      const int ocs = __shfl_xor(cs, off), oxs = __shfl_xor(xs, off), ocd = __shfl_xor(cd, off), oxd = __shfl_xor(xd, off);
      const int ofk = __shfl_xor(fk, off), ofj = __shfl_xor(fj, off);
      n += __shfl_xor(n, off);
      if (pr_less(os, ocs, oxs, vs, cs, xs)) { vs = os; cs = ocs; xs = oxs; }
      if (pr_less(od, ocd, oxd, vd, cd, xd)) { vd = od; cd = ocd; xd = oxd; }
      if (pr_first_less(ofk, ofj, fk, fj)) { fk = ofk; fj = ofj; }
    }
    if (lane == 0) {
      w_s2[wave][r] = vs; w_js[wave][r] = cs; w_ks[wave][r] = xs;
      w_d2[wave][r] = vd; w_jd[wave][r] = cd; w_kd[wave][r] = xd;
      w_kf[wave][r] = fk; w_jf[wave][r] = fj; w_nc[wave][r] = n;
    }
  }
  __syncthreads();
  if (tid < PR_TR) {
    for (int w = 1; w < PR_WAVES; ++w) {
      if (pr_less(w_s2[w][tid], w_js[w][tid], w_ks[w][tid], w_s2[0][tid], w_js[0][tid], w_ks[0][tid])) {
        w_s2[0][tid] = w_s2[w][tid]; w_js[0][tid] = w_js[w][tid]; w_ks[0][tid] = w_ks[w][tid];
      }
      if (pr_less(w_d2[w][tid], w_jd[w][tid], w_kd[w][tid], w_d2[0][tid], w_jd[0][tid], w_kd[0][tid])) {
        w_d2[0][tid] = w_d2[w][tid]; w_jd[0][tid] = w_jd[w][tid]; w_kd[0][tid] = w_kd[w][tid];
      }
      if (pr_first_less(w_kf[w][tid], w_jf[w][tid], w_kf[0][tid], w_jf[0][tid])) {
        w_kf[0][tid] = w_kf[w][tid]; w_jf[0][tid] = w_jf[w][tid];
      }
      w_nc[0][tid] += w_nc[w][tid];
    }
    f_nc[tid] = w_nc[0][tid];
    for (int q = 0; q < 4; ++q) f_conf[tid][q] = -1;
  }
  __syncthreads();
  // the conflict lists: the rows with a conflict only, one wave a row
  for (int r = wave; r < PR_TR; r += PR_WAVES) {
    const int i = si[r];
    if (i < 0 || f_nc[r] == 0 || !s_on[r]) continue;   // (wave-uniform)
    int cnt = 0;
    for (int c0 = 0; c0 < ncols && cnt < 4; c0 += 64) {   // (cnt comes from a ballot: wave-uniform)
      const int c = c0 + lane;
      const bool ok = c < ncols && c != i && (P.active == nullptr || c >= P.n_agents || P.active[c] != 0);
      const int cl = c < ncols ? c : 0;
      const double cwxy = cl < P.n_agents ? P.wxy : P.ow[2 * (cl - P.n_agents)];
      const double cwz = cl < P.n_agents ? P.wz : P.ow[2 * (cl - P.n_agents) + 1];
      bool any = false;
      for (int k = 0; k < H; ++k) {
        const double* rp = sp + ((size_t)k * PR_TR + r) * 3;
        const double dx = rp[0] - path[((size_t)k * 3) * nc + cl], dy = rp[1] - path[((size_t)k * 3 + 1) * nc + cl],
                     dz = rp[2] - path[((size_t)k * 3 + 2) * nc + cl];
        const double q = dx * dx + dy * dy;
        const double zz = dz * dz;
        const double s2 = q * cwxy + zz * cwz;
        any = any || PR_HIT(s2);
      }
      const bool h = ok && any;
      const unsigned long long b = __ballot(h);
      if (h) {
        const int pos = cnt + __popcll(b & ((1ull << lane) - 1ull));
        if (pos < 4) f_conf[r][pos] = c;
      }
      cnt += __popcll(b);
    }
  }
  __syncthreads();
  if (tid < PR_TR && si[tid] >= 0) {
    lqro_predict_row R;
    const bool on = s_on[tid] != 0;
    const int cs = w_js[0][tid], cd = w_jd[0][tid], fk = w_kf[0][tid];
    R.s2_min = on ? w_s2[0][tid] : inf;
    R.d2_min = on ? w_d2[0][tid] : inf;
    R.j_s2 = on && cs != INT_MAX ? cs : -1; R.k_s2 = on && cs != INT_MAX ? w_ks[0][tid] : -1;
    R.j_d2 = on && cd != INT_MAX ? cd : -1; R.k_d2 = on && cd != INT_MAX ? w_kd[0][tid] : -1;
    R.k_first = on && fk != INT_MAX ? fk : -1; R.j_first = on && fk != INT_MAX ? w_jf[0][tid] : -1;
    R.n_conf = on ? f_nc[tid] : 0;
    R.reserved = 0;
    for (int q = 0; q < 4; ++q) R.conf[q] = on ? f_conf[tid][q] : -1;
    P.rows[row0 + tid] = R;
  }
}

// The obstacle columns of the predicting calls, behind k_conf: one wave an own
// row, the obstacle's path from the row's own tables and v_o = x_o[3..5], one
// slice a lane; the obstacles in turn, each joined over (value, slice) keys
// and merged into the row's record.  An obstacle column is larger than every
// agent column, so only a strictly smaller value or first slice replaces what
// the record holds.  One code path for shared and per-agent gains.
__global__ void __launch_bounds__(64) k_conf_obs(PredArgs P) {
  const int lrow = blockIdx.x, lane = threadIdx.x;
  const int i = P.row_begin + lrow * P.row_stride, X = P.X, H = P.H;
  if (P.active != nullptr && P.active[i] == 0) return;   // (the cleared record stays)
  const size_t set = P.nsets > 1 ? (size_t)i : 0, nc = (size_t)P.nc;
  const double* cg = P.cg + set * H * 9;
  const double* ncf = P.NCF + set * H * 3 * X;
  const double inf = __builtin_huge_val();
  const lqro_predict_row R0 = P.rows[lrow];
  double s2m = R0.s2_min, d2m = R0.d2_min;
  int j_s2 = R0.j_s2, k_s2 = R0.k_s2, j_d2 = R0.j_d2, k_d2 = R0.k_d2, k_first = R0.k_first, j_first = R0.j_first;
  int n_conf = R0.n_conf, c0 = R0.conf[0], c1 = R0.conf[1], c2 = R0.conf[2], c3 = R0.conf[3];
  for (int o = 0; o < P.nobs; ++o) {
    const double* xo = P.obs + (size_t)o * X;
    const double wxy = P.ow[2 * o], wz = P.ow[2 * o + 1];
    const int col = P.n_agents + o;
    double vs = inf, vd = inf;
    int xs = INT_MAX, xd = INT_MAX, fk = INT_MAX;
    for (int k0 = 0; k0 < H; k0 += 64) {
      const int k = k0 + lane;
      const bool ok = k < H;
      const int kc = ok ? k : 0;
      double d[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s = 0.0, f = 0.0;
        for (int c = 0; c < 3; ++c) s += cg[kc * 9 + r * 3 + c] * xo[3 + c];
        for (int m = 0; m < X; ++m) f += ncf[((size_t)kc * 3 + r) * X + m] * xo[m];
        d[r] = P.path[((size_t)kc * 3 + r) * nc + i] - (s - f);
      }
      const double q = d[0] * d[0] + d[1] * d[1];
      const double zz = d[2] * d[2];
      const double d2 = q + zz;
      const double s2 = q * wxy + zz * wz;
      if (ok && s2 < vs) { vs = s2; xs = k; }
      if (ok && d2 < vd) { vd = d2; xd = k; }
      if (ok && PR_HIT(s2) && k < fk) fk = k;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const double os = __shfl_xor(vs, off), od = __shfl_xor(vd, off);
      const int oxs = __shfl_xor(xs, off), oxd = __shfl_xor(xd, off), ofk = __shfl_xor(fk, off);
      if (os < vs || (os == vs && oxs < xs)) { vs = os; xs = oxs; }
      if (od < vd || (od == vd && oxd < xd)) { vd = od; xd = oxd; }
      fk = ofk < fk ? ofk : fk;
    }
    if (vs < s2m) { s2m = vs; j_s2 = col; k_s2 = xs; }
    if (vd < d2m) { d2m = vd; j_d2 = col; k_d2 = xd; }
    if (fk != INT_MAX) {
      if (k_first < 0 || fk < k_first) { k_first = fk; j_first = col; }
      if (n_conf == 0) c0 = col;
      else if (n_conf == 1) c1 = col;
      else if (n_conf == 2) c2 = col;
      else if (n_conf == 3) c3 = col;
      ++n_conf;
    }
  }
  if (lane != 0) return;
  lqro_predict_row R;
  R.s2_min = s2m; R.d2_min = d2m;
  R.j_s2 = j_s2; R.k_s2 = k_s2; R.j_d2 = j_d2; R.k_d2 = k_d2;
  R.k_first = k_first; R.j_first = j_first;
  R.n_conf = n_conf; R.reserved = 0;
  R.conf[0] = c0; R.conf[1] = c1; R.conf[2] = c2; R.conf[3] = c3;
  P.rows[lrow] = R;
}

// the smaller (value, i, j, k) key; the smaller (k, i, j) key
struct PrKey {
  double v;
  int i, j, k;
};
__device__ __forceinline__ bool pr_key_less(const PrKey& a, const PrKey& b) {
  return a.v < b.v || (a.v == b.v && (a.i < b.i || (a.i == b.i && (a.j < b.j || (a.j == b.j && a.k < b.k)))));
}
struct PrFirst {
  int k, i, j;
};
__device__ __forceinline__ bool pr_fkey_less(const PrFirst& a, const PrFirst& b) {
  return a.k < b.k || (a.k == b.k && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

// One workgroup over the rows: the last total with lqro.h's tie rules, then
// folded into the since-reset total (a strictly smaller value replaces the
// kept one, so its indices are those of the earliest measurement attaining it).
__global__ void __launch_bounds__(256) k_conf_total(PredArgs P) {
  __shared__ PrKey k_s[256], k_d[256];
  __shared__ PrFirst k_f[256];
  __shared__ long long n_c[256], n_r[256];
  const int tid = threadIdx.x;
  const double inf = __builtin_huge_val();
  PrKey ks{inf, INT_MAX, INT_MAX, INT_MAX}, kd = ks;
  PrFirst kf{INT_MAX, INT_MAX, INT_MAX};
  long long ncf = 0, nr = 0;
  for (int lrow = tid; lrow < P.nrows; lrow += 256) {
    const lqro_predict_row R = P.rows[lrow];
    const int i = P.row_begin + lrow * P.row_stride;
    const PrKey a{R.s2_min, i, R.j_s2, R.k_s2}, b{R.d2_min, i, R.j_d2, R.k_d2};
    const PrFirst f{R.k_first, i, R.j_first};
    if (pr_key_less(a, ks)) ks = a;
    if (pr_key_less(b, kd)) kd = b;
    if (R.k_first >= 0 && pr_fkey_less(f, kf)) kf = f;
    ncf += R.n_conf;
    nr += R.n_conf > 0 ? 1 : 0;
  }
  k_s[tid] = ks; k_d[tid] = kd; k_f[tid] = kf;
  n_c[tid] = ncf; n_r[tid] = nr;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
      if (pr_key_less(k_s[tid + w], k_s[tid])) k_s[tid] = k_s[tid + w];
      if (pr_key_less(k_d[tid + w], k_d[tid])) k_d[tid] = k_d[tid + w];
      if (pr_fkey_less(k_f[tid + w], k_f[tid])) k_f[tid] = k_f[tid + w];
      n_c[tid] += n_c[tid + w]; n_r[tid] += n_r[tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  lqro_predict_total L;
  ks = k_s[0]; kd = k_d[0]; kf = k_f[0];
  if (!(ks.v < inf)) ks.i = ks.j = ks.k = -1;   // (a minimum of +inf names no pair)
  if (!(kd.v < inf)) kd.i = kd.j = kd.k = -1;
  if (kf.k == INT_MAX) kf.k = kf.i = kf.j = -1;
  L.s2_min = ks.v; L.s2_i = ks.i; L.s2_j = ks.j; L.s2_k = ks.k;
  L.d2_min = kd.v; L.d2_i = kd.i; L.d2_j = kd.j; L.d2_k = kd.k;
  L.first_k = kf.k; L.first_i = kf.i; L.first_j = kf.j; L.reserved = 0;
  L.n_conf = n_c[0]; L.n_rows_conf = n_r[0];
  L.n_measured = 1;
  lqro_predict_total S = P.tot[1];
  if (L.s2_min < S.s2_min) { S.s2_min = L.s2_min; S.s2_i = L.s2_i; S.s2_j = L.s2_j; S.s2_k = L.s2_k; }
  if (L.d2_min < S.d2_min) { S.d2_min = L.d2_min; S.d2_i = L.d2_i; S.d2_j = L.d2_j; S.d2_k = L.d2_k; }
  if (L.first_k >= 0 && (S.first_k < 0 || L.first_k < S.first_k)) {
    S.first_k = L.first_k; S.first_i = L.first_i; S.first_j = L.first_j;
  }
  S.n_conf += L.n_conf; S.n_rows_conf += L.n_rows_conf;
  S.n_measured += 1;
  P.tot[0] = L;
  P.tot[1] = S;
}

namespace lqro {

size_t predict_lds_bytes(int H) { return sizeof(double) * 3 * (size_t)PR_TR * (size_t)H; }

void launch_predict_cg(hipStream_t s, const PredArgs& P) {
  hipLaunchKernelGGL(k_pred_cg, dim3((unsigned)P.nsets), dim3(256), 0, s, P);
}

void launch_predict(hipStream_t s, const PredArgs& P, hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[0], s);
  if (P.given) {
    const long n = (long)P.nc * P.H;
    hipLaunchKernelGGL(k_pred_tr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P);
  } else {
    const long n = (long)P.n_agents * P.H;
    hipLaunchKernelGGL(k_pred_paths, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P);
  }
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(k_conf, dim3((unsigned)((P.nrows + PR_TR - 1) / PR_TR)), dim3(PR_BLOCK), predict_lds_bytes(P.H), s, P);
  if (ev) (void)hipEventRecord(ev[2], s);
  if (!P.given && P.nobs > 0) hipLaunchKernelGGL(k_conf_obs, dim3((unsigned)P.nrows), dim3(64), 0, s, P);
  if (ev) (void)hipEventRecord(ev[3], s);
  hipLaunchKernelGGL(k_conf_total, dim3(1), dim3(256), 0, s, P);
  if (ev) (void)hipEventRecord(ev[4], s);
}

}  // namespace lqro
