// lqro_kern_audit.hip — the LP audit's kernels (lqro.h: lqro_set_lp_audit,
// lqro_audit_new_v): k_lp_audit, k_lp_audit_total.  An object of
// its own beside the step's kernels: it reads the plane list through the
// LpArgs the LP was launched with (lqro_kern.hpp) and evaluates it with
// lqro_lp.hpp's own vdot / vsub, so it cannot drift from what the LP reads;
// nothing in a step reads what it writes.
// Exactness: every + - * below rounds once (-ffp-contract=off), in the order
// lqro.h states, so tests/lp_audit_ref.py's numpy restatement matches bit for
// bit; maxima are (value, k) keys, counts are ballot popcounts.
#include <hip/hip_runtime.h>

#include <climits>

#include "lqro_lp.hpp"
#include "lqro_kern.hpp"

using namespace lqro;

// a running maximum with the plane that attains it
struct AuBest {
  float v;
  int k, kind, id;
};
// what a wave keeps of its row: the lanes' own maxima, the wave's counts
struct AuRow {
  AuBest all, hard;
  int n_viol, n_tol, n_hard_tol;
};

// Lane's plane (f: it has one) at list index k against the result v.  A
// lane's k ascends over the passes, so the strict > keeps the lowest k of
// equal values.  Every lane of the wave calls this (the ballots).
__device__ __forceinline__ void au_plane(AuRow& R, bool f, v3 pt, v3 nm, v3 v, float tol, int k, bool hard, int kind,
                                         int id) {
  const float viol = vdot(nm, vsub(pt, v));   // lp_violates' expression (LQRO:1083, 1138, 1170)
  if (f && viol > R.all.v) { R.all.v = viol; R.all.k = k; R.all.kind = kind; R.all.id = id; }
  if (f && hard && viol > R.hard.v) { R.hard.v = viol; R.hard.k = k; R.hard.kind = kind; R.hard.id = id; }
  R.n_viol += __popcll(__ballot(f && viol > 0.0f));
  R.n_tol += __popcll(__ballot(f && viol > tol));
  R.n_hard_tol += __popcll(__ballot(f && hard && viol > tol));
}

// the lanes' maxima as one: the larger value, of equal values the lower k
__device__ __forceinline__ AuBest au_join(AuBest b) {
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(b.v, off);
    const int ok = __shfl_xor(b.k, off), okind = __shfl_xor(b.kind, off), oid = __shfl_xor(b.id, off);
    if (ov > b.v || (ov == b.v && ok < b.k)) { b.v = ov; b.k = ok; b.kind = okind; b.id = oid; }
  }
  if (b.k == INT_MAX) b.k = b.kind = b.id = -1;   // (no plane)
  return b;
}

// the p-th emitted fence face's index 2 a + side (k_fence emits the set bits of `faces` in ascending order)
__device__ __forceinline__ int au_face(int faces, int p) {
  int face = -1;
  for (int b = 0; b < 6; ++b)
    if ((faces >> b) & 1) {
      if (p == 0) face = b;
      --p;
    }
  return face;
}

// The slots [s0, s0 + n) of a row, 64 a pass with lp_compact's two 16-byte
// loads a slot (the next pass's loads are issued before this pass is
// evaluated); list indices from the ballot's prefix counts.  Returns the list's
// length behind them.
__device__ __forceinline__ int au_slots(const LpArgs& A, const LpAuditArgs& B, AuRow& R, int lrow, int i, int s0, int n,
                                        int m, int hard_lim, v3 v, int lane) {
  const float* slots = A.slots + (size_t)lrow * A.npr * 8;
  float4 na = make_float4(0, 0, 0, 0), nb = make_float4(0, 0, 0, 0);
  if (lane < n) {
    const float4* p = reinterpret_cast<const float4*>(slots + 8 * (size_t)(s0 + lane));
    na = p[0];
    nb = p[1];
  }
  for (int base = 0; base < n; base += 64) {
    const float4 a = na, b = nb;
    const int q = s0 + base + lane;
    const bool f = base + lane < n && __float_as_int(b.z) == 1;
    if (base + 64 + lane < n) {
      const float4* p = reinterpret_cast<const float4*>(slots + 8 * (size_t)(q + 64));
      na = p[0];
      nb = p[1];
    }
    const unsigned long long bal = __ballot(f);
    const int k = m + __popcll(bal & ((1ull << lane) - 1ull));
    int kind = LQRO_AUDIT_USER, id = k;
    if (f && !B.plain) {
      const int jj = A.nbr ? A.nbr[(size_t)lrow * A.npr + q] : q;   // the slot's pair: the jj-th other column
      kind = LQRO_AUDIT_COLUMN;
      id = jj + (jj >= i ? 1 : 0);
    }
    au_plane(R, f, V3(a.x, a.y, a.z), V3(a.w, b.x, b.y), v, B.tol, k, k < hard_lim, kind, id);
    m += __popcll(bal);
  }
  return m;
}

// One wave per own row: the row's plane list as lp_row assembles it (fence,
// live user planes, the slots in LP order), streamed, never staged.  No LDS,
// no private memory, no atomics.
__global__ void __launch_bounds__(256) k_lp_audit(LpArgs A, LpAuditArgs B) {
  const int lane = threadIdx.x & 63;
  const int lrow = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (lrow >= A.nrows) return;   // (wave-uniform)
  const int i = A.row_begin + lrow * A.row_stride;
  if (A.active != nullptr && A.active[i] == 0) {   // not in this step (lqro_set_active): the cleared record
    if (lane != 0) return;
    const int ninf_bits = __float_as_int(-__builtin_huge_valf());
    int4* o = reinterpret_cast<int4*>(B.rows + lrow);
    o[0] = make_int4(ninf_bits, ninf_bits, 0, 0);
    o[1] = make_int4(i, 0, 0, 0);
    o[2] = make_int4(0, 0, -1, -1);
    o[3] = make_int4(-1, -1, -1, -1);
    return;
  }
  const v3 v = V3((float)A.newv[3 * i], (float)A.newv[3 * i + 1], (float)A.newv[3 * i + 2]);
  const v3 pref = V3((float)A.vgoal[3 * i], (float)A.vgoal[3 * i + 1], (float)A.vgoal[3 * i + 2]);
  const float ninf = -__builtin_huge_valf();
  AuRow R;
  R.all.v = ninf; R.all.k = INT_MAX; R.all.kind = -1; R.all.id = -1;
  R.hard = R.all;
  R.n_viol = R.n_tol = R.n_hard_tol = 0;
  // the head, as lp_row's: nfence fence planes, then the live user planes
  int m0 = 0, nf = 0;
  if (A.cap != A.npr) {
    const int nu = A.umax <= 0 ? 0 : A.ucounts ? max(0, min(A.ucounts[i], A.umax)) : A.umax;
    nf = A.nfence;
    m0 = nf + nu;
  }
  // the hard prefix, as lp_row's: from the level, or the row's own count
  int n_hard = A.hard >= 2 ? m0 : A.hard == 1 ? min(A.nfence, m0) : 0;
  const bool obs_ahead = A.hard >= 3 && A.obs_first >= 0;
  const int hard_row = A.nhard_rows ? A.nhard_rows[lrow] : -1;
  int hard_lim = A.nhard_rows ? hard_row : n_hard;
  for (int p0 = 0; p0 < m0; p0 += 64) {
    const int p = p0 + lane;
    const bool f = p < m0;
    v3 pt = V3(0, 0, 0), nm = V3(0, 0, 0);
    int kind = LQRO_AUDIT_USER, id = p - nf;
    if (f) {
      const float* s = p < nf ? A.fence + ((size_t)lrow * A.nfence + p) * 6 : A.uplanes + ((size_t)i * A.umax + (p - nf)) * 6;
      pt = V3(s[0], s[1], s[2]);
      nm = V3(s[3], s[4], s[5]);
      if (p < nf) { kind = LQRO_AUDIT_FENCE; id = au_face(B.faces, p); }
    }
    au_plane(R, f, pt, nm, v, B.tol, p, p < hard_lim, kind, id);
  }
  int m;
  if (obs_ahead) {
    int f = min(A.obs_first, A.npr);   // the row's first obstacle slot
    if (A.nbr) {
      f = 0;
      for (int base = 0; base < A.npr; base += 64) {
        const int q = base + lane;
        const int jj = q < A.npr ? A.nbr[(size_t)lrow * A.npr + q] : -1;
        f += __popcll(__ballot(jj >= 0 && jj < A.obs_first));
      }
    }
    n_hard = au_slots(A, B, R, lrow, i, f, A.npr - f, m0, A.nhard_rows ? hard_row : INT_MAX, v, lane);
    if (!A.nhard_rows) hard_lim = n_hard;
    m = au_slots(A, B, R, lrow, i, 0, f, n_hard, hard_lim, v, lane);
  } else {
    m = au_slots(A, B, R, lrow, i, 0, A.npr, m0, hard_lim, v, lane);
  }
  if (A.nhard_rows) n_hard = min(hard_row, m);
  const AuBest all = au_join(R.all), hard = au_join(R.hard);
  if (lane != 0) return;
  const float v2 = vdot(v, v);
  const v3 d = vsub(v, pref);
  const float dv2 = vdot(d, d);
  int4* o = reinterpret_cast<int4*>(B.rows + lrow);   // the 64-byte record as four 16-byte stores
  o[0] = make_int4(__float_as_int(all.v), __float_as_int(hard.v), __float_as_int(v2), __float_as_int(dv2));
  o[1] = make_int4(i, m, n_hard, R.n_viol);
  o[2] = make_int4(R.n_tol, R.n_hard_tol, all.k, all.kind);
  o[3] = make_int4(all.id, hard.k, hard.kind, hard.id);
}

// the larger value, then the smaller i, then the smaller k
struct AuKey {
  float v;
  int i, k, kind, id;
};
__device__ __forceinline__ bool au_key_better(const AuKey& a, const AuKey& b) {
  return a.v > b.v || (a.v == b.v && (a.i < b.i || (a.i == b.i && a.k < b.k)));
}

// One workgroup over the rows: the last total with lqro.h's tie rules, then
// folded into the since-reset total (a strictly larger maximum replaces the
// kept one, so its indices are those of the earliest audit attaining it).
__global__ void __launch_bounds__(256) k_lp_audit_total(LpArgs A, LpAuditArgs B) {
  __shared__ AuKey k_a[256], k_h[256], k_d[256];
  __shared__ long long n_rv[256], n_rh[256], n_vt[256], n_pl[256];
  const int tid = threadIdx.x;
  const float ninf = -__builtin_huge_valf();
  AuKey ka{ninf, INT_MAX, INT_MAX, -1, -1}, kh = ka, kd = ka;
  long long rv = 0, rh = 0, vt = 0, pl = 0;
  for (int lrow = tid; lrow < A.nrows; lrow += 256) {
    const lqro_lp_row R = B.rows[lrow];
    if (A.active != nullptr && A.active[R.i] == 0) continue;   // (its dv2 = 0 is no measurement)
    const AuKey a{R.viol_max, R.i, R.k_viol, R.kind_viol, R.id_viol};
    const AuKey h{R.hard_viol_max, R.i, R.k_hard, R.kind_hard, R.id_hard};
    const AuKey d{R.dv2, R.i, 0, -1, -1};
    if (au_key_better(a, ka)) ka = a;
    if (au_key_better(h, kh)) kh = h;
    if (au_key_better(d, kd)) kd = d;
    rv += R.n_viol_tol > 0 ? 1 : 0;
    rh += R.n_hard_viol > 0 ? 1 : 0;
    vt += R.n_viol_tol;
    pl += R.m;
  }
  k_a[tid] = ka; k_h[tid] = kh; k_d[tid] = kd;
  n_rv[tid] = rv; n_rh[tid] = rh; n_vt[tid] = vt; n_pl[tid] = pl;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
      if (au_key_better(k_a[tid + w], k_a[tid])) k_a[tid] = k_a[tid + w];
      if (au_key_better(k_h[tid + w], k_h[tid])) k_h[tid] = k_h[tid + w];
      if (au_key_better(k_d[tid + w], k_d[tid])) k_d[tid] = k_d[tid + w];
      n_rv[tid] += n_rv[tid + w]; n_rh[tid] += n_rh[tid + w]; n_vt[tid] += n_vt[tid + w]; n_pl[tid] += n_pl[tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  ka = k_a[0]; kh = k_h[0]; kd = k_d[0];
  if (!(ka.v > ninf)) ka.i = ka.k = ka.kind = ka.id = -1;   // (a maximum of -inf names no plane)
  if (!(kh.v > ninf)) kh.i = kh.k = kh.kind = kh.id = -1;
  if (!(kd.v > ninf)) kd.i = -1;
  lqro_lp_total L;
  L.viol_max = ka.v; L.viol_i = ka.i; L.viol_k = ka.k; L.viol_kind = ka.kind; L.viol_id = ka.id;
  L.hard_viol_max = kh.v; L.hard_i = kh.i; L.hard_k = kh.k; L.hard_kind = kh.kind; L.hard_id = kh.id;
  L.dv2_max = kd.v; L.dv2_i = kd.i;
  L.n_rows_viol = n_rv[0]; L.n_rows_hard_viol = n_rh[0]; L.n_viol_tol = n_vt[0]; L.n_planes = n_pl[0];
  L.n_measured = 1;
  lqro_lp_total S = B.tot[1];
  if (L.viol_max > S.viol_max) {
    S.viol_max = L.viol_max; S.viol_i = L.viol_i; S.viol_k = L.viol_k; S.viol_kind = L.viol_kind; S.viol_id = L.viol_id;
  }
  if (L.hard_viol_max > S.hard_viol_max) {
    S.hard_viol_max = L.hard_viol_max; S.hard_i = L.hard_i; S.hard_k = L.hard_k; S.hard_kind = L.hard_kind;
    S.hard_id = L.hard_id;
  }
  if (L.dv2_max > S.dv2_max) { S.dv2_max = L.dv2_max; S.dv2_i = L.dv2_i; }
  S.n_rows_viol += L.n_rows_viol; S.n_rows_hard_viol += L.n_rows_hard_viol; S.n_viol_tol += L.n_viol_tol;
  S.n_planes += L.n_planes;
  S.n_measured += 1;
  B.tot[0] = L;
  B.tot[1] = S;
}

namespace lqro {

void launch_lp_audit(hipStream_t s, const LpArgs& La, const LpAuditArgs& B, hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(k_lp_audit, dim3((unsigned)((La.nrows + 3) / 4)), dim3(256), 0, s, La, B);
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(k_lp_audit_total, dim3(1), dim3(256), 0, s, La, B);
  if (ev) (void)hipEventRecord(ev[2], s);
}

}  // namespace lqro
