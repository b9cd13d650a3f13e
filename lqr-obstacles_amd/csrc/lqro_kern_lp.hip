// lqro_kern_lp.hip — the kernels around the pair loop that are not its own:
// k_tables (the horizon tables, once per set of gains), the LP kernels k_lp,
// k_lp_lds and k_lp4 (lqro_lp.hpp), k_copy_claimed and k_fence, with their
// launch functions (lqro_kern.hpp).
#include <hip/hip_runtime.h>

#include "lqro_device.hpp"
#include "lqro_lp.hpp"
#include "lqro_kern.hpp"

using namespace lqro;

#define LQRO_MAXX 16
// Horizon tables (per agent): T_k = !(C*G_k) (3x3), NCF_k = (-C)*F_k (3xX),
// with F_k, G_k from findFG iterated from F=I, G=0.  One workgroup per agent;
// thread (r, c) owns entry (r, c) of the X x X recursion.
__global__ void __launch_bounds__(256) k_tables(int X, int U, int H, const double* __restrict__ A,
                                                const double* __restrict__ B,
                                                const double* __restrict__ L,
                                                const double* __restrict__ E, int per_agent,
                                                double* __restrict__ Tout,
                                                double* __restrict__ Nout,
                                                double* __restrict__ Rout,
                                                double* __restrict__ TFout, double rad0,
                                                double rad1, double rad2, double umax,
                                                int* __restrict__ err) {
  __shared__ double sAt[LQRO_MAXX * LQRO_MAXX], sBt[LQRO_MAXX * 3];
  __shared__ double sF[LQRO_MAXX * LQRO_MAXX], sG[LQRO_MAXX * 3];
  __shared__ double sFn[LQRO_MAXX * LQRO_MAXX], sGn[LQRO_MAXX * 3];
  __shared__ double sA[LQRO_MAXX * LQRO_MAXX], sB[LQRO_MAXX * 4], sL[4 * LQRO_MAXX], sE[4 * 3];
  const int agent = blockIdx.x;
  const double* Li = L + (per_agent ? (size_t)agent * U * X : 0);
  const double* Ei = E + (per_agent ? (size_t)agent * U * 3 : 0);
  const int t = threadIdx.x;
  for (int q = t; q < X * X; q += blockDim.x) sA[q] = A[q];
  for (int q = t; q < X * U; q += blockDim.x) sB[q] = B[q];
  for (int q = t; q < U * X; q += blockDim.x) sL[q] = Li[q];
  for (int q = t; q < U * 3; q += blockDim.x) sE[q] = Ei[q];
  __syncthreads();
  const int r = t / X, c = t % X;
  const bool act = t < X * X;
  if (act) {
    // Atilde = A + (B*L), Btilde = B*E   (LQRObstacles.cpp:725-728)
    double bl = 0.0;
    for (int k = 0; k < U; ++k) bl += sB[r * U + k] * sL[k * X + c];
    sAt[r * X + c] = sA[r * X + c] + bl;
    if (c < 3) {
      double be = 0.0;
      for (int k = 0; k < U; ++k) be += sB[r * U + k] * sE[k * 3 + c];
      sBt[r * 3 + c] = be;
    }
    sF[r * X + c] = (r == c) ? 1.0 : 0.0;   // Ft = identity (:1401)
    if (c < 3) sG[r * 3 + c] = 0.0;          // Gt = zeros   (:1402)
  }
  __syncthreads();
  double* Ta = Tout + (size_t)agent * H * 9;
  double* Na = Nout + (size_t)agent * H * 3 * X;
  for (int k = 0; k < H; ++k) {
    if (act) {
      double f = 0.0;
      for (int m = 0; m < X; ++m) f += sAt[r * X + m] * sF[m * X + c];
      sFn[r * X + c] = f;
      if (c < 3) {
        double g = 0.0;
        for (int m = 0; m < X; ++m) g += sAt[r * X + m] * sG[m * 3 + c];
        sGn[r * 3 + c] = g + sBt[r * 3 + c];
      }
    }
    __syncthreads();
    if (act) {
      sF[r * X + c] = sFn[r * X + c];
      if (c < 3) sG[r * 3 + c] = sGn[r * 3 + c];
    }
    __syncthreads();
    // NCF_k = (-C)*F_k, entries of -C are -1.0 / -0.0 (:773)
    if (t < 3 * X) {
      const int rr = t / X, cc = t % X;
      double s = 0.0;
      for (int m = 0; m < X; ++m) {
        double nc = (m == rr) ? -1.0 : -0.0;
        s += nc * sF[m * X + cc];
      }
      Na[(size_t)k * 3 * X + rr * X + cc] = s;
    }
    if (t == 0) {
      // T_k = !(C*G_k)  (:771)
      double cg[9], inv[9];
      for (int rr = 0; rr < 3; ++rr)
        for (int cc = 0; cc < 3; ++cc) {
          double s = 0.0;
          for (int m = 0; m < X; ++m) s += ((m == rr) ? 1.0 : 0.0) * sG[m * 3 + cc];
          cg[rr * 3 + cc] = s;
        }
      inverse3(cg, inv);
      for (int q = 0; q < 9; ++q) {
        Ta[(size_t)k * 9 + q] = inv[q];
        if (!isfinite(inv[q])) atomicOr(err, 1);
      }
      // slice bounds for k_pair: |T_k s_p| <= ||T_k diag(rad)||_F * max|u_p|
      const double rad[3] = {rad0, rad1, rad2};
      double fr = 0.0, ff = 0.0;
      for (int rr = 0; rr < 3; ++rr)
        for (int cc = 0; cc < 3; ++cc) {
          const double tv = inv[rr * 3 + cc];
          fr += (tv * rad[cc]) * (tv * rad[cc]);
          ff += tv * tv;
        }
      Rout[(size_t)agent * H + k] = sqrt(fr) * umax * (1.0 + 1e-12);
      TFout[(size_t)agent * H + k] = sqrt(ff);
    }
    __syncthreads();
  }
}

// LP kernels: one wavefront per row agent (lqro_lp.hpp), fp32 as the reference.
// one row's LP; `planes` holds its compacted plane list (stride PS floats:
// 6 in LDS, 8 in global memory)
template <int PS>
__device__ __forceinline__ void lp_row(const LpArgs& A, int lrow, float* planes, int lane) {
  const int i = A.row_begin + lrow * A.row_stride;
  if (A.active != nullptr && A.active[i] == 0) {   // not in this step (lqro_set_active): no LP, newV = +0.0
    if (lane == 0) {
      A.newv[3 * i] = 0.0;
      A.newv[3 * i + 1] = 0.0;
      A.newv[3 * i + 2] = 0.0;
    }
    return;
  }
  int m0 = 0;
  if (A.cap != A.npr) {
    const int nu = A.umax <= 0 ? 0 : A.ucounts ? max(0, min(A.ucounts[i], A.umax)) : A.umax;
    lp_head<PS>(A.fence + (size_t)lrow * A.nfence * 6, A.nfence, A.uplanes + (size_t)i * A.umax * 6, nu, planes,
                lane);
    m0 = A.nfence + nu;
  }
  // the hard prefix (LpArgs::hard): fence planes, live user planes, and at
  // level 3 the obstacle slots' planes, compacted ahead of the agent slots'
  int n_hard = A.hard >= 2 ? m0 : A.hard == 1 ? min(A.nfence, m0) : 0;
  const float* slots = A.slots + (size_t)lrow * A.npr * 8;
  int m;
  if (A.hard >= 3 && A.obs_first >= 0) {
    int f = min(A.obs_first, A.npr);   // the row's first obstacle slot
    if (A.nbr) {
      f = 0;
      for (int base = 0; base < A.npr; base += 64) {
        const int q = base + lane;
        const int jj = q < A.npr ? A.nbr[(size_t)lrow * A.npr + q] : -1;
        f += __popcll(__ballot(jj >= 0 && jj < A.obs_first));
      }
    }
    n_hard = lp_compact<PS>(slots + 8 * (size_t)f, A.npr - f, planes, lane, m0);
    m = lp_compact<PS>(slots, f, planes, lane, n_hard);
  } else {
    m = lp_compact<PS>(slots, A.npr, planes, lane, m0);
  }
  if (A.nhard_rows) n_hard = min(A.nhard_rows[lrow], m);
  const v3 pref = V3((float)A.vgoal[3 * i], (float)A.vgoal[3 * i + 1], (float)A.vgoal[3 * i + 2]);
  v3 nv = V3(0.0f, 0.0f, 0.0f);
  const int fail = w_lp3<PS>(planes, m, A.vmax, pref, false, nv, lane);          // :1228
#ifdef LQRO_LP_PROFILE
  int lp4_iters = 0;
  if (fail < m)
    w_lp4<PS, true>(planes, m, fail, (float)A.vmax, nv, A.proj + (size_t)lrow * A.cap * PS, lane, lp4_iters, n_hard);
  if (lane == 0 && A.prof && lrow < 4096) A.prof[32 + 4096 + lrow] = ((unsigned long long)m << 40) |
                                               ((unsigned long long)fail << 20) | (unsigned)lp4_iters;
#else
  if (fail < m && A.lp4_list != nullptr) {
    // linearProgram4 (:1230) in k_lp4, with its projected planes in LDS too:
    // hand over the compacted planes (stride PS) and linearProgram3's result
    float* dst = A.compact + (size_t)lrow * A.cap * 8;
    if (dst != planes)
      for (int q = lane; q < PS * m; q += 64) dst[q] = planes[q];
    if (lane == 0) {
      const int k = atomicAdd(A.lp4_count, 1);
      int* e = A.lp4_list + 8 * (size_t)k;
      e[0] = lrow; e[1] = fail; e[2] = m;
      e[3] = __float_as_int(nv.x); e[4] = __float_as_int(nv.y); e[5] = __float_as_int(nv.z);
      e[6] = n_hard; e[7] = 0;
    }
    return;
  }
  if (fail < m)
    w_lp4<PS, true>(planes, m, fail, (float)A.vmax, nv, A.proj + (size_t)lrow * A.cap * PS, lane, n_hard);  // :1230
#endif
  if (lane == 0) {
    A.newv[3 * i] = nv.x;
    A.newv[3 * i + 1] = nv.y;
    A.newv[3 * i + 2] = nv.z;
  }
}

// plane list in global scratch (rows with more planes than LDS holds)
__global__ void __launch_bounds__(256) k_lp(LpArgs A) {
  const int lane = threadIdx.x & 63;
  const int lrow = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (lrow >= A.nrows) return;
  lp_row<8>(A, lrow, A.compact + (size_t)lrow * A.cap * 8, lane);
}

// one wave per workgroup, the row's plane list in LDS (the LP rescans it for
// every violated plane: LDS round trips instead of L2 ones), 32 B a plane
// (16-B aligned loads) up to 2,048 planes, 24 B beyond (C4: 4,095)
template <int PS>
__global__ void __launch_bounds__(64) k_lp_lds(LpArgs A) {
  extern __shared__ float lp_planes[];
  const int lrow = blockIdx.x;
  if (lrow >= A.nrows) return;
  if (A.rowclaim) {
    int go;
    if (A.mode == 1) {
      go = 0;
      if (threadIdx.x == 0)
        go = __hip_atomic_load(A.rowpend + lrow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.row_target &&
             atomicCAS(A.rowclaim + lrow, 0, 1) == 0;
      go = __builtin_amdgcn_readfirstlane(go);
      __threadfence();   // the row's planes (acquire)
    } else {
      go = A.rowclaim[lrow] != 1;
    }
    if (!go) return;
  }
#ifdef LQRO_LP_PROFILE
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  lp_row<PS>(A, lrow, lp_planes, threadIdx.x);
#ifdef LQRO_LP_PROFILE
  if (threadIdx.x == 0 && lrow < 8192) A.prof[32 + lrow] = __builtin_amdgcn_s_memtime() - t0;
#endif
}

// linearProgram4 for the rows k_lp_lds listed (one wave per row): the planes
// in LDS, and their projections too when both fit (else the projections in
// global memory), so the O(m^2) rescans of linearProgram4's inner
// linearProgram3 stay out of L2
template <int PS>
__global__ void __launch_bounds__(64) k_lp4(LpArgs A, int proj_in_lds) {
  extern __shared__ float lp4_sm[];
  float* planes = lp4_sm;
  const int lane = threadIdx.x;
  {
    // one workgroup per listed row (a persistent loop over the list around
    // these ballot-driven loops hung on gfx950; the extra workgroups exit at once)
    const int job = blockIdx.x;
    if (job >= *A.lp4_count) return;
    const int* e = A.lp4_list + 8 * (size_t)job;
    const int lrow = e[0], fail = e[1], m = e[2], n_hard = e[6];
    float* proj = proj_in_lds ? lp4_sm + (size_t)A.cap * PS : A.proj + (size_t)lrow * A.cap * PS;
    v3 nv = V3(__int_as_float(e[3]), __int_as_float(e[4]), __int_as_float(e[5]));
    const float* src = A.compact + (size_t)lrow * A.cap * 8;
    for (int q = lane; q < PS * m; q += 64) planes[q] = src[q];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#ifdef LQRO_LP_PROFILE
    int lp4_iters = 0;
    w_lp4<PS, true>(planes, m, fail, (float)A.vmax, nv, proj, lane, lp4_iters, n_hard);  // :1230
#else
    w_lp4<PS, true>(planes, m, fail, (float)A.vmax, nv, proj, lane, n_hard);              // :1230
#endif
    if (lane == 0) {
      const int i = A.row_begin + lrow * A.row_stride;
      A.newv[3 * i] = nv.x;
      A.newv[3 * i + 1] = nv.y;
      A.newv[3 * i + 2] = nv.z;
    }
  }
}

// lqro_step_device_end after an early LP in _begin: the rows it ran (claimed
// 1) have their newV in the context's buffer; the tail wrote the others
__global__ void __launch_bounds__(256) k_copy_claimed(const int* rowclaim, int nrows, int rb, int rs,
                                                      const double* src, double* dst) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows || rowclaim[r] != 1) return;
  const size_t i = (size_t)rb + (size_t)r * rs;
  dst[3 * i] = src[3 * i];
  dst[3 * i + 1] = src[3 * i + 1];
  dst[3 * i + 2] = src[3 * i + 2];
}

__global__ void __launch_bounds__(256) k_fence(FenceArgs F) {
  const int lrow = blockIdx.x * blockDim.x + threadIdx.x;
  if (lrow >= F.nrows) return;
  const size_t i = (size_t)F.row_begin + (size_t)lrow * F.row_stride;
  float* o = F.out + (size_t)lrow * F.nfence * 6;
  for (int a = 0; a < 3; ++a) {
    const double p = F.x[i * F.X + a];
    for (int side = 0; side < 2; ++side) {
      if (!((F.faces >> (2 * a + side)) & 1)) continue;
      const double b = side == 0 ? ((F.lo[a] + F.m[a]) - p) / F.tau : ((F.hi[a] - F.m[a]) - p) / F.tau;
      for (int q = 0; q < 6; ++q) o[q] = 0.0f;
      o[a] = (float)b;
      o[3 + a] = side == 0 ? 1.0f : -1.0f;
      o += 6;
    }
  }
}
// The obstacle classes' slice bounds (lqro_set_obstacles[_ex] with shapes of
// their own): k_tables' R with each class's semi-axes and max |u_p| (osc, 4
// a class), from the T it left.  Ro is (class, agent of n_agents, k); the
// first n_gains agents of a class are written.
__global__ void __launch_bounds__(256) k_obs_rtab(int n, int per_cls, int cls_pitch, const double* __restrict__ T,
                                                  const double* __restrict__ osc, double* __restrict__ Ro) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;   // (class, agent, k)
  if (q >= n) return;
  const int c = q / per_cls, ak = q - c * per_cls;
  const double* inv = T + (size_t)ak * 9;
  const double rad[3] = {osc[4 * c], osc[4 * c + 1], osc[4 * c + 2]};
  const double umax = osc[4 * c + 3];
  double fr = 0.0;
  for (int rr = 0; rr < 3; ++rr)
    for (int cc = 0; cc < 3; ++cc) {
      const double tv = inv[rr * 3 + cc];
      fr += (tv * rad[cc]) * (tv * rad[cc]);
    }
  Ro[(size_t)c * cls_pitch + ak] = sqrt(fr) * umax * (1.0 + 1e-12);
}

// The step's columns in one array: the agents' states, then the obstacles'
// (the kernels address column j at x + j X).
__global__ void __launch_bounds__(256) k_cols(const double* __restrict__ x, size_t nx,
                                              const double* __restrict__ obs, size_t nobs,
                                              double* __restrict__ cols) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nx) cols[q] = x[q];
  else if (q < nx + nobs) cols[q] = obs[q - nx];
}

namespace lqro {

void launch_obs_rtab(hipStream_t s, int n_cls, int n_gains, int n_agents, int H, const double* T, const double* osc,
                     double* Ro) {
  const int n = n_cls * n_gains * H;
  hipLaunchKernelGGL(k_obs_rtab, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, n_gains * H, n_agents * H, T, osc,
                     Ro);
}

void launch_cols(hipStream_t s, const double* x, size_t nx, const double* obs, size_t nobs, double* cols) {
  hipLaunchKernelGGL(k_cols, dim3((unsigned)((nx + nobs + 255) / 256)), dim3(256), 0, s, x, nx, obs, nobs, cols);
}

void launch_tables(hipStream_t s, int n_gains, int X, int U, int H, const double* A, const double* B, const double* L,
                   const double* E, int per_agent, double* T, double* NCF, double* R, double* TF, double rad0,
                   double rad1, double rad2, double umax, int* err) {
  hipLaunchKernelGGL(k_tables, dim3((unsigned)n_gains), dim3(256), 0, s, X, U, H, A, B, L, E, per_agent, T, NCF, R, TF,
                     rad0, rad1, rad2, umax, err);
}

template <int PS>
static hipError_t launch_lp_lds(LpArgs La, hipStream_t s) {
  const size_t lds = (size_t)La.cap * 4 * PS;
  hipError_t e = hipFuncSetAttribute((const void*)k_lp_lds<PS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kLpLdsMax);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_lp_lds<PS>, dim3((unsigned)La.nrows), dim3(64), lds, s, La);
  e = hipGetLastError();
  if (e != hipSuccess || La.lp4_list == nullptr) return e;
  e = hipFuncSetAttribute((const void*)k_lp4<PS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLpLdsMax);
  if (e != hipSuccess) return e;
  const int proj_in_lds = 2 * lds <= kLpLdsMax;
  hipLaunchKernelGGL(k_lp4<PS>, dim3((unsigned)La.nrows), dim3(64), proj_in_lds ? 2 * lds : lds, s, La,
                     proj_in_lds);
  return hipGetLastError();
}

hipError_t launch_lp(LpArgs La, hipStream_t s, bool early) {
  if (early || (size_t)La.cap * 32 <= 64 * 1024) return launch_lp_lds<8>(La, s);
  if ((size_t)La.cap * 24 <= kLpLdsMax) return launch_lp_lds<6>(La, s);
  La.lp4_list = nullptr;
  hipLaunchKernelGGL(k_lp, dim3((unsigned)((La.nrows + 3) / 4)), dim3(256), 0, s, La);
  return hipGetLastError();
}

void launch_copy_claimed(hipStream_t s, const int* rowclaim, int nrows, int row_begin, int row_stride,
                         const double* src, double* dst) {
  hipLaunchKernelGGL(k_copy_claimed, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, rowclaim, nrows,
                     row_begin, row_stride, src, dst);
}

void launch_fence(hipStream_t s, const FenceArgs& F) {
  hipLaunchKernelGGL(k_fence, dim3((unsigned)((F.nrows + 255) / 256)), dim3(256), 0, s, F);
}

}  // namespace lqro
