// gpx_ard.hip — the dense route's kernels for specs with ARD terms (GPX_TERM_ARD, gpx_kfun_ard.h):
// the K / cross-covariance build and prediction's k**. The ARD gradient contraction is an epilogue
// of the fused K⁻¹ = WᵀW GEMM (gpx_kernels.hip, EPI_CONTRACT_ARD*). The host sends a call's ARD
// problems here and its isotropic ones to the kernels of gpx_kernels.hip (gpx_dense.hip,
// gpx_predict.hip): which kernel evaluates a slot is a property of the slot's spec.
#include <hip/hip_runtime.h>
#include "gpx_internal.h"
#include "gpx_kfun_ard.h"

namespace gpx {

// build_kernel's tile geometry and padding; every stationary term's rows staged over its ℓ (ℓ_d
// for an ARD term), term t's at soff[t]: the tile's 64 rows then its 64 columns.
__global__ __launch_bounds__(256) void build_ard_kernel(BuildArgs a) {
  const int b = a.active[blockIdx.y];
  int ti, tj;
  if (a.symmetric) {
    // lower tiles, row-major
    int t = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((t + 1) * (t + 2) / 2 <= (int)blockIdx.x) ++t;
    while (t * (t + 1) / 2 > (int)blockIdx.x) --t;
    ti = t;
    tj = blockIdx.x - t * (t + 1) / 2;
  } else {
    const int ntj = a.cols / 64;
    ti = blockIdx.x / ntj;
    tj = blockIdx.x - ti * ntj;
  }
  __shared__ double sxp[128 * GPX_MAX_DIM];  // scaled rows, then (Linear / Periodic terms) raw rows
  __shared__ double sth[GPX_THETA_STRIDE];
  __shared__ int soff[GPX_MAX_TERMS];
  const int D = a.D, tid = threadIdx.x;
  const int n = a.rows_valid > 0 ? a.rows_valid : a.nvalid[b];
  const int ncol = a.symmetric ? n : a.m2;
  const double* X = a.X + (long long)b * a.sX;
  const double* X2 = a.symmetric ? X : a.X2 + (long long)b * a.sX2;
  const DevSpec spec = a.specs[b];
  const DevSpec* gs = a.specs + b;  // (dynamic term index: read from memory, not the register copy)
  const double* th = a.theta + b * GPX_THETA_STRIDE;
  int P = 0;
  bool raw = false;
  for (int t = 0; t < gs->n_terms; ++t) {
    if (ard_prescaled(gs->terms[t])) P += gs->terms[t].dim_count;
    else raw = true;
  }
  const int Dr = raw ? D : 0;
  const bool fits = P + Dr <= GPX_MAX_DIM;  // (refused at create / rebind otherwise)
  if (tid == 0) {
    int o = 0;
    for (int t = 0; t < GPX_MAX_TERMS; ++t) {
      const bool pre = t < gs->n_terms && ard_prescaled(gs->terms[t]);
      soff[t] = 128 * o;
      o += pre ? gs->terms[t].dim_count : 0;
    }
  }
  if (tid < GPX_THETA_STRIDE) sth[tid] = th[tid];
  double* sxr = sxp + 128 * P;
  if (fits) {
    for (int t = 0, o = 0; t < gs->n_terms; ++t) {
      const gpx_term& tm = gs->terms[t];
      if (!ard_prescaled(tm)) continue;
      const int dn = tm.dim_count, e0 = ard_ell_slot(tm);
      const bool vec = ard_on(tm);
      for (int e = tid; e < 64 * dn; e += 256) {
        const int r = e / dn, dd = e - r * dn, d = tm.dim_start + dd;
        const double ell = th[e0 + (vec ? dd : 0)];
        const int gi = ti * 64 + r, gj = tj * 64 + r;
        sxp[128 * o + e] = (gi < n ? X[(long long)gi * D + d] : 0.0) / ell;
        sxp[128 * o + 64 * dn + e] = (gj < ncol ? X2[(long long)gj * D + d] : 0.0) / ell;
      }
      o += dn;
    }
    for (int e = tid; e < 64 * Dr; e += 256) {
      const int r = e / Dr, d = e - r * Dr;
      const int gi = ti * 64 + r, gj = tj * 64 + r;
      sxr[e] = gi < n ? X[(long long)gi * D + d] : 0.0;
      sxr[64 * Dr + e] = gj < ncol ? X2[(long long)gj * D + d] : 0.0;
    }
  }
  __syncthreads();
  const double noise = sth[spec.n_params];
  double* out = a.out + (long long)b * a.sOut;
  const int c = tid & 63;
  const int gj = tj * 64 + c;
#pragma unroll 1
  for (int q = 0; q < 16; ++q) {
    const int r = (tid >> 6) + 4 * q;
    const int gi = ti * 64 + r;
    double v;
    const bool valid = fits && gi < n && gj < ncol;
    if (valid) {
      v = ard_eval_k(spec, sth, sxr + r * Dr, sxr + (64 + c) * Dr, sxp, soff, r, 64 + c);
      if (a.symmetric && gi == gj) v += noise;
    } else {
      v = (a.symmetric && gi == gj) ? 1.0 : 0.0;
    }
    out[(long long)gi * a.ldo + gj] = v;
  }
}

void launch_build_ard(const BuildArgs& a, int n_active, hipStream_t s) {
  const int ti = a.rows / 64, tj = a.cols / 64;
  const int ntiles = a.symmetric ? ti * (ti + 1) / 2 : ti * tj;
  hipLaunchKernelGGL(build_ard_kernel, dim3(ntiles, n_active), dim3(256), 0, s, a);
}

// var_j = k(x*_j, x*_j) − Σ_rowtiles colsum partials (+ σn² for predict_y): predvar_kernel's, with
// the σ² of an ARD term read at its own θ slot
__global__ __launch_bounds__(256) void predvar_ard_kernel(PredVarArgs a) {
  const int b = a.active[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.M) return;
  const DevSpec* gs = a.specs + b;
  const double* th = a.theta + b * GPX_THETA_STRIDE;
  const double* x = a.Xnew + (long long)b * a.sXnew + (long long)j * a.D;
  const double kss = ard_eval_kdiag(*gs, th, x);
  const double* part = a.partial + (long long)b * a.sPartial;
  double s = 0.0;
  for (int t = 0; t < a.nrowtiles; ++t) s += part[(long long)t * a.ldp + j];
  double v = kss - s;
  if (a.add_noise) v += th[gs->n_params];
  a.var[(long long)b * a.sVar + j] = v;
}

void launch_predvar_ard(const PredVarArgs& a, int n_active, hipStream_t s) {
  hipLaunchKernelGGL(predvar_ard_kernel, dim3((a.M + 255) / 256, n_active), dim3(256), 0, s, a);
}

}  // namespace gpx
