// gpx_coregion.hip — the dense route's kernels for specs with a Coregion term (GPX_COREGION,
// gpx_kfun_coreg.h): the K / cross-covariance build and prediction's k**. The gradient contraction
// is an epilogue of the fused K⁻¹ = WᵀW GEMM (gpx_kernels.hip, EPI_CONTRACT_COREG). The host orders
// a call's Coregion problems behind its isotropic and ARD ones and sends them here (gpx_dense.hip,
// gpx_predict.hip): which kernel evaluates a slot is a property of the slot's spec.
#include <hip/hip_runtime.h>
#include "gpx_internal.h"
#include "gpx_kfun_coreg.h"

namespace gpx {

// build_ard_kernel's tile geometry, padding and staging of the partner terms' rows; B = W Wᵀ + diag(κ)
// formed once per workgroup, the tile's row and column output indices read once and clamped.
__global__ __launch_bounds__(256) void build_coreg_kernel(BuildArgs a) {
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
  __shared__ double sB[kCoregMaxP * kCoregMaxP];
  __shared__ int sidx[128];                  // output index of the tile's 64 rows, then its 64 columns
  __shared__ int soff[GPX_MAX_TERMS];
  const int D = a.D, tid = threadIdx.x;
  const int n = a.rows_valid > 0 ? a.rows_valid : a.nvalid[b];
  const int ncol = a.symmetric ? n : a.m2;
  const double* X = a.X + (long long)b * a.sX;
  const double* X2 = a.symmetric ? X : a.X2 + (long long)b * a.sX2;
  const DevSpec spec = a.specs[b];
  const DevSpec* gs = a.specs + b;  // (dynamic term index: read from memory, not the register copy)
  const double* th = a.theta + b * GPX_THETA_STRIDE;
  const int P = cg_P(spec), R = cg_R(spec);
  int S = 0, tc = -1;
  bool raw = false;
  for (int t = 0; t < gs->n_terms; ++t) {
    if (cg_is(gs->terms[t])) tc = t;
    else if (ard_prescaled(gs->terms[t])) S += gs->terms[t].dim_count;
    else raw = true;
  }
  const int Dr = raw ? D : 0;
  // (refused at create / rebind otherwise)
  const bool fits = S + Dr <= GPX_MAX_DIM && tc >= 0 && P >= 1 && P <= kCoregMaxP && R >= 1 &&
                    gs->terms[tc < 0 ? 0 : tc].param_offset + P * R + P <= spec.n_params;
  if (tid == 0) {
    int o = 0;
    for (int t = 0; t < GPX_MAX_TERMS; ++t) {
      const bool pre = t < gs->n_terms && cg_prescaled(gs->terms[t]);
      soff[t] = 128 * o;
      o += pre ? gs->terms[t].dim_count : 0;
    }
  }
  if (tid < GPX_THETA_STRIDE) sth[tid] = th[tid];
  double* sxr = sxp + 128 * S;
  if (fits) {
    const gpx_term& ct = gs->terms[tc];
    if (tid < P * P) {
      const int p = tid / P, q = tid - p * P;
      sB[p * kCoregMaxP + q] = cg_b(th + ct.param_offset, P, R, p, q);
    }
    if (tid >= 64 && tid < 128) {
      const int r = tid - 64, gi = ti * 64 + r;
      sidx[r] = gi < n ? cg_index(X[(long long)gi * D + ct.dim_start], P) : 0;
    } else if (tid >= 128 && tid < 192) {
      const int r = tid - 128, gj = tj * 64 + r;
      sidx[64 + r] = gj < ncol ? cg_index(X2[(long long)gj * D + ct.dim_start], P) : 0;
    }
    for (int t = 0, o = 0; t < gs->n_terms; ++t) {
      const gpx_term& tm = gs->terms[t];
      if (!cg_prescaled(tm)) continue;
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
      v = cg_eval_k(spec, sth, sxr + r * Dr, sxr + (64 + c) * Dr, sxp, soff, r, 64 + c, sB, sidx[r],
                    sidx[64 + c]);
      if (a.symmetric && gi == gj) v += noise;
    } else {
      v = (a.symmetric && gi == gj) ? 1.0 : 0.0;
    }
    out[(long long)gi * a.ldo + gj] = v;
  }
}

void launch_build_coreg(const BuildArgs& a, int n_active, hipStream_t s) {
  const int ti = a.rows / 64, tj = a.cols / 64;
  const int ntiles = a.symmetric ? ti * (ti + 1) / 2 : ti * tj;
  hipLaunchKernelGGL(build_coreg_kernel, dim3(ntiles, n_active), dim3(256), 0, s, a);
}

// var_j = k(x*_j, x*_j) − Σ_rowtiles colsum partials (+ σn² for predict_y): predvar_kernel's, with
// k** the partners' K_diag times B[a_j][a_j]
__global__ __launch_bounds__(256) void predvar_coreg_kernel(PredVarArgs a) {
  const int b = a.active[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.M) return;
  const DevSpec* gs = a.specs + b;
  const double* th = a.theta + b * GPX_THETA_STRIDE;
  const double* x = a.Xnew + (long long)b * a.sXnew + (long long)j * a.D;
  const int P = cg_P(*gs), R = cg_R(*gs);
  // (a spec the create / rebind checks would have refused: no read outside the θ row)
  const bool ok = P >= 1 && P <= kCoregMaxP && R >= 1 && P * R + P <= gs->n_params;
  const double kss = ok ? cg_eval_kdiag(*gs, th, x) : 0.0;
  const double* part = a.partial + (long long)b * a.sPartial;
  double s = 0.0;
  for (int t = 0; t < a.nrowtiles; ++t) s += part[(long long)t * a.ldp + j];
  double v = kss - s;
  if (a.add_noise) v += th[gs->n_params];
  a.var[(long long)b * a.sVar + j] = v;
}

void launch_predvar_coreg(const PredVarArgs& a, int n_active, hipStream_t s) {
  hipLaunchKernelGGL(predvar_coreg_kernel, dim3((a.M + 255) / 256, n_active), dim3(256), 0, s, a);
}

}  // namespace gpx
