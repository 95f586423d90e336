// gpx_mean.h — the parametric mean functions (gpx_mean_spec: Constant, Linear, Polynomial) and
// their coefficient derivatives, for host and device code alike.
//
// One evaluation order, every product and sum rounded on its own (no FMA contraction), powers by
// repeated multiplication (no pow): the residual kernel, the prediction kernel, the gradient kernel
// and a host caller all see the same bits for the same (x, β).
//   CONSTANT    m = c
//   LINEAR      m = ((x_0 A_0 + x_1 A_1) + ...) + b          β = [A_0 .. A_{D-1}, b]
//   POLYNOMIAL  m = ((w_0 + w_1 x) + w_2 x²) + ...,  x^k = x^(k-1) · x     β = [w_0 .. w_degree]
#pragma once
#include "../../include/gpx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPX_HD __host__ __device__ __forceinline__
#else
#define GPX_HD inline
#endif

namespace gpx {

constexpr int kMeanMaxDegree = 4;
constexpr int kMeanMaxCoef = GPX_THETA_STRIDE - 2;  // at least one kernel parameter and the noise slot

// per-slot mean as the kernels read it: the spec and the θ-row column of its first coefficient
struct DevMean {
  int kind, degree, n_coef, off;
};

// m(x; β): x the point's D inputs, beta the slot's n_coef coefficients
GPX_HD double mean_eval(int kind, int n_coef, const double* beta, const double* x, int D) {
#pragma clang fp contract(off)
  switch (kind) {
    case GPX_MEAN_CONSTANT:
      return beta[0];
    case GPX_MEAN_LINEAR: {
      double s = x[0] * beta[0];
      for (int d = 1; d < D; ++d) s = s + x[d] * beta[d];
      return s + beta[D];
    }
    case GPX_MEAN_POLYNOMIAL: {
      double p = 1.0, s = beta[0];
      for (int k = 1; k < n_coef; ++k) {
        p = p * x[0];
        s = s + beta[k] * p;
      }
      return s;
    }
    default:
      return 0.0;
  }
}

// ∂m(x)/∂β_k for coefficient k < n_coef (the powers formed as mean_eval forms them)
GPX_HD double mean_dcoef(int kind, int k, const double* x, int D) {
#pragma clang fp contract(off)
  switch (kind) {
    case GPX_MEAN_LINEAR:
      return k < D ? x[k] : 1.0;
    case GPX_MEAN_POLYNOMIAL: {
      double p = 1.0;
      for (int i = 0; i < k; ++i) p = p * x[0];
      return p;
    }
    default:
      return 1.0;
  }
}

}  // namespace gpx
