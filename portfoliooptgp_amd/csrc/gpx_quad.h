// gpx_quad.h — the per-row variational expectation shared by the VGP and SVGP quadrature kernels
// (vgp_quad_kernel, svgp_lik_quad_kernel): closed form for the Gaussian likelihood, GPflow's
// 20-point Gauss–Hermite rule for Student-t. One table, one arithmetic; device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "gpx_internal.h"

namespace gpx {

// numpy.polynomial.hermite.hermgauss(20): nodes x_i and weights w_i (GPflow's NDiagGHQuadrature
// divides the weights by √π and evaluates at μ + √(2v) x_i)
static __constant__ double kGhX[kGhPoints] = {
    -5.3874808900112328, -4.6036824495507442, -3.9447640401156252, -3.3478545673832163,
    -2.7888060584281305, -2.2549740020892757, -1.7385377121165861, -1.2340762153953231,
    -0.73747372854539439, -0.24534070830090124, 0.24534070830090124, 0.73747372854539439,
    1.2340762153953231, 1.7385377121165861, 2.2549740020892757, 2.7888060584281305,
    3.3478545673832163, 3.9447640401156252, 4.6036824495507442, 5.3874808900112328};
static __constant__ double kGhW[kGhPoints] = {
    2.2293936455341447e-13, 4.3993409922731747e-10, 1.0860693707692782e-07, 7.8025564785320599e-06,
    0.00022833863601635365, 0.0032437733422378567, 0.024810520887463643, 0.10901720602002329,
    0.28667550536283415, 0.46224366960061009, 0.46224366960061009, 0.28667550536283415,
    0.10901720602002329, 0.024810520887463643, 0.0032437733422378567, 0.00022833863601635365,
    7.8025564785320599e-06, 1.0860693707692782e-07, 4.3993409922731747e-10, 2.2293936455341447e-13};
constexpr double kInvSqrtPi = 0.56418958354775628;  // 1/√π

// ve(μ, v, y) of one row and its derivatives: E = ve, gm = ∂ve/∂μ, gv = ∂ve/∂v, gphi = ∂ve/∂φ
// (φ: the Gaussian variance or the Student-t scale). c0 is the likelihood's constant: −½ log 2π,
// or lgamma((df+1)/2) − lgamma(df/2) − ½(log df + log π). The Student-t branch divides by √(2v):
// the caller keeps rows with v = 0 (padding) away from it.
__device__ __forceinline__ void ve_row(int lik, double phi, double df, double c0, double mu, double v,
                                       double y, double& E, double& gm, double& gv, double& gphi) {
  if (lik == GPX_LIK_GAUSSIAN) {
    const double s = phi, r = y - mu, q = fma(r, r, v);
    E = c0 - 0.5 * log(s) - q / (2.0 * s);
    gm = r / s;
    gv = -0.5 / s;
    gphi = -0.5 / s + q / (2.0 * s * s);
  } else {
    const double sc = phi, sd = sqrt(2.0 * v), isd = 1.0 / sd;
    const double s2df = sc * sc * df, lsc = log(sc);
    E = 0.0;
    gm = 0.0;
    gv = 0.0;
    gphi = 0.0;
#pragma unroll 4
    for (int i = 0; i < kGhPoints; ++i) {
      const double w = kGhW[i] * kInvSqrtPi, x = kGhX[i];
      const double d = y - fma(sd, x, mu);        // y − f
      const double d2 = d * d;
      const double den = s2df + d2;                // scale² df + (y − f)²
      const double lp = c0 - lsc - 0.5 * (df + 1.0) * log1p(d2 / s2df);
      const double dlf = (df + 1.0) * d / den;     // ∂logp/∂f
      const double dls = (-1.0 + (df + 1.0) * d2 / den) / sc;  // ∂logp/∂scale
      E = fma(w, lp, E);
      gm = fma(w, dlf, gm);
      gv = fma(w * x, dlf, gv);
      gphi = fma(w, dls, gphi);
    }
    gv *= isd;
  }
}

}  // namespace gpx
