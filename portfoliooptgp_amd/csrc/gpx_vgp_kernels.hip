// gpx_vgp_kernels.hip — device kernels of the VGP ELBO path (gpx_vgp.hip) that are not GEMMs:
// the triangle/padding pass that turns K̃ Wᵀ into L, the row stream over A = L R (v_n and the
// scaled copy g_v ∘ A), the per-row variational expectation (closed form for the Gaussian
// likelihood, 20-point Gauss–Hermite for Student-t) and the N×N elementwise tail.
#include <hip/hip_runtime.h>
#include "gpx_internal.h"

namespace gpx {

namespace {

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// numpy.polynomial.hermite.hermgauss(20): nodes x_i and weights w_i (GPflow's NDiagGHQuadrature
// divides the weights by √π and evaluates at μ + √(2v) x_i)
__constant__ double kGhX[kGhPoints] = {
    -5.3874808900112328, -4.6036824495507442, -3.9447640401156252, -3.3478545673832163,
    -2.7888060584281305, -2.2549740020892757, -1.7385377121165861, -1.2340762153953231,
    -0.73747372854539439, -0.24534070830090124, 0.24534070830090124, 0.73747372854539439,
    1.2340762153953231, 1.7385377121165861, 2.2549740020892757, 2.7888060584281305,
    3.3478545673832163, 3.9447640401156252, 4.6036824495507442, 5.3874808900112328};
__constant__ double kGhW[kGhPoints] = {
    2.2293936455341447e-13, 4.3993409922731747e-10, 1.0860693707692782e-07, 7.8025564785320599e-06,
    0.00022833863601635365, 0.0032437733422378567, 0.024810520887463643, 0.10901720602002329,
    0.28667550536283415, 0.46224366960061009, 0.46224366960061009, 0.28667550536283415,
    0.10901720602002329, 0.024810520887463643, 0.0032437733422378567, 0.00022833863601635365,
    7.8025564785320599e-06, 1.0860693707692782e-07, 4.3993409922731747e-10, 2.2293936455341447e-13};
constexpr double kInvSqrtPi = 0.56418958354775628;  // 1/√π

// L = tril(P) on the leading n×n block (P = K̃ Wᵀ from the GEMM), zeros above the diagonal, the
// identity on the padding: every np×np entry is written.
__global__ __launch_bounds__(256) void vgp_ltri_kernel(VgpLtriArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(e / a.np), j = (int)(e - (long long)(e / a.np) * a.np);
  if (i >= a.np) return;
  double* p = a.L + (long long)i * a.np + j;
  if (j > i) *p = 0.0;
  else if (i >= a.n) *p = (i == j) ? 1.0 : 0.0;
}

// One wave per row of the lower-triangular A (4 rows per workgroup), entries j <= n only.
// gv == nullptr: v_n = Σ_j A_nj². Otherwise GA_nj = gv_n A_nj.
__global__ __launch_bounds__(256) void vgp_rowsq_kernel(VgpRowsqArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  if (n >= a.rows) return;
  const double* r = a.A + (long long)n * a.ld;
  if (a.gv == nullptr) {
    double s0 = 0.0, s1 = 0.0;
    int j = lane;
    for (; j + 64 <= n; j += 128) {
      const double x0 = r[j], x1 = r[j + 64];
      s0 = fma(x0, x0, s0);
      s1 = fma(x1, x1, s1);
    }
    for (; j <= n; j += 64) s0 = fma(r[j], r[j], s0);
    const double s = wsum(s0 + s1);
    if (lane == 0) a.v[n] = s;
  } else {
    const double g = a.gv[n];
    double* o = a.GA + (long long)n * a.ld;
    for (int j = lane; j <= n; j += 64) o[j] = g * r[j];
  }
}

// Variational expectation of row n (one row per lane) and its derivatives:
//   part[block][0] = Σ ve(μ_n, v_n, y_n),  part[block][1] = Σ ∂ve/∂φ  (φ: variance or scale)
//   gmu_n = ∂ve/∂μ,  gv_n = ∂ve/∂v;  the padding rows n.. npad − 1 get gmu = gv = 0.
// c0 is the likelihood's constant: −½ log 2π, or lgamma((df+1)/2) − lgamma(df/2) − ½(log df + log π).
__global__ __launch_bounds__(256) void vgp_quad_kernel(VgpQuadArgs a) {
  __shared__ double sred[4][2];
  const int n = blockIdx.x * 256 + threadIdx.x;
  double E = 0.0, gphi = 0.0;
  if (n < a.n) {
    const double mu = a.mu[n], v = a.v[n], y = a.y[n];
    double gm, gv;
    if (a.lik == GPX_LIK_GAUSSIAN) {
      const double s = a.phi, r = y - mu, q = fma(r, r, v);
      E = a.c0 - 0.5 * log(s) - q / (2.0 * s);
      gm = r / s;
      gv = -0.5 / s;
      gphi = -0.5 / s + q / (2.0 * s * s);
    } else {
      const double sc = a.phi, df = a.df, sd = sqrt(2.0 * v), isd = 1.0 / sd;
      const double s2df = sc * sc * df, lsc = log(sc);
      gm = 0.0;
      gv = 0.0;
#pragma unroll 4
      for (int i = 0; i < kGhPoints; ++i) {
        const double w = kGhW[i] * kInvSqrtPi, x = kGhX[i];
        const double d = y - fma(sd, x, mu);        // y − f
        const double d2 = d * d;
        const double den = s2df + d2;                // scale² df + (y − f)²
        const double lp = a.c0 - lsc - 0.5 * (df + 1.0) * log1p(d2 / s2df);
        const double dlf = (df + 1.0) * d / den;     // ∂logp/∂f
        const double dls = (-1.0 + (df + 1.0) * d2 / den) / sc;  // ∂logp/∂scale
        E = fma(w, lp, E);
        gm = fma(w, dlf, gm);
        gv = fma(w * x, dlf, gv);
        gphi = fma(w, dls, gphi);
      }
      gv *= isd;
    }
    a.gmu[n] = gm;
    a.gv[n] = gv;
  } else if (n < a.npad) {
    a.gmu[n] = 0.0;
    a.gv[n] = 0.0;
  }
  const double tE = wsum(E), tg = wsum(gphi);
  if ((threadIdx.x & 63) == 0) { sred[threadIdx.x >> 6][0] = tE; sred[threadIdx.x >> 6][1] = tg; }
  __syncthreads();
  if (threadIdx.x < 2)
    a.part[(long long)blockIdx.x * 2 + threadIdx.x] =
        (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}

// N×N tail (valid i, j < n; nothing else is written):
//   Phi  = Φ(t qᵀ + 2 C Rᵀ)  (lower, diagonal halved, zeros above)   [ld]
//   Rbar = tril(2C − R + diag(1/R_ii))                               [n][n] compact
// and the factorisation's info word as a double beside the sums (one download).
__global__ __launch_bounds__(256) void vgp_final_kernel(VgpFinalArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e == 0) a.info_out[0] = (double)a.info[0];
  const int i = (int)(e / a.n), j = (int)(e - (long long)(e / a.n) * a.n);
  if (i >= a.n) return;
  const long long o = (long long)i * a.ld + j;
  const long long oc = (long long)i * a.n + j;
  if (j <= i) {
    const double F = fma(2.0, a.CRt[o], a.t[i] * a.q[j]);
    const double r = a.R[o];
    a.Phi[o] = (i == j) ? 0.5 * F : F;
    a.Rbar[oc] = 2.0 * a.C[o] - r + ((i == j) ? 1.0 / r : 0.0);
  } else {
    a.Phi[o] = 0.0;
    a.Rbar[oc] = 0.0;
  }
}

}  // namespace

void launch_vgp_ltri(const VgpLtriArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(vgp_ltri_kernel, dim3((unsigned)(((long long)a.np * a.np + 255) / 256)), dim3(256), 0, s, a);
}

void launch_vgp_rowsq(const VgpRowsqArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(vgp_rowsq_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
}

int vgp_quad_blocks(int npad) { return (npad + 255) / 256; }

void launch_vgp_quad(const VgpQuadArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(vgp_quad_kernel, dim3(vgp_quad_blocks(a.npad)), dim3(256), 0, s, a);
}

void launch_vgp_final(const VgpFinalArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(vgp_final_kernel, dim3((unsigned)(((long long)a.n * a.n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace gpx
