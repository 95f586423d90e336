// gpx_svgp_lik_kernels.hip — device kernels of SVGP's per-point route (gpx_svgp_create_lik; the
// launch sequence is in gpx_svgp.hip): between the GEMM Q = P·Kmn and the split-K GEMM
// G_w = (Kmn·diag(g_v))·Kmnᵀ they form the marginal variance of every data row, its variational
// expectation, and the per-row weights flowing back. Kmn, Q and Ks are row-major [Mp][Ncols], so
// every M×N stream runs lanes along n, 16 bytes per lane (Ncols is a multiple of 64 and the
// buffers come from hipMalloc: every double2 below is aligned). Plain vector stores, no atomics:
// sums leave as block / slice partials for launch_sum.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "gpx_internal.h"
#include "gpx_quad.h"
#include "gpx_reduce.h"

namespace gpx {

namespace {

constexpr int kColsPerBlock = 512;   // 256 lanes x double2

// part[b][n] = Σ_{m in slice b} Kmn[m,n]·Q[m,n]  (+ k(x_n, x_n) in slice 0, n < a.n). Four rows in
// flight per lane (eight independent 16-byte loads); the grid is (column blocks) x (m-slices).
__global__ __launch_bounds__(256) void svgp_colvar_kernel(SvgpColvarArgs a) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (c >= a.ld) return;
  const int rs = a.rows / a.slices;
  const long long ld2 = a.ld / 2;
  const long long o = (long long)blockIdx.y * rs * ld2 + c / 2;
  const double2* __restrict__ k = reinterpret_cast<const double2*>(a.Kmn) + o;
  const double2* __restrict__ q = reinterpret_cast<const double2*>(a.Q) + o;
  double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
  for (int m = 0; m < rs; m += 4) {
    const double2 k0 = k[0], k1 = k[ld2], k2 = k[2 * ld2], k3 = k[3 * ld2];
    const double2 q0 = q[0], q1 = q[ld2], q2 = q[2 * ld2], q3 = q[3 * ld2];
    x0 = fma(k0.x, q0.x, x0); y0 = fma(k0.y, q0.y, y0);
    x1 = fma(k1.x, q1.x, x1); y1 = fma(k1.y, q1.y, y1);
    x2 = fma(k2.x, q2.x, x2); y2 = fma(k2.y, q2.y, y2);
    x3 = fma(k3.x, q3.x, x3); y3 = fma(k3.y, q3.y, y3);
    k += 4 * ld2;
    q += 4 * ld2;
  }
  double2 v;
  v.x = (x0 + x1) + (x2 + x3);
  v.y = (y0 + y1) + (y2 + y3);
  if (blockIdx.y == 0) {
    const DevSpec spec = *a.spec;
    if (c < a.n) v.x += eval_kdiag(spec, a.theta, a.X + (long long)c * a.D);
    if (c + 1 < a.n) v.y += eval_kdiag(spec, a.theta, a.X + (long long)(c + 1) * a.D);
  }
  reinterpret_cast<double2*>(a.part)[(long long)blockIdx.y * ld2 + c / 2] = v;
}

// vgp_quad_kernel's expectation (ve_row) with the minibatch scale on the two row weights.
__global__ __launch_bounds__(256) void svgp_lik_quad_kernel(SvgpLikQuadArgs b) {
  __shared__ double sred[4][2];
  const VgpQuadArgs& a = b.q;
  const int n = blockIdx.x * 256 + threadIdx.x;
  double E = 0.0, gphi = 0.0;
  if (n < a.n) {
    double gm, gv;
    ve_row(a.lik, a.phi, a.df, a.c0, a.mu[n], a.v[n], a.y[n], E, gm, gv, gphi);
    a.gmu[n] = b.scale * gm;
    a.gv[n] = b.scale * gv;
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

// Y = 2·Y·diag(g_v) in place, Ks = Kmn·diag(g_v): two columns x four rows per lane.
__global__ __launch_bounds__(256) void svgp_colscale_kernel(SvgpColscaleArgs a) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (c >= a.ld) return;
  const long long ld2 = a.ld / 2;
  const long long o = (long long)blockIdx.y * 4 * ld2 + c / 2;
  const double2 g = reinterpret_cast<const double2*>(a.gv)[c / 2];
  const double2* __restrict__ k = reinterpret_cast<const double2*>(a.Kmn) + o;
  double2* __restrict__ y = reinterpret_cast<double2*>(a.Y) + o;
  double2* __restrict__ ks = reinterpret_cast<double2*>(a.Ks) + o;
  const double2 k0 = k[0], k1 = k[ld2], k2 = k[2 * ld2], k3 = k[3 * ld2];
  const double2 y0 = y[0], y1 = y[ld2], y2 = y[2 * ld2], y3 = y[3 * ld2];
  const double gx2 = 2.0 * g.x, gy2 = 2.0 * g.y;
  y[0] = make_double2(y0.x * gx2, y0.y * gy2);
  y[ld2] = make_double2(y1.x * gx2, y1.y * gy2);
  y[2 * ld2] = make_double2(y2.x * gx2, y2.y * gy2);
  y[3 * ld2] = make_double2(y3.x * gx2, y3.y * gy2);
  ks[0] = make_double2(k0.x * g.x, k0.y * g.y);
  ks[ld2] = make_double2(k1.x * g.x, k1.y * g.y);
  ks[2 * ld2] = make_double2(k2.x * g.x, k2.y * g.y);
  ks[3 * ld2] = make_double2(k3.x * g.x, k3.y * g.y);
}

// Σ_n g_v,n ∂k(x_n, x_n)/∂θ: one row per lane, X staged through LDS (resid_kernel's layout).
__global__ __launch_bounds__(256) void svgp_knn_kernel(SvgpKnnArgs a) {
  __shared__ double sx[256 * GPX_MAX_DIM];
  __shared__ double sth[GPX_THETA_STRIDE];
  __shared__ double sred[64];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * 256, D = a.D;
  for (int e = tid; e < 256 * D; e += 256) {
    const int j = j0 + e / D;
    sx[e] = j < a.n ? a.X[(long long)j0 * D + e] : 0.0;
  }
  if (tid < GPX_THETA_STRIDE) sth[tid] = a.theta[tid];
  __syncthreads();
  const DevSpec spec = *a.spec;
  const int j = j0 + tid;
  double sums[GPX_MAX_TERMS][3];
#pragma unroll
  for (int t = 0; t < GPX_MAX_TERMS; ++t) sums[t][0] = sums[t][1] = sums[t][2] = 0.0;
  if (j < a.n) {
    const double g = a.gv[j];
    double dk[GPX_MAX_TERMS][3];
    (void)eval_k_grad<GPX_MAX_TERMS>(spec, sth, sx + tid * D, sx + tid * D, dk);
#pragma unroll
    for (int t = 0; t < GPX_MAX_TERMS; ++t) {
      sums[t][0] = g * dk[t][0]; sums[t][1] = g * dk[t][1]; sums[t][2] = g * dk[t][2];
    }
  }
  reduce_theta(sums, a.spec, sred, a.part + (long long)blockIdx.x * GPX_THETA_STRIDE);
}

}  // namespace

// Each 256-lane workgroup is one wave per SIMD; the M×N stream wants several per SIMD on all 256
// CUs, so short column grids are multiplied by m-slices (a power of two, at most 16: Mp is a
// multiple of 64, every slice a multiple of four rows).
int svgp_colvar_slices(int rows, int ld) {
  const int bx = (ld + kColsPerBlock - 1) / kColsPerBlock;
  int s = 1;
  while (s < 16 && bx * s < 2048) s *= 2;
  while (s > 1 && rows % (4 * s) != 0) s /= 2;
  return s;
}

void launch_svgp_colvar(const SvgpColvarArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(svgp_colvar_kernel, dim3((a.ld + kColsPerBlock - 1) / kColsPerBlock, a.slices), dim3(256),
                     0, s, a);
}

int svgp_lik_quad_blocks(int npad) { return (npad + 255) / 256; }

void launch_svgp_lik_quad(const SvgpLikQuadArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(svgp_lik_quad_kernel, dim3(svgp_lik_quad_blocks(a.q.npad)), dim3(256), 0, s, a);
}

void launch_svgp_colscale(const SvgpColscaleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(svgp_colscale_kernel, dim3((a.ld + kColsPerBlock - 1) / kColsPerBlock, a.rows / 4),
                     dim3(256), 0, s, a);
}

int svgp_lik_knn_blocks(int n) { return (n + 255) / 256; }

void launch_svgp_knn(const SvgpKnnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(svgp_knn_kernel, dim3(svgp_lik_knn_blocks(a.n)), dim3(256), 0, s, a);
}

}  // namespace gpx
