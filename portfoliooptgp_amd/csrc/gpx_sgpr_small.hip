// gpx_sgpr_small.hip — a batch of small SGPR models (the collapsed Titsias bound, Gaussian
// likelihood, zero mean), one model per 256-thread workgroup, one launch per call: a sweep of the
// reference's SGPR cell (test_scripts/SVGP.py:393-400: SGPR((X, Y), SquaredExponential(),
// inducing_variable=np.linspace(0, 360, 10)[:, None]), N ≈ 113, M = 10) over kernels, inducing
// counts and series. The arithmetic is the header comment of gpx_sgpr.hip (W = L⁻¹, G, w, Ĝ, â,
// B = I + Ĝ/s, WB = LB⁻¹, B⁻¹, γ, H, P = WᵀHW, K̄mn, K̄mm, k̄_nn, ∂θ, ∂Z, jitter 1e-6; F and ∂s are
// put together on the host from the downloaded scalars); the limits are M <= 32, N <= 4096,
// D <= GPX_MAX_DIM, no ARD terms.
//
// A workgroup keeps every M x M matrix in LDS (32 x 32, stride 33; no loop reads rows or columns
// >= M) and streams the N axis TWICE in 64-column chunks, because P depends on G, which needs the
// whole axis:
//   pass 1   Kc = k(Z, chunk);  G += Kc Kcᵀ,  w += Kc y,  Σy²,  Σk_nn,  k̄_nn Σ∂k_nn/∂θ
//   middle   Ĝ = W G Wᵀ, â = W w, B, LB, WB, γ, B⁻¹, the traces, H, the K̄mm middle, P, K̄mm'
//   pass 2   Kc again;  Yc = P·Kc;  K̄mn = Yc + u yᵀ contracted with ∂Kmn/∂θ and ∂Kmn/∂Z
//   tail     sym(K̄mm') contracted with ∂Kmm/∂θ and ∂Kmm/∂Z (factor 2 on Z)
// Kmn is never kept (at M = 32, N = 4096 it is 1 MiB).
//
// Ordering: every sum is taken in an order fixed by the model's own (n, M, D, spec) — chunks
// ascending, columns ascending inside a thread, the 64-lane butterfly, the four waves in order —
// and the kernel instance is picked by the model's own spec (single-term or not) and the object's
// D. Workgroups share nothing: no atomics, no flags. A model's result is therefore the same bits
// whatever else is in the call and wherever it sits in the active list.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "gpx_host.h"
#include "gpx_reduce.h"

using namespace gpx;

namespace {

constexpr int kSmallM = 32;       // M limit: the padded edge of every M x M matrix
constexpr int kSmallN = 4096;     // N limit
constexpr int kChunk = 64;        // columns of the N axis per pass step
constexpr int kLd = kSmallM + 1;  // LDS stride of the M x M matrices
constexpr int kLdc = kChunk + 1;  // LDS stride of the M x 64 chunk matrices
constexpr double kJitter = 1e-6;  // gpflow.config.default_jitter()
constexpr int kHdr = 4;           // ints per row header: slot, n, m, 0
// the downloaded scalars of a row: Σy², Σk_nn, tr(Ĝ), Σ B⁻¹∘Ĝ, γᵀĜγ, âᵀγ, Σ log LB_ii, info Kmm, info B
constexpr int kScal = 12;

// per-slot state written by gpx_sgpr_small_bind
struct SgprMeta {
  DevSpec spec;
};

// Packed per-call rows, one per active model, in launch order (row k = block k0 + blockIdx.x):
//   in  [θ 16][Z m·D]   (compact, the model's own m; row stride in_stride)
//   out [scalars 12][∂θ 16][∂Z m·D]
struct SgprArgs {
  const int* hdr;         // [rows][kHdr]
  const SgprMeta* meta;   // [B]
  const double* X;        // [B][Nmax·D]
  const double* Y;        // [B][Nmax]
  const double* in;
  double* out;
  int in_stride, out_stride;
  int Nmax, Mmax, D, k0;
};

struct SgprPredArgs {
  const int* hdr;         // one row
  const SgprMeta* meta;
  const double* X;        // the slot's data
  const double* Y;
  const double* in;       // one packed input row
  const double* Xnew;     // [Mn][D]
  double* mean;           // [Mn]
  double* var;            // [Mn]
  int* info;              // [2]
  int Mn, D, add_noise;
};

// the LDS of one workgroup (doubles). DM <= 8: at most 76.0 KiB, DM = 16: 84.0 KiB
// (profiles/sgpr_batch.md). The roles of the buffers over the phases are DESIGN's LDS map.
template <int DM>
struct SgprLds {
  double A[kSmallM * kLd];    // Kmm -> L;  middle: B -> LB, then H·W, then Mid·W
  double W[kSmallM * kLd];    // L⁻¹
  double WB[kSmallM * kLd];   // LB⁻¹;  from the end of the middle: P = Wᵀ H W
  double M1[kSmallM * kLd];   // G, then B⁻¹, then K̄mm' = Wᵀ Mid W
  double Kc[kSmallM * kLdc];  // the Kmn chunk;  middle (stride kLd): W·G, then H
  double Yc[kSmallM * kLdc];  // P·Kc;  middle (stride kLd): Ĝ, then Mid in place
  double z[kSmallM * DM];
  double x[kChunk * DM];
  double gz[kSmallM * DM];    // ∂Z accumulated
  double y[kChunk];
  double w[kSmallM], ah[kSmallM], t1[kSmallM], gam[kSmallM], u[kSmallM];
  double th[GPX_THETA_STRIDE];
  double red[64];
  double out16[GPX_THETA_STRIDE];
  int info[2];
};

// the elements (i, j) of a 32 x 32 matrix owned by this thread, i, j < m
template <class F>
__device__ __forceinline__ void for_mm(int m, F f) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = threadIdx.x + 256 * r;
    const int i = e >> 5, j = e & 31;
    if (i < m && j < m) f(i, j);
  }
}

// In-LDS factorisation of the leading m x m block of A (lower triangle read) and its inverse:
// A <- chol(A) by the right-looking sweep, Wi <- A⁻¹ by forward substitution, one column per
// thread. A pivot that is not > 0 records its 1-based index in *info (the first one only); the
// arithmetic goes on (NaN from there), so the workgroup's control flow never depends on the data.
__device__ __forceinline__ void chol_and_inverse(double* A, double* Wi, int m, int* info) {
  const int tid = threadIdx.x;
  for (int j = 0; j < m; ++j) {
    __syncthreads();
    if (tid == 0) {
      const double p = A[j * kLd + j];
      if (!(p > 0.0) && *info == 0) *info = j + 1;
      A[j * kLd + j] = sqrt(p);
    }
    __syncthreads();
    if (tid > j && tid < m) A[tid * kLd + j] /= A[j * kLd + j];
    __syncthreads();
    for_mm(m, [&](int i, int k) {
      if (k > j && k <= i) A[i * kLd + k] = fma(-A[i * kLd + j], A[k * kLd + j], A[i * kLd + k]);
    });
  }
  __syncthreads();
  if (tid < m) {
    const int j = tid;
    Wi[j * kLd + j] = 1.0 / A[j * kLd + j];
    for (int i = j + 1; i < m; ++i) {
      double acc = 0.0;
      for (int k = j; k < i; ++k) acc = fma(A[i * kLd + k], Wi[k * kLd + j], acc);
      Wi[i * kLd + j] = -acc / A[i * kLd + i];
    }
  }
  __syncthreads();
}

// the chunk [c0, c0 + nv) of the column points into LDS; Kc = k(Z, chunk), zero on rows >= m and
// columns >= nv. Ends with a barrier.
template <int DM>
__device__ __forceinline__ void chunk_k(SgprLds<DM>& s, const DevSpec& spec, const double* __restrict__ X, int c0,
                                        int nv, int m, int D) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < nv * D; e += 256) s.x[e] = X[(long long)c0 * D + e];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = wave + 4 * r;
    double v = 0.0;
    if (i < m && lane < nv) v = eval_k(spec, s.th, s.z + i * D, s.x + lane * D);
    s.Kc[i * kLdc + lane] = v;
  }
  __syncthreads();
}

// What the bound and the prediction share: θ and Z into LDS, Kmm = k(Z, Z) + 1e-6 I, L, W = L⁻¹;
// pass 1 over the slot's data (G, w, and with GRAD also Σy², Σk_nn and k̄_nn Σ∂k_nn/∂θ into sums /
// sq / kd of wave 0's threads); Ĝ = W G Wᵀ (left in s.Yc, stride kLd), â = W w, B = I + Ĝ/s,
// LB (s.A), WB = LB⁻¹, γ = WBᵀ(WB â). Ends with a barrier.
template <int DM, int NT, bool GRAD>
__device__ __forceinline__ void sgpr_state(SgprLds<DM>& s, const DevSpec& spec, const double* __restrict__ in,
                                           const double* __restrict__ X, const double* __restrict__ Y, int n, int m,
                                           int D, double (&sums)[NT][3], double& sq, double& kd) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* gZ = in + GPX_THETA_STRIDE;
  if (tid < GPX_THETA_STRIDE) s.th[tid] = in[tid];
  for (int e = tid; e < m * D; e += 256) s.z[e] = gZ[e];
  if (tid < 2) s.info[tid] = 0;
  if (tid < kSmallM) s.w[tid] = 0.0;
  __syncthreads();
  for (int e = tid; e < kSmallM * kSmallM; e += 256) {
    const int i = e >> 5, j = e & 31;
    double v = 0.0;
    if (i < m && j <= i) {
      v = eval_k(spec, s.th, s.z + i * D, s.z + j * D);
      if (i == j) v += kJitter;
    }
    s.A[i * kLd + j] = v;
    s.W[i * kLd + j] = 0.0;
    s.WB[i * kLd + j] = 0.0;
  }
  chol_and_inverse(s.A, s.W, m, &s.info[0]);

  const double s2 = s.th[spec.n_params];
  const double cnn = -0.5 / s2;  // k̄_nn
  double gacc[4] = {0.0, 0.0, 0.0, 0.0};  // G entries e = tid + 256 r
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int nv = min(kChunk, n - c0);
    __syncthreads();  // the previous chunk's readers are done with x, y, Kc
    if (tid < kChunk) s.y[tid] = tid < nv ? Y[c0 + tid] : 0.0;
    chunk_k<DM>(s, spec, X, c0, nv, m, D);
    if (GRAD && tid < nv) {  // one column per thread of wave 0
      const double yv = s.y[tid];
      sq = fma(yv, yv, sq);
      double dk[NT][3];
      kd += eval_k_grad<NT>(spec, s.th, s.x + tid * D, s.x + tid * D, dk);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        sums[t][0] = fma(cnn, dk[t][0], sums[t][0]);
        sums[t][1] = fma(cnn, dk[t][1], sums[t][1]);
        sums[t][2] = fma(cnn, dk[t][2], sums[t][2]);
      }
    }
    // w += Kc y (Kc and y are zero past nv)
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const int i = wave + 4 * r;
      if (i >= m) break;  // (wave-uniform)
      const double wv = wsum(s.Kc[i * kLdc + lane] * s.y[lane]);
      if (lane == 0) s.w[i] += wv;
    }
    // G += Kc Kcᵀ
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = tid + 256 * r;
      const int i = e >> 5, k = e & 31;
      if (i < m && k < m) {
        double acc = gacc[r];
        for (int j = 0; j < kChunk; ++j) acc = fma(s.Kc[i * kLdc + j], s.Kc[k * kLdc + j], acc);
        gacc[r] = acc;
      }
    }
  }
  __syncthreads();

  // ---- the middle, first half ----
  double* G = s.M1;
  double* T = s.Kc;   // stride kLd from here to pass 2
  double* Gh = s.Yc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = tid + 256 * r;
    const int i = e >> 5, j = e & 31;
    G[i * kLd + j] = (i < m && j < m) ? gacc[r] : 0.0;
  }
  __syncthreads();
  // T = W G;  â = W w
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = 0; k <= i; ++k) acc = fma(s.W[i * kLd + k], G[k * kLd + j], acc);
    T[i * kLd + j] = acc;
  });
  if (tid < m) {
    double acc = 0.0;
    for (int k = 0; k <= tid; ++k) acc = fma(s.W[tid * kLd + k], s.w[k], acc);
    s.ah[tid] = acc;
  }
  __syncthreads();
  // Ĝ = T Wᵀ
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = 0; k <= j; ++k) acc = fma(T[i * kLd + k], s.W[j * kLd + k], acc);
    Gh[i * kLd + j] = acc;
  });
  __syncthreads();
  // B = I + Ĝ/s over L's buffer (lower triangle), factored in place: LB, WB
  for_mm(m, [&](int i, int j) {
    s.A[i * kLd + j] = j <= i ? (i == j ? 1.0 : 0.0) + Gh[i * kLd + j] / s2 : 0.0;
  });
  chol_and_inverse(s.A, s.WB, m, &s.info[1]);
  // γ = WBᵀ (WB â)
  if (tid < m) {
    double acc = 0.0;
    for (int k = 0; k <= tid; ++k) acc = fma(s.WB[tid * kLd + k], s.ah[k], acc);
    s.t1[tid] = acc;
  }
  __syncthreads();
  if (tid < m) {
    double acc = 0.0;
    for (int k = tid; k < m; ++k) acc = fma(s.WB[k * kLd + tid], s.t1[k], acc);
    s.gam[tid] = acc;
  }
  __syncthreads();
}

template <int DM, int NT>
__global__ __launch_bounds__(256) void sgpr_small_kernel(SgprArgs a) {
  __shared__ SgprLds<DM> s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = a.k0 + blockIdx.x;
  const int* h = a.hdr + row * kHdr;
  const int b = h[0];
  const int n = min(max(h[1], 1), min(a.Nmax, kSmallN));
  const int m = min(max(h[2], 1), min(a.Mmax, kSmallM));
  const int D = a.D;
  const DevSpec spec = a.meta[b].spec;
  const double* in = a.in + (long long)row * a.in_stride;
  double* out = a.out + (long long)row * a.out_stride;
  const double* X = a.X + (long long)b * a.Nmax * D;
  const double* Y = a.Y + (long long)b * a.Nmax;

  double sums[NT][3];
#pragma unroll
  for (int t = 0; t < NT; ++t) sums[t][0] = sums[t][1] = sums[t][2] = 0.0;
  double sq = 0.0, kd = 0.0;  // Σy², Σk_nn over this thread's columns (wave 0)
  sgpr_state<DM, NT, true>(s, spec, in, X, Y, n, m, D, sums, sq, kd);
  const double s2 = s.th[spec.n_params];
  for (int e = tid; e < kSmallM * DM; e += 256) s.gz[e] = 0.0;

  // ---- the middle, second half (all M x M buffers at stride kLd) ----
  double* Bi = s.M1;  // B⁻¹ = WBᵀ WB (G is consumed)
  double* Gh = s.Yc;
  double* H = s.Kc;
  double* Mid = s.Yc;  // in place over Ĝ
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = (i > j ? i : j); k < m; ++k) acc = fma(s.WB[k * kLd + i], s.WB[k * kLd + j], acc);
    Bi[i * kLd + j] = acc;
  });
  const double ssq = wsum(sq), skd = wsum(kd);
  double ld = (tid < m) ? log(s.A[tid * kLd + tid]) : 0.0;
  ld = wsum(ld);
  if (tid == 0) { s.red[0] = ssq; s.red[1] = skd; s.red[2] = ld; }
  __syncthreads();
  // the traces tr(Ĝ), Σ B⁻¹∘Ĝ, γᵀĜγ, âᵀγ;  H = (I − B⁻¹)/s − γγᵀ/s³;  Mid = ½(I − B⁻¹) − γγᵀ/(2s²) − Ĝ/(2s)
  double tr[4] = {0.0, 0.0, 0.0, 0.0};
  for_mm(m, [&](int i, int j) {
    const double gh = Gh[i * kLd + j], bi = Bi[i * kLd + j];
    const double gi = s.gam[i], gj = s.gam[j];
    const double imb = (i == j ? 1.0 : 0.0) - bi, gg = gi * gj;
    if (i == j) tr[0] += gh;
    tr[1] = fma(bi, gh, tr[1]);
    tr[2] = fma(gi * gh, gj, tr[2]);
    if (j == 0) tr[3] = fma(s.ah[i], gi, tr[3]);
    H[i * kLd + j] = imb / s2 - gg / (s2 * s2 * s2);
    Mid[i * kLd + j] = 0.5 * imb - gg / (2.0 * s2 * s2) - gh / (2.0 * s2);
  });
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = wsum(tr[q]);
    if (lane == 0) s.red[8 + wave * 4 + q] = v;
  }
  __syncthreads();
  double* oth = out + kScal;
  double* oZ = oth + GPX_THETA_STRIDE;
  if (tid == 0) {
    out[0] = s.red[0];
    out[1] = s.red[1];
#pragma unroll
    for (int q = 0; q < 4; ++q) out[2 + q] = (s.red[8 + q] + s.red[12 + q]) + (s.red[16 + q] + s.red[20 + q]);
    out[6] = s.red[2];
    out[7] = (double)s.info[0];
    out[8] = (double)s.info[1];
    out[9] = out[10] = out[11] = 0.0;
  }
  // T = H W (over LB);  u = Wᵀ γ/s²
  double* T = s.A;
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = j; k < m; ++k) acc = fma(H[i * kLd + k], s.W[k * kLd + j], acc);
    T[i * kLd + j] = acc;
  });
  if (tid < kSmallM) {
    double acc = 0.0;
    if (tid < m) {
      const double is2 = 1.0 / (s2 * s2);
      for (int k = tid; k < m; ++k) acc = fma(s.W[k * kLd + tid], s.gam[k] * is2, acc);
    }
    s.u[tid] = acc;
  }
  __syncthreads();
  // P = Wᵀ T (over WB, which is consumed)
  double* P = s.WB;
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = i; k < m; ++k) acc = fma(s.W[k * kLd + i], T[k * kLd + j], acc);
    P[i * kLd + j] = acc;
  });
  __syncthreads();
  // T2 = Mid W (over T);  K̄mm' = Wᵀ T2 (over B⁻¹)
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = j; k < m; ++k) acc = fma(Mid[i * kLd + k], s.W[k * kLd + j], acc);
    T[i * kLd + j] = acc;
  });
  __syncthreads();
  double* Sb = s.M1;
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = i; k < m; ++k) acc = fma(s.W[k * kLd + i], T[k * kLd + j], acc);
    Sb[i * kLd + j] = acc;
  });

  // ---- pass 2: K̄mn = P·Kmn + u yᵀ contracted with ∂Kmn/∂θ and ∂Kmn/∂Z ----
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int nv = min(kChunk, n - c0);
    __syncthreads();  // the previous chunk's (or the middle's) readers are done with x, y, Kc, Yc
    if (tid < kChunk) s.y[tid] = tid < nv ? Y[c0 + tid] : 0.0;
    chunk_k<DM>(s, spec, X, c0, nv, m, D);
    double acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.0;
    for (int k = 0; k < m; ++k) {
      const double kv = s.Kc[k * kLdc + lane];
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = fma(P[(wave + 4 * r) * kLd + k], kv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = wave + 4 * r;
      s.Yc[i * kLdc + lane] = i < m ? acc[r] : 0.0;
    }
    // (a thread reads back only the Yc entries it wrote: no barrier in between)
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const int i = wave + 4 * r;
      if (i >= m) break;  // (wave-uniform)
      const bool on = lane < nv;
      const int jj = on ? lane : 0;
      const double kb = on ? fma(s.u[i], s.y[lane], s.Yc[i * kLdc + lane]) : 0.0;
      double dk[NT][3];
      eval_k_grad<NT>(spec, s.th, s.z + i * D, s.x + jj * D, dk);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        sums[t][0] = fma(kb, dk[t][0], sums[t][0]);
        sums[t][1] = fma(kb, dk[t][1], sums[t][1]);
        sums[t][2] = fma(kb, dk[t][2], sums[t][2]);
      }
      double gzv[DM];
      eval_k_dx1<DM>(spec, s.th, s.z + i * D, s.x + jj * D, gzv);
#pragma unroll
      for (int d = 0; d < DM; ++d) {
        const double v = wsum(kb * gzv[d]);
        if (lane == 0 && d < D) s.gz[i * D + d] += v;
      }
    }
  }
  __syncthreads();
  // ---- sym(K̄mm') contracted with ∂Kmm/∂θ and ∂Kmm/∂Z (symmetric: factor 2 on Z) ----
#pragma unroll 1
  for (int r = 0; r < 8; ++r) {
    const int i = wave + 4 * r;
    if (i >= m) break;  // (wave-uniform)
    const bool on = lane < m;
    const int jj = on ? lane : 0;
    const double kb = on ? 0.5 * (Sb[i * kLd + jj] + Sb[jj * kLd + i]) : 0.0;
    double dk[NT][3];
    eval_k_grad<NT>(spec, s.th, s.z + i * D, s.z + jj * D, dk);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      sums[t][0] = fma(kb, dk[t][0], sums[t][0]);
      sums[t][1] = fma(kb, dk[t][1], sums[t][1]);
      sums[t][2] = fma(kb, dk[t][2], sums[t][2]);
    }
    double gzv[DM];
    eval_k_dx1<DM>(spec, s.th, s.z + i * D, s.z + jj * D, gzv);
#pragma unroll
    for (int d = 0; d < DM; ++d) {
      const double v = wsum(kb * gzv[d]);
      if (lane == 0 && d < D) s.gz[i * D + d] += 2.0 * v;
    }
  }
  __syncthreads();
  for (int e = tid; e < m * D; e += 256) oZ[e] = s.gz[e];
  reduce_theta<NT>(sums, &a.meta[b].spec, s.red, s.out16);
  if (tid < GPX_THETA_STRIDE) oth[tid] = tid < spec.n_params ? s.out16[tid] : 0.0;
}

// predict_f / predict_y of one slot at Mn points, 64 per workgroup; every workgroup recomputes
// the model's state from the bound data (pass 1 and the first half of the middle):
//   mean = Kmsᵀ Wᵀγ/s,  var = k** − Σ_m (W Kms)² + Σ_m (WB W Kms)² (+σ²)
template <int DM>
__global__ __launch_bounds__(256) void sgpr_small_predict_kernel(SgprPredArgs a) {
  __shared__ SgprLds<DM> s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = a.hdr[0];
  const int n = min(max(a.hdr[1], 1), kSmallN);
  const int m = min(max(a.hdr[2], 1), kSmallM);
  const int D = a.D;
  const DevSpec spec = a.meta[b].spec;
  double sums[1][3] = {{0.0, 0.0, 0.0}};
  double sq = 0.0, kd = 0.0;
  sgpr_state<DM, 1, false>(s, spec, a.in, a.X, a.Y, n, m, D, sums, sq, kd);
  const double s2 = s.th[spec.n_params];
  if (blockIdx.x == 0 && tid < 2) a.info[tid] = s.info[tid];
  // u = Wᵀ γ/s
  if (tid < kSmallM) {
    double acc = 0.0;
    if (tid < m) {
      const double is = 1.0 / s2;
      for (int k = tid; k < m; ++k) acc = fma(s.W[k * kLd + tid], s.gam[k] * is, acc);
    }
    s.u[tid] = acc;
  }
  const int c0 = blockIdx.x * kChunk;
  const int nv = min(kChunk, a.Mn - c0);
  chunk_k<DM>(s, spec, a.Xnew, c0, nv, m, D);  // (its barriers also publish u)
  double mu = 0.0;
  if (tid < nv)
    for (int i = 0; i < m; ++i) mu = fma(s.Kc[i * kLdc + tid], s.u[i], mu);
  // A* = W Kc into Yc
#pragma unroll 1
  for (int r = 0; r < 8; ++r) {
    const int i = wave + 4 * r;
    double acc = 0.0;
    if (i < m)
      for (int k = 0; k <= i; ++k) acc = fma(s.W[i * kLd + k], s.Kc[k * kLdc + lane], acc);
    s.Yc[i * kLdc + lane] = acc;
  }
  __syncthreads();
  // WB A* over Kc
#pragma unroll 1
  for (int r = 0; r < 8; ++r) {
    const int i = wave + 4 * r;
    double acc = 0.0;
    if (i < m)
      for (int k = 0; k <= i; ++k) acc = fma(s.WB[i * kLd + k], s.Yc[k * kLdc + lane], acc);
    s.Kc[i * kLdc + lane] = acc;
  }
  __syncthreads();
  if (tid < nv) {
    double va = 0.0, vb = 0.0;
    for (int i = 0; i < m; ++i) {
      const double av = s.Yc[i * kLdc + tid], bv = s.Kc[i * kLdc + tid];
      va = fma(av, av, va);
      vb = fma(bv, bv, vb);
    }
    double v = eval_kdiag(spec, s.th, s.x + tid * D) - va + vb;
    if (a.add_noise) v += s2;
    a.mean[c0 + tid] = mu;
    a.var[c0 + tid] = v;
  }
}

int dm_of(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : 16; }

template <int NT>
void launch_sgpr_small_nt(const SgprArgs& a, int nblocks, hipStream_t s) {
  const dim3 grid(nblocks), block(256);
  switch (dm_of(a.D)) {
    case 1: hipLaunchKernelGGL((sgpr_small_kernel<1, NT>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((sgpr_small_kernel<2, NT>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((sgpr_small_kernel<4, NT>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((sgpr_small_kernel<8, NT>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((sgpr_small_kernel<16, NT>), grid, block, 0, s, a); break;
  }
}

void launch_sgpr_small_predict(const SgprPredArgs& a, hipStream_t s) {
  const dim3 grid((a.Mn + kChunk - 1) / kChunk), block(256);
  switch (dm_of(a.D)) {
    case 1: hipLaunchKernelGGL((sgpr_small_predict_kernel<1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((sgpr_small_predict_kernel<2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((sgpr_small_predict_kernel<4>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((sgpr_small_predict_kernel<8>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((sgpr_small_predict_kernel<16>), grid, block, 0, s, a); break;
  }
}

}  // namespace

struct gpx_sgpr_small {
  gpx_ctx* ctx = nullptr;
  int B = 0, Nmax = 0, Mmax = 0, D = 0;
  int in_stride = 0, out_stride = 0;  // doubles per packed row
  std::vector<int> n, m;              // per slot; n = 0: not bound
  std::vector<gpx_kernel_spec> specs;
  double *dX = nullptr, *dY = nullptr;
  SgprMeta* d_meta = nullptr;
  // one device block and its pinned mirror per direction: [hdr B·4 ints][B packed input rows] up,
  // [B packed output rows] down
  char *d_in = nullptr, *h_in = nullptr;
  double *d_out = nullptr, *h_out = nullptr;
  size_t hdr_bytes = 0;
  // predict: grow-only [hdr][θ][Z][Xnew Mn·D] up and [mean Mn][var Mn][info 2] down
  double *d_px = nullptr, *h_px = nullptr, *d_po = nullptr, *h_po = nullptr;
  size_t px_cap = 0, po_cap = 0;
  std::vector<int> order;  // the call's launch order (positions into `active`)
};

namespace {

const char* kArdMsg = "ARD terms (GPX_TERM_ARD) are served by the gpx_batch_* entry points only";
const char* kKmmMsg = "Kmm + jitter I is not positive definite";
const char* kBMsg = "B = I + W G Wᵀ/s is not positive definite";

// the θ / Z checks of gpx_sgpr.hip's prelude for one slot's row
int check_row(gpx_ctx* ctx, const gpx_kernel_spec& spec, int m, int D, const double* theta, const double* Z) {
  for (int p = 0; p <= spec.n_params; ++p)
    if (!(theta[p] > 0.0) || !std::isfinite(theta[p]))
      return fail(ctx, GPX_BAD_ARG, "theta must be finite and > 0 (constrained space)");
  for (int e = 0; e < m * D; ++e)
    if (!std::isfinite(Z[e])) return fail(ctx, GPX_BAD_ARG, "Z must be finite");
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_sgpr_small_limits(int* m_max, int* n_max) {
  if (!m_max || !n_max) return GPX_BAD_ARG;
  *m_max = kSmallM;
  *n_max = kSmallN;
  return GPX_OK;
}

int gpx_sgpr_small_destroy(gpx_sgpr_small* sm) {
  if (!sm) return GPX_BAD_ARG;
  (void)hipSetDevice(sm->ctx->device);
  for (void* p : {(void*)sm->dX, (void*)sm->dY, (void*)sm->d_meta, (void*)sm->d_in, (void*)sm->d_out,
                  (void*)sm->d_px, (void*)sm->d_po})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)sm->h_in, (void*)sm->h_out, (void*)sm->h_px, (void*)sm->h_po})
    if (p) (void)hipHostFree(p);
  delete sm;
  return GPX_OK;
}

int gpx_sgpr_small_create(gpx_ctx* ctx, int B, int N_max, int M_max, int D, gpx_sgpr_small** out) {
  if (!ctx || !out) return GPX_BAD_ARG;
  *out = nullptr;
  if (B < 1 || N_max < 1 || M_max < 1 || D < 1)
    return fail(ctx, GPX_BAD_ARG, "bad sgpr_small dimensions");
  if (M_max > kSmallM || N_max > kSmallN || D > GPX_MAX_DIM)
    return fail(ctx, GPX_BAD_ARG, "shape over the fused small-shape limits (M <= 32, N <= 4096, D <= 16)");
  HIPX(ctx, hipSetDevice(ctx->device));
  gpx_sgpr_small* sm = new gpx_sgpr_small();
  sm->ctx = ctx; sm->B = B; sm->Nmax = N_max; sm->Mmax = M_max; sm->D = D;
  sm->in_stride = GPX_THETA_STRIDE + M_max * D;
  sm->out_stride = kScal + GPX_THETA_STRIDE + M_max * D;
  sm->n.assign(B, 0);
  sm->m.assign(B, 0);
  sm->specs.resize(B);
  sm->hdr_bytes = ((size_t)B * kHdr * sizeof(int) + 15) / 16 * 16;
  const size_t in_bytes = sm->hdr_bytes + sizeof(double) * (size_t)B * sm->in_stride;
  const size_t out_bytes = sizeof(double) * (size_t)B * sm->out_stride;
  if (hipMalloc(&sm->dX, sizeof(double) * (size_t)B * N_max * D) != hipSuccess ||
      hipMalloc(&sm->dY, sizeof(double) * (size_t)B * N_max) != hipSuccess ||
      hipMalloc(&sm->d_meta, sizeof(SgprMeta) * B) != hipSuccess ||
      hipMalloc(&sm->d_in, in_bytes) != hipSuccess || hipMalloc(&sm->d_out, out_bytes) != hipSuccess ||
      hipMemset(sm->dX, 0, sizeof(double) * (size_t)B * N_max * D) != hipSuccess ||
      hipMemset(sm->dY, 0, sizeof(double) * (size_t)B * N_max) != hipSuccess ||
      hipMemset(sm->d_meta, 0, sizeof(SgprMeta) * B) != hipSuccess ||
      hipMemset(sm->d_in, 0, in_bytes) != hipSuccess || hipMemset(sm->d_out, 0, out_bytes) != hipSuccess) {
    gpx_sgpr_small_destroy(sm);
    return fail(ctx, GPX_HIP_ERROR, "out of device memory");
  }
  if (hipHostMalloc(&sm->h_in, in_bytes, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(&sm->h_out, out_bytes, hipHostMallocDefault) != hipSuccess) {
    gpx_sgpr_small_destroy(sm);
    return fail(ctx, GPX_HIP_ERROR, "out of pinned host memory");
  }
  std::memset(sm->h_in, 0, in_bytes);
  std::memset(sm->h_out, 0, out_bytes);
  *out = sm;
  return GPX_OK;
}

int gpx_sgpr_small_bind(gpx_sgpr_small* sm, int b, int n, int m, const double* X, const double* Y,
                        const gpx_kernel_spec* spec) {
  if (!sm) return GPX_BAD_ARG;
  gpx_ctx* ctx = sm->ctx;
  if (b < 0 || b >= sm->B || !X || !Y || !spec || n < 1 || m < 1)
    return fail(ctx, GPX_BAD_ARG, "bad sgpr_small bind arguments");
  if (n > sm->Nmax || m > sm->Mmax)
    return fail(ctx, GPX_BAD_ARG, "model larger than the object's N_max / M_max");
  if (ard_spec(*spec)) return fail(ctx, GPX_BAD_ARG, kArdMsg);
  if (coreg_spec(*spec)) return fail(ctx, GPX_BAD_ARG, kCoregBatchOnlyMsg);
  if (const char* why = spec_error(*spec, sm->D)) return fail(ctx, GPX_BAD_ARG, why);
  HIPX(ctx, hipSetDevice(ctx->device));
  SgprMeta meta;
  static_assert(sizeof(DevSpec) == sizeof(gpx_kernel_spec), "spec layout");
  std::memcpy(&meta.spec, spec, sizeof(DevSpec));
  HIPX(ctx, hipMemcpy(sm->dX + (size_t)b * sm->Nmax * sm->D, X, sizeof(double) * (size_t)n * sm->D,
                      hipMemcpyHostToDevice));
  HIPX(ctx, hipMemcpy(sm->dY + (size_t)b * sm->Nmax, Y, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPX(ctx, hipMemcpy(sm->d_meta + b, &meta, sizeof(SgprMeta), hipMemcpyHostToDevice));
  sm->n[b] = n;
  sm->m[b] = m;
  sm->specs[b] = *spec;
  return GPX_OK;
}

int gpx_sgpr_small_elbo_grad(gpx_sgpr_small* sm, int n_active, const int32_t* active, const double* theta,
                             const double* Z, double* elbo, double* grad_theta, double* grad_Z, int32_t* info,
                             void* stream) {
  if (!sm) return GPX_BAD_ARG;
  gpx_ctx* ctx = sm->ctx;
  if (n_active < 0 || n_active > sm->B || (n_active > 0 && !active) || !theta || !Z || !elbo || !grad_theta ||
      !grad_Z || !info)
    return fail(ctx, GPX_BAD_ARG, "null sgpr_small argument or bad active count");
  if (n_active == 0) return GPX_OK;
  const int B = sm->B, D = sm->D, Mx = sm->Mmax;
  const size_t sZ = (size_t)Mx * D;
  std::vector<char> seen(B, 0);
  for (int k = 0; k < n_active; ++k) {
    const int b = active[k];
    if (b < 0 || b >= B || seen[b] || sm->n[b] == 0)
      return fail(ctx, GPX_BAD_ARG, "active slot out of range, repeated or not bound");
    seen[b] = 1;
    const int rc = check_row(ctx, sm->specs[b], sm->m[b], D, theta + (size_t)b * GPX_THETA_STRIDE, Z + b * sZ);
    if (rc != GPX_OK) return rc;
  }
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // launch order: the single-term models, then the others, each group in the caller's order (a
  // model's kernel instance depends on its own spec only)
  sm->order.clear();
  for (int k = 0; k < n_active; ++k)
    if (sm->specs[active[k]].n_terms == 1) sm->order.push_back(k);
  const int n1 = (int)sm->order.size();
  for (int k = 0; k < n_active; ++k)
    if (sm->specs[active[k]].n_terms != 1) sm->order.push_back(k);
  int* hdr = reinterpret_cast<int*>(sm->h_in);
  double* rows = reinterpret_cast<double*>(sm->h_in + sm->hdr_bytes);
  for (int r = 0; r < n_active; ++r) {
    const int b = active[sm->order[r]];
    hdr[r * kHdr] = b; hdr[r * kHdr + 1] = sm->n[b]; hdr[r * kHdr + 2] = sm->m[b]; hdr[r * kHdr + 3] = 0;
    double* row = rows + (size_t)r * sm->in_stride;
    std::memcpy(row, theta + (size_t)b * GPX_THETA_STRIDE, sizeof(double) * GPX_THETA_STRIDE);
    std::memcpy(row + GPX_THETA_STRIDE, Z + b * sZ, sizeof(double) * sm->m[b] * D);
  }
  const size_t up = sm->hdr_bytes + sizeof(double) * (size_t)n_active * sm->in_stride;
  HIPX(ctx, hipMemcpyAsync(sm->d_in, sm->h_in, up, hipMemcpyHostToDevice, s));
  SgprArgs a{};
  a.hdr = reinterpret_cast<const int*>(sm->d_in);
  a.meta = sm->d_meta; a.X = sm->dX; a.Y = sm->dY;
  a.in = reinterpret_cast<const double*>(sm->d_in + sm->hdr_bytes);
  a.out = sm->d_out; a.in_stride = sm->in_stride; a.out_stride = sm->out_stride;
  a.Nmax = sm->Nmax; a.Mmax = Mx; a.D = D;
  if (n1 > 0) {
    a.k0 = 0;
    launch_sgpr_small_nt<1>(a, n1, s);
  }
  if (n_active > n1) {
    a.k0 = n1;
    launch_sgpr_small_nt<GPX_MAX_TERMS>(a, n_active - n1, s);
  }
  HIPX(ctx, hipGetLastError());
  HIPX(ctx, hipMemcpyAsync(sm->h_out, sm->d_out, sizeof(double) * (size_t)n_active * sm->out_stride,
                           hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  int bad_kmm = 0, bad_b = 0;
  for (int r = 0; r < n_active; ++r) {
    const int b = active[sm->order[r]];
    const int m = sm->m[b], np = sm->specs[b].n_params;
    const double* o = sm->h_out + (size_t)r * sm->out_stride;
    const double* oth = o + kScal;
    const double* oZ = oth + GPX_THETA_STRIDE;
    const double s2 = theta[(size_t)b * GPX_THETA_STRIDE + np], n = (double)sm->n[b];
    const double yy = o[0], knn = o[1], trG = o[2], trBG = o[3], gGg = o[4], ag = o[5], ld = o[6];
    elbo[b] = -0.5 * n * std::log(2.0 * M_PI) - 0.5 * n * std::log(s2) - ld - yy / (2.0 * s2) +
              ag / (2.0 * s2 * s2) - knn / (2.0 * s2) + trG / (2.0 * s2);
    double* gth = grad_theta + (size_t)b * GPX_THETA_STRIDE;
    for (int p = 0; p < GPX_THETA_STRIDE; ++p) gth[p] = p < np ? oth[p] : 0.0;
    gth[np] = -n / (2.0 * s2) + yy / (2.0 * s2 * s2) - ag / (s2 * s2 * s2) + knn / (2.0 * s2 * s2) -
              trG / (2.0 * s2 * s2) + trBG / (2.0 * s2 * s2) + gGg / (2.0 * s2 * s2 * s2 * s2);
    std::memcpy(grad_Z + b * sZ, oZ, sizeof(double) * m * D);
    info[2 * b] = (int32_t)o[7];
    info[2 * b + 1] = (int32_t)o[8];
    if (info[2 * b] != 0) ++bad_kmm;
    else if (info[2 * b + 1] != 0) ++bad_b;
  }
  if (bad_kmm) return fail(ctx, GPX_NOT_PD, kKmmMsg);
  if (bad_b) return fail(ctx, GPX_NOT_PD, kBMsg);
  return GPX_OK;
}

int gpx_sgpr_small_predict(gpx_sgpr_small* sm, int b, const double* theta, const double* Z, const double* Xnew,
                           int Mn, int add_noise, double* mean, double* var, int32_t* info, void* stream) {
  if (!sm) return GPX_BAD_ARG;
  gpx_ctx* ctx = sm->ctx;
  if (b < 0 || b >= sm->B || sm->n[b] == 0) return fail(ctx, GPX_BAD_ARG, "slot out of range or not bound");
  if (Mn == 0) return GPX_OK;  // empty Xnew: empty outputs
  if (!theta || !Z || !Xnew || Mn < 0 || !mean || !var) return fail(ctx, GPX_BAD_ARG, "bad predict args");
  const int D = sm->D, m = sm->m[b];
  int rc = check_row(ctx, sm->specs[b], m, D, theta, Z);
  if (rc != GPX_OK) return rc;
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // up: [hdr 4 ints][θ 16][Z m·D][Xnew Mn·D];  down: [mean][var][info 2 ints]
  const size_t row = GPX_THETA_STRIDE + (size_t)m * D;
  const size_t up = 2 + row + (size_t)Mn * D, down = 2 * (size_t)Mn + 1;
  if (sm->px_cap < up) {
    if (sm->d_px) (void)hipFree(sm->d_px);
    if (sm->h_px) (void)hipHostFree(sm->h_px);
    sm->d_px = sm->h_px = nullptr; sm->px_cap = 0;
    HIPX(ctx, hipMalloc(&sm->d_px, sizeof(double) * up));
    HIPX(ctx, hipHostMalloc(&sm->h_px, sizeof(double) * up, hipHostMallocDefault));
    sm->px_cap = up;
  }
  if (sm->po_cap < down) {
    if (sm->d_po) (void)hipFree(sm->d_po);
    if (sm->h_po) (void)hipHostFree(sm->h_po);
    sm->d_po = sm->h_po = nullptr; sm->po_cap = 0;
    HIPX(ctx, hipMalloc(&sm->d_po, sizeof(double) * down));
    HIPX(ctx, hipHostMalloc(&sm->h_po, sizeof(double) * down, hipHostMallocDefault));
    sm->po_cap = down;
  }
  int* hdr = reinterpret_cast<int*>(sm->h_px);
  hdr[0] = b; hdr[1] = sm->n[b]; hdr[2] = m; hdr[3] = 0;
  double* r = sm->h_px + 2;
  std::memcpy(r, theta, sizeof(double) * GPX_THETA_STRIDE);
  std::memcpy(r + GPX_THETA_STRIDE, Z, sizeof(double) * m * D);
  std::memcpy(r + row, Xnew, sizeof(double) * (size_t)Mn * D);
  HIPX(ctx, hipMemcpyAsync(sm->d_px, sm->h_px, sizeof(double) * up, hipMemcpyHostToDevice, s));
  SgprPredArgs a{};
  a.hdr = reinterpret_cast<const int*>(sm->d_px);
  a.meta = sm->d_meta;
  a.X = sm->dX + (size_t)b * sm->Nmax * D;
  a.Y = sm->dY + (size_t)b * sm->Nmax;
  a.in = sm->d_px + 2;
  a.Xnew = sm->d_px + 2 + row;
  a.mean = sm->d_po;
  a.var = sm->d_po + Mn;
  a.info = reinterpret_cast<int*>(sm->d_po + 2 * (size_t)Mn);
  a.Mn = Mn; a.D = D; a.add_noise = add_noise ? 1 : 0;
  launch_sgpr_small_predict(a, s);
  HIPX(ctx, hipGetLastError());
  HIPX(ctx, hipMemcpyAsync(sm->h_po, sm->d_po, sizeof(double) * down, hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  std::memcpy(mean, sm->h_po, sizeof(double) * Mn);
  std::memcpy(var, sm->h_po + Mn, sizeof(double) * Mn);
  const int* inf = reinterpret_cast<const int*>(sm->h_po + 2 * (size_t)Mn);
  if (info) { info[0] = inf[0]; info[1] = inf[1]; }
  if (inf[0] != 0) return fail(ctx, GPX_NOT_PD, kKmmMsg);
  if (inf[1] != 0) return fail(ctx, GPX_NOT_PD, kBMsg);
  return GPX_OK;
}

}  // extern "C"
