// gpx_svgp_small.hip — a batch of small whitened SVGP models (Gaussian likelihood, closed form),
// one model per 256-thread workgroup, one launch per call: the sweep of the reference's
// train_svgp_model (test_scripts/GPR.py:118-138: 8 kernels x one gpflow.models.SVGP with
// inducing_variable = X[:20], N = 5..~800). The arithmetic is the header comment of gpx_svgp.hip
// (W = L⁻¹, u = Wᵀq_mu, P = Wᵀ(S − I)W, G, Ĝ, K̄mn, Φ(LᵀL̄), K̄mm, ∂q_mu, ∂q_sqrt, ∂θ, ∂Z, jitter
// 1e-6); the limits are M <= 32, N <= 4096, D <= GPX_MAX_DIM, no ARD terms.
//
// A workgroup keeps every M x M matrix in LDS (32 x 32, stride 33; rows and columns >= M carry the
// identity in L and W and zeros elsewhere, and no loop reads them) and streams the N axis once in
// 64-column chunks: P and u depend on (Z, θ, q) only, so they are ready before the stream and one
// pass gives μ, g_μ, Yc = 2c·P·Kc, the K̄mn contraction with ∂Kmn/∂θ and ∂Kmn/∂Z, G += Kc Kcᵀ,
// w = Kmn g_μ, Σ(y − μ)², Σ k_nn and c Σ ∂k_nn/∂θ. The O(M³) tail and the ∂Kmm contraction follow.
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
constexpr int kChunk = 64;        // columns of the N axis per pass
constexpr int kLd = kSmallM + 1;  // LDS stride of the M x M matrices
constexpr int kLdc = kChunk + 1;  // LDS stride of the M x 64 chunk matrices
constexpr double kJitter = 1e-6;  // gpflow.config.default_jitter()
constexpr int kHdr = 4;           // ints per row header: slot, n, m, 0
constexpr int kScal = 4;          // Σ(y−μ)², Σ k_nn, tr((S − I)Ĝ), info

// per-slot state written by gpx_svgp_small_bind
struct SmallMeta {
  DevSpec spec;
  double scale;  // num_data / n
};

// Packed per-call rows, one per active model, in launch order (row k = block k0 + blockIdx.x):
//   in  [θ 16][Z m·D][q_mu m][q_sqrt m·m]   (compact, the model's own m; row stride in_stride)
//   out [scalars 4][∂θ 16][∂Z m·D][∂q_mu m][∂q_sqrt m·m]
struct SmallArgs {
  const int* hdr;          // [rows][kHdr]
  const SmallMeta* meta;   // [B]
  const double* X;         // [B][Nmax·D]
  const double* Y;         // [B][Nmax]
  const double* in;
  double* out;
  int in_stride, out_stride;
  int Nmax, Mmax, D, k0;
};

struct PredArgs {
  const int* hdr;          // one row
  const SmallMeta* meta;
  const double* in;        // one packed input row
  const double* Xnew;      // [Mn][D]
  double* mean;            // [Mn]
  double* var;             // [Mn]
  int* info;
  int Mn, D, add_noise;
};

// the LDS of one workgroup (doubles). DM <= 8: at most 76.3 KiB, DM = 16: 84.3 KiB
// (profiles/svgp_batch.md).
template <int DM>
struct SmallLds {
  double A[kSmallM * kLd];    // Kmm -> L; in the tail G, then Ĝ·R, then Φ
  double W[kSmallM * kLd];    // L⁻¹
  double S1[kSmallM * kLd];   // S − I
  double P[kSmallM * kLd];    // Wᵀ(S − I)W; in the tail q_sqrt
  double Kc[kSmallM * kLdc];  // the Kmn chunk; prologue: (S − I)W; tail: W·G, then (S − I)Ĝ, then WᵀΦ
  double Yc[kSmallM * kLdc];  // 2c·P·Kc; prologue: q_sqrt; tail: Ĝ, then K̄mm'
  double z[kSmallM * DM];
  double x[kChunk * DM];
  double gz[kSmallM * DM];    // ∂Z accumulated
  double y[kChunk];
  double g[kChunk];           // g_μ of the chunk
  double q[kSmallM], u[kSmallM], w[kSmallM], ah[kSmallM];
  double th[GPX_THETA_STRIDE];
  double red[64];
  double out16[GPX_THETA_STRIDE];
  int info;
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

// What the ELBO and the prediction share: θ, Z, q_mu, q_sqrt into LDS, Kmm = k(Z, Z) + 1e-6 I,
// L = chol(Kmm) in place, W = L⁻¹, u = Wᵀq_mu, S − I, P = Wᵀ(S − I)W. q_sqrt is left in s.Yc
// (stride kLd). A pivot that is not > 0 records its 1-based index in s.info; the arithmetic goes on
// (NaN from there) so that the workgroup's control flow never depends on the data.
template <int DM>
__device__ __forceinline__ void small_prologue(SmallLds<DM>& s, const DevSpec& spec, const double* __restrict__ in, int m, int D,
                               int Mmax) {
  const int tid = threadIdx.x;
  const double* gZ = in + GPX_THETA_STRIDE;
  const double* gq = gZ + (long long)Mmax * D;
  const double* gR = gq + Mmax;
  double* R = s.Yc;
  double* T = s.Kc;
  if (tid < GPX_THETA_STRIDE) s.th[tid] = in[tid];
  for (int e = tid; e < m * D; e += 256) s.z[e] = gZ[e];
  if (tid < kSmallM) s.q[tid] = tid < m ? gq[tid] : 0.0;
  if (tid == 0) s.info = 0;
  for (int e = tid; e < kSmallM * kSmallM; e += 256) {
    const int i = e >> 5, j = e & 31;
    R[i * kLd + j] = (i < m && j <= i) ? gR[i * m + j] : 0.0;
    s.W[i * kLd + j] = (i == j && i >= m) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < kSmallM * kSmallM; e += 256) {
    const int i = e >> 5, j = e & 31;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < m && j <= i) {
      v = eval_k(spec, s.th, s.z + i * D, s.z + j * D);
      if (i == j) v += kJitter;
    } else if (i < m && j < m) {
      v = 0.0;
    }
    s.A[i * kLd + j] = v;
  }
  // right-looking Cholesky of the leading m x m block
  for (int j = 0; j < m; ++j) {
    __syncthreads();
    if (tid == 0) {
      const double p = s.A[j * kLd + j];
      if (!(p > 0.0) && s.info == 0) s.info = j + 1;
      s.A[j * kLd + j] = sqrt(p);
    }
    __syncthreads();
    if (tid > j && tid < m) s.A[tid * kLd + j] /= s.A[j * kLd + j];
    __syncthreads();
    for_mm(m, [&](int i, int k) {
      if (k > j && k <= i) s.A[i * kLd + k] = fma(-s.A[i * kLd + j], s.A[k * kLd + j], s.A[i * kLd + k]);
    });
  }
  __syncthreads();
  // W = L⁻¹, one column per thread, by forward substitution
  if (tid < m) {
    const int j = tid;
    s.W[j * kLd + j] = 1.0 / s.A[j * kLd + j];
    for (int i = j + 1; i < m; ++i) {
      double acc = 0.0;
      for (int k = j; k < i; ++k) acc = fma(s.A[i * kLd + k], s.W[k * kLd + j], acc);
      s.W[i * kLd + j] = -acc / s.A[i * kLd + i];
    }
  }
  // S − I = q_sqrt q_sqrtᵀ − I
  for_mm(m, [&](int i, int j) {
    const int kmax = i < j ? i : j;
    double acc = 0.0;
    for (int k = 0; k <= kmax; ++k) acc = fma(R[i * kLd + k], R[j * kLd + k], acc);
    s.S1[i * kLd + j] = acc - (i == j ? 1.0 : 0.0);
  });
  __syncthreads();
  // u = Wᵀ q_mu;  T = (S − I) W
  if (tid < kSmallM) {
    double acc = 0.0;
    if (tid < m)
      for (int i = tid; i < m; ++i) acc = fma(s.W[i * kLd + tid], s.q[i], acc);
    s.u[tid] = acc;
  }
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = j; k < m; ++k) acc = fma(s.S1[i * kLd + k], s.W[k * kLd + j], acc);
    T[i * kLd + j] = acc;
  });
  __syncthreads();
  // P = Wᵀ T
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = i; k < m; ++k) acc = fma(s.W[k * kLd + i], T[k * kLd + j], acc);
    s.P[i * kLd + j] = acc;
  });
  __syncthreads();
}

// the chunk [c0, c0 + nv) of the column points into LDS; Kc = k(Z, chunk), zero on rows >= m and
// columns >= nv; Yc = alpha·P·Kc
template <int DM>
__device__ __forceinline__ void small_chunk(SmallLds<DM>& s, const DevSpec& spec, const double* __restrict__ X,
                                            int c0, int nv, int m, int D, double alpha) {
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
  double acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.0;
  for (int k = 0; k < m; ++k) {
    const double kv = s.Kc[k * kLdc + lane];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = fma(s.P[(wave + 4 * r) * kLd + k], kv, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = wave + 4 * r;
    s.Yc[i * kLdc + lane] = i < m ? alpha * acc[r] : 0.0;
  }
}

template <int DM, int NT>
__global__ __launch_bounds__(256) void svgp_small_kernel(SmallArgs a) {
  __shared__ SmallLds<DM> s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = a.k0 + blockIdx.x;
  const int* h = a.hdr + row * kHdr;
  const int b = h[0];
  const int n = min(max(h[1], 1), min(a.Nmax, kSmallN));
  const int m = min(max(h[2], 1), min(a.Mmax, kSmallM));
  const int D = a.D;
  const DevSpec spec = a.meta[b].spec;
  const double scale = a.meta[b].scale;
  const double* in = a.in + (long long)row * a.in_stride;
  double* out = a.out + (long long)row * a.out_stride;
  const double* X = a.X + (long long)b * a.Nmax * D;
  const double* Y = a.Y + (long long)b * a.Nmax;

  small_prologue<DM>(s, spec, in, m, D, a.Mmax);
  const double s2 = s.th[spec.n_params];
  const double c2 = -scale / s2;  // 2c
  const double c = 0.5 * c2;
  for (int e = tid; e < kSmallM * DM; e += 256) s.gz[e] = 0.0;
  if (tid < kSmallM) s.w[tid] = 0.0;

  double sums[NT][3];
#pragma unroll
  for (int t = 0; t < NT; ++t) sums[t][0] = sums[t][1] = sums[t][2] = 0.0;
  double gacc[4] = {0.0, 0.0, 0.0, 0.0};  // G entries e = tid + 256 r
  double sq = 0.0, kd = 0.0;              // Σ(y−μ)², Σ k_nn over this thread's columns (wave 0)

  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int nv = min(kChunk, n - c0);
    __syncthreads();  // the previous chunk's readers are done with x, Kc, Yc, g
    if (tid < kChunk) s.y[tid] = tid < nv ? Y[c0 + tid] : 0.0;
    small_chunk<DM>(s, spec, X, c0, nv, m, D, c2);
    // μ, g_μ, the residual and k_nn sums: one column per thread of wave 0
    if (tid < kChunk) {
      double gj = 0.0;
      if (tid < nv) {
        double mu = 0.0;
        for (int i = 0; i < m; ++i) mu = fma(s.Kc[i * kLdc + tid], s.u[i], mu);
        const double rr = s.y[tid] - mu;
        gj = scale * rr / s2;
        sq = fma(rr, rr, sq);
        double dk[NT][3];
        kd += eval_k_grad<NT>(spec, s.th, s.x + tid * D, s.x + tid * D, dk);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          sums[t][0] = fma(c, dk[t][0], sums[t][0]);
          sums[t][1] = fma(c, dk[t][1], sums[t][1]);
          sums[t][2] = fma(c, dk[t][2], sums[t][2]);
        }
      }
      s.g[tid] = gj;
    }
    __syncthreads();
    // K̄mn = u g_μᵀ + Yc contracted with ∂Kmn/∂θ and ∂Kmn/∂Z; w += Kc g_μ
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const int i = wave + 4 * r;
      if (i >= m) break;  // (wave-uniform)
      const bool on = lane < nv;
      const int jj = on ? lane : 0;
      const double gj = s.g[lane];
      const double kb = on ? fma(s.u[i], gj, s.Yc[i * kLdc + lane]) : 0.0;
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
      const double wv = wsum(s.Kc[i * kLdc + lane] * gj);
      if (lane == 0) s.w[i] += wv;
#pragma unroll
      for (int d = 0; d < DM; ++d) {
        const double v = wsum(kb * gzv[d]);
        if (lane == 0 && d < D) s.gz[i * D + d] += v;
      }
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

  // ---- the O(M³) tail ----
  double* G = s.A;
  double* T = s.Kc;
  double* Gh = s.Yc;
  double* R = s.P;
  const double* gR = in + GPX_THETA_STRIDE + (long long)a.Mmax * D + a.Mmax;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = tid + 256 * r;
    const int i = e >> 5, j = e & 31;
    G[i * kLd + j] = (i < m && j < m) ? gacc[r] : 0.0;
    R[i * kLd + j] = (i < m && j <= i) ? gR[i * m + j] : 0.0;
  }
  const double ssq = wsum(sq), skd = wsum(kd);
  if (tid == 0) { s.red[0] = ssq; s.red[1] = skd; }
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
  // X1 = (S − I) Ĝ (over T);  GR = Ĝ q_sqrt (over G);  tr((S − I) Ĝ)
  double* X1 = T;
  double* GR = G;
  double tr = 0.0;
  for_mm(m, [&](int i, int j) {
    double acc = 0.0, acc2 = 0.0;
    for (int k = 0; k < m; ++k) acc = fma(s.S1[i * kLd + k], Gh[k * kLd + j], acc);
    for (int k = j; k < m; ++k) acc2 = fma(Gh[i * kLd + k], R[k * kLd + j], acc2);
    X1[i * kLd + j] = acc;
    GR[i * kLd + j] = acc2;
    tr = fma(s.S1[i * kLd + j], Gh[i * kLd + j], tr);
  });
  tr = wsum(tr);
  if (lane == 0) s.red[8 + wave] = tr;
  __syncthreads();
  // outputs ∂q_mu, ∂q_sqrt, the scalars;  Φ over GR's buffer once GR is consumed
  double* oth = out + kScal;
  double* oZ = oth + GPX_THETA_STRIDE;
  double* oq = oZ + (long long)a.Mmax * D;
  double* oR = oq + a.Mmax;
  if (tid < m) oq[tid] = s.ah[tid] - s.q[tid];
  if (tid == 0) {
    out[0] = s.red[0];
    out[1] = s.red[1];
    out[2] = (s.red[8] + s.red[9]) + (s.red[10] + s.red[11]);
    out[3] = (double)s.info;
  }
  double phi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = tid + 256 * r;
    const int i = e >> 5, j = e & 31;
    phi[r] = 0.0;
    if (i < m && j < m) {
      double rb = 0.0;
      if (j <= i) {
        const double F = -(s.q[i] * s.ah[j] + c2 * X1[i * kLd + j]);
        phi[r] = (i == j) ? 0.5 * F : F;
        const double rv = R[i * kLd + j];
        rb = c2 * GR[i * kLd + j] - rv + ((i == j) ? 1.0 / rv : 0.0);
      }
      oR[i * m + j] = rb;
    }
  }
  __syncthreads();
  double* Phi = G;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = tid + 256 * r;
    Phi[(e >> 5) * kLd + (e & 31)] = phi[r];
  }
  __syncthreads();
  // T2 = Wᵀ Φ (over X1);  K̄mm' = T2 W (over Ĝ)
  double* T2 = T;
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = (i > j ? i : j); k < m; ++k) acc = fma(s.W[k * kLd + i], Phi[k * kLd + j], acc);
    T2[i * kLd + j] = acc;
  });
  __syncthreads();
  double* Sb = Gh;
  for_mm(m, [&](int i, int j) {
    double acc = 0.0;
    for (int k = j; k < m; ++k) acc = fma(T2[i * kLd + k], s.W[k * kLd + j], acc);
    Sb[i * kLd + j] = acc;
  });
  __syncthreads();
  // sym(K̄mm') contracted with ∂Kmm/∂θ and ∂Kmm/∂Z (symmetric: factor 2 on Z)
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

// predict_f / predict_y of one slot at Mn points, 64 per workgroup:
//   mean = Kmsᵀ u,  var = k** + Σ_m Kms ∘ (P·Kms) (+σ²)
template <int DM>
__global__ __launch_bounds__(256) void svgp_small_predict_kernel(PredArgs a) {
  __shared__ SmallLds<DM> s;
  const int tid = threadIdx.x;
  const int b = a.hdr[0];
  const int m = min(max(a.hdr[2], 1), kSmallM);
  const int D = a.D;
  const DevSpec spec = a.meta[b].spec;
  small_prologue<DM>(s, spec, a.in, m, D, m);
  if (blockIdx.x == 0 && tid == 0) a.info[0] = s.info;
  const int c0 = blockIdx.x * kChunk;
  const int nv = min(kChunk, a.Mn - c0);
  small_chunk<DM>(s, spec, a.Xnew, c0, nv, m, D, 1.0);
  __syncthreads();
  if (tid < nv) {
    double mu = 0.0, v = 0.0;
    for (int i = 0; i < m; ++i) {
      const double kv = s.Kc[i * kLdc + tid];
      mu = fma(kv, s.u[i], mu);
      v = fma(kv, s.Yc[i * kLdc + tid], v);
    }
    v += eval_kdiag(spec, s.th, s.x + tid * D);
    if (a.add_noise) v += s.th[spec.n_params];
    a.mean[c0 + tid] = mu;
    a.var[c0 + tid] = v;
  }
}

int dm_of(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : 16; }

template <int NT>
void launch_small_nt(const SmallArgs& a, int nblocks, hipStream_t s) {
  const dim3 grid(nblocks), block(256);
  switch (dm_of(a.D)) {
    case 1: hipLaunchKernelGGL((svgp_small_kernel<1, NT>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((svgp_small_kernel<2, NT>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((svgp_small_kernel<4, NT>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((svgp_small_kernel<8, NT>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((svgp_small_kernel<16, NT>), grid, block, 0, s, a); break;
  }
}

void launch_small_predict(const PredArgs& a, hipStream_t s) {
  const dim3 grid((a.Mn + kChunk - 1) / kChunk), block(256);
  switch (dm_of(a.D)) {
    case 1: hipLaunchKernelGGL((svgp_small_predict_kernel<1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((svgp_small_predict_kernel<2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((svgp_small_predict_kernel<4>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((svgp_small_predict_kernel<8>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((svgp_small_predict_kernel<16>), grid, block, 0, s, a); break;
  }
}

}  // namespace

struct gpx_svgp_small {
  gpx_ctx* ctx = nullptr;
  int B = 0, Nmax = 0, Mmax = 0, D = 0;
  int in_stride = 0, out_stride = 0;  // doubles per packed row
  std::vector<int> n, m;              // per slot; n = 0: not bound
  std::vector<gpx_kernel_spec> specs;
  std::vector<double> num_data;
  double *dX = nullptr, *dY = nullptr;
  SmallMeta* d_meta = nullptr;
  // one device block and its pinned mirror per direction: [hdr B·4 ints][B packed input rows] up,
  // [B packed output rows] down
  char *d_in = nullptr, *h_in = nullptr;
  double *d_out = nullptr, *h_out = nullptr;
  size_t hdr_bytes = 0;
  // predict: grow-only [Xnew Mn·D] up and [mean Mn][var Mn][info] down
  double *d_px = nullptr, *h_px = nullptr, *d_po = nullptr, *h_po = nullptr;
  size_t px_cap = 0, po_cap = 0;
  std::vector<int> order;  // the call's launch order (positions into `active`)
};

namespace {

const char* kArdMsg = "ARD terms (GPX_TERM_ARD) are served by the gpx_batch_* entry points only";

// the θ / Z / q_sqrt checks of gpx_svgp.hip's prelude for one slot's rows
int check_row(gpx_ctx* ctx, const gpx_kernel_spec& spec, int m, int D, const double* theta, const double* Z,
              const double* q_mu, const double* q_sqrt) {
  for (int p = 0; p <= spec.n_params; ++p)
    if (!(theta[p] > 0.0) || !std::isfinite(theta[p]))
      return fail(ctx, GPX_BAD_ARG, "theta must be finite and > 0 (constrained space)");
  for (int e = 0; e < m * D; ++e)
    if (!std::isfinite(Z[e])) return fail(ctx, GPX_BAD_ARG, "Z must be finite");
  (void)q_mu;
  for (int i = 0; i < m; ++i)
    if (!(q_sqrt[(size_t)i * m + i] != 0.0)) return fail(ctx, GPX_BAD_ARG, "q_sqrt has a zero diagonal");
  return GPX_OK;
}

// one packed input row: [θ 16][Z m·D][q_mu m][q_sqrt m·m], the rest of the row untouched
void pack_row(const gpx_svgp_small* sm, int m, const double* theta, const double* Z, const double* q_mu,
              const double* q_sqrt, double* row) {
  std::memcpy(row, theta, sizeof(double) * GPX_THETA_STRIDE);
  double* z = row + GPX_THETA_STRIDE;
  std::memcpy(z, Z, sizeof(double) * m * sm->D);
  double* q = z + (size_t)sm->Mmax * sm->D;
  std::memcpy(q, q_mu, sizeof(double) * m);
  std::memcpy(q + sm->Mmax, q_sqrt, sizeof(double) * m * m);
}

}  // namespace

extern "C" {

int gpx_svgp_small_limits(int* m_max, int* n_max) {
  if (!m_max || !n_max) return GPX_BAD_ARG;
  *m_max = kSmallM;
  *n_max = kSmallN;
  return GPX_OK;
}

int gpx_svgp_small_destroy(gpx_svgp_small* sm) {
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

int gpx_svgp_small_create(gpx_ctx* ctx, int B, int N_max, int M_max, int D, gpx_svgp_small** out) {
  if (!ctx || !out) return GPX_BAD_ARG;
  *out = nullptr;
  if (B < 1 || N_max < 1 || M_max < 1 || D < 1)
    return fail(ctx, GPX_BAD_ARG, "bad svgp_small dimensions");
  if (M_max > kSmallM || N_max > kSmallN || D > GPX_MAX_DIM)
    return fail(ctx, GPX_BAD_ARG, "shape over the fused small-shape limits (M <= 32, N <= 4096, D <= 16)");
  HIPX(ctx, hipSetDevice(ctx->device));
  gpx_svgp_small* sm = new gpx_svgp_small();
  sm->ctx = ctx; sm->B = B; sm->Nmax = N_max; sm->Mmax = M_max; sm->D = D;
  const int body = M_max * D + M_max + M_max * M_max;
  sm->in_stride = GPX_THETA_STRIDE + body;
  sm->out_stride = kScal + GPX_THETA_STRIDE + body;
  sm->n.assign(B, 0);
  sm->m.assign(B, 0);
  sm->specs.resize(B);
  sm->num_data.assign(B, 0.0);
  sm->hdr_bytes = ((size_t)B * kHdr * sizeof(int) + 15) / 16 * 16;
  const size_t in_bytes = sm->hdr_bytes + sizeof(double) * (size_t)B * sm->in_stride;
  const size_t out_bytes = sizeof(double) * (size_t)B * sm->out_stride;
  if (hipMalloc(&sm->dX, sizeof(double) * (size_t)B * N_max * D) != hipSuccess ||
      hipMalloc(&sm->dY, sizeof(double) * (size_t)B * N_max) != hipSuccess ||
      hipMalloc(&sm->d_meta, sizeof(SmallMeta) * B) != hipSuccess ||
      hipMalloc(&sm->d_in, in_bytes) != hipSuccess || hipMalloc(&sm->d_out, out_bytes) != hipSuccess ||
      hipMemset(sm->dX, 0, sizeof(double) * (size_t)B * N_max * D) != hipSuccess ||
      hipMemset(sm->dY, 0, sizeof(double) * (size_t)B * N_max) != hipSuccess ||
      hipMemset(sm->d_meta, 0, sizeof(SmallMeta) * B) != hipSuccess ||
      hipMemset(sm->d_in, 0, in_bytes) != hipSuccess || hipMemset(sm->d_out, 0, out_bytes) != hipSuccess) {
    gpx_svgp_small_destroy(sm);
    return fail(ctx, GPX_HIP_ERROR, "out of device memory");
  }
  if (hipHostMalloc(&sm->h_in, in_bytes, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(&sm->h_out, out_bytes, hipHostMallocDefault) != hipSuccess) {
    gpx_svgp_small_destroy(sm);
    return fail(ctx, GPX_HIP_ERROR, "out of pinned host memory");
  }
  std::memset(sm->h_in, 0, in_bytes);
  std::memset(sm->h_out, 0, out_bytes);
  *out = sm;
  return GPX_OK;
}

int gpx_svgp_small_bind(gpx_svgp_small* sm, int b, int n, int m, const double* X, const double* Y,
                        const gpx_kernel_spec* spec, double num_data) {
  if (!sm) return GPX_BAD_ARG;
  gpx_ctx* ctx = sm->ctx;
  if (b < 0 || b >= sm->B || !X || !Y || !spec || n < 1 || m < 1 || !(num_data > 0.0) || !std::isfinite(num_data))
    return fail(ctx, GPX_BAD_ARG, "bad svgp_small bind arguments");
  if (n > sm->Nmax || m > sm->Mmax)
    return fail(ctx, GPX_BAD_ARG, "model larger than the object's N_max / M_max");
  if (ard_spec(*spec)) return fail(ctx, GPX_BAD_ARG, kArdMsg);
  if (coreg_spec(*spec)) return fail(ctx, GPX_BAD_ARG, kCoregBatchOnlyMsg);
  if (const char* why = spec_error(*spec, sm->D)) return fail(ctx, GPX_BAD_ARG, why);
  HIPX(ctx, hipSetDevice(ctx->device));
  SmallMeta meta;
  static_assert(sizeof(DevSpec) == sizeof(gpx_kernel_spec), "spec layout");
  std::memcpy(&meta.spec, spec, sizeof(DevSpec));
  meta.scale = num_data / (double)n;
  HIPX(ctx, hipMemcpy(sm->dX + (size_t)b * sm->Nmax * sm->D, X, sizeof(double) * (size_t)n * sm->D,
                      hipMemcpyHostToDevice));
  HIPX(ctx, hipMemcpy(sm->dY + (size_t)b * sm->Nmax, Y, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPX(ctx, hipMemcpy(sm->d_meta + b, &meta, sizeof(SmallMeta), hipMemcpyHostToDevice));
  sm->n[b] = n;
  sm->m[b] = m;
  sm->specs[b] = *spec;
  sm->num_data[b] = num_data;
  return GPX_OK;
}

int gpx_svgp_small_elbo_grad(gpx_svgp_small* sm, int n_active, const int32_t* active, const double* theta,
                             const double* Z, const double* q_mu, const double* q_sqrt, double* elbo,
                             double* grad_theta, double* grad_Z, double* grad_q_mu, double* grad_q_sqrt,
                             int32_t* info, void* stream) {
  if (!sm) return GPX_BAD_ARG;
  gpx_ctx* ctx = sm->ctx;
  if (n_active < 0 || n_active > sm->B || (n_active > 0 && !active) || !theta || !Z || !q_mu || !q_sqrt ||
      !elbo || !grad_theta || !grad_Z || !grad_q_mu || !grad_q_sqrt || !info)
    return fail(ctx, GPX_BAD_ARG, "null svgp_small argument or bad active count");
  if (n_active == 0) return GPX_OK;
  const int B = sm->B, D = sm->D, Mx = sm->Mmax;
  const size_t sZ = (size_t)Mx * D, sR = (size_t)Mx * Mx;
  std::vector<char> seen(B, 0);
  for (int k = 0; k < n_active; ++k) {
    const int b = active[k];
    if (b < 0 || b >= B || seen[b] || sm->n[b] == 0)
      return fail(ctx, GPX_BAD_ARG, "active slot out of range, repeated or not bound");
    seen[b] = 1;
    const int rc = check_row(ctx, sm->specs[b], sm->m[b], D, theta + (size_t)b * GPX_THETA_STRIDE, Z + b * sZ,
                             q_mu + (size_t)b * Mx, q_sqrt + b * sR);
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
    pack_row(sm, sm->m[b], theta + (size_t)b * GPX_THETA_STRIDE, Z + b * sZ, q_mu + (size_t)b * Mx,
             q_sqrt + b * sR, rows + (size_t)r * sm->in_stride);
  }
  const size_t up = sm->hdr_bytes + sizeof(double) * (size_t)n_active * sm->in_stride;
  HIPX(ctx, hipMemcpyAsync(sm->d_in, sm->h_in, up, hipMemcpyHostToDevice, s));
  SmallArgs a{};
  a.hdr = reinterpret_cast<const int*>(sm->d_in);
  a.meta = sm->d_meta; a.X = sm->dX; a.Y = sm->dY;
  a.in = reinterpret_cast<const double*>(sm->d_in + sm->hdr_bytes);
  a.out = sm->d_out; a.in_stride = sm->in_stride; a.out_stride = sm->out_stride;
  a.Nmax = sm->Nmax; a.Mmax = Mx; a.D = D;
  if (n1 > 0) {
    a.k0 = 0;
    launch_small_nt<1>(a, n1, s);
  }
  if (n_active > n1) {
    a.k0 = n1;
    launch_small_nt<GPX_MAX_TERMS>(a, n_active - n1, s);
  }
  HIPX(ctx, hipGetLastError());
  HIPX(ctx, hipMemcpyAsync(sm->h_out, sm->d_out, sizeof(double) * (size_t)n_active * sm->out_stride,
                           hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  int bad = 0;
  for (int r = 0; r < n_active; ++r) {
    const int b = active[sm->order[r]];
    const int n = sm->n[b], m = sm->m[b], np = sm->specs[b].n_params;
    const double* o = sm->h_out + (size_t)r * sm->out_stride;
    const double* oth = o + kScal;
    const double* oZ = oth + GPX_THETA_STRIDE;
    const double* oq = oZ + sZ;
    const double* oR = oq + Mx;
    const double* th = theta + (size_t)b * GPX_THETA_STRIDE;
    const double* q = q_mu + (size_t)b * Mx;
    const double* R = q_sqrt + b * sR;
    const double s2 = th[np], scale = sm->num_data[b] / (double)n, ntot = (double)n;
    const double sumv = o[1] + o[2];
    double kl = -m;
    for (int i = 0; i < m; ++i) {
      kl += q[i] * q[i];
      for (int j = 0; j <= i; ++j) kl += R[(size_t)i * m + j] * R[(size_t)i * m + j];
      kl -= std::log(R[(size_t)i * m + i] * R[(size_t)i * m + i]);
    }
    kl *= 0.5;
    elbo[b] = scale * (-0.5 * ntot * std::log(2.0 * M_PI * s2) - (o[0] + sumv) / (2.0 * s2)) - kl;
    double* gth = grad_theta + (size_t)b * GPX_THETA_STRIDE;
    for (int p = 0; p < GPX_THETA_STRIDE; ++p) gth[p] = p < np ? oth[p] : 0.0;
    gth[np] = scale * (-0.5 * ntot / s2 + 0.5 * (o[0] + sumv) / (s2 * s2));
    std::memcpy(grad_Z + b * sZ, oZ, sizeof(double) * m * D);
    std::memcpy(grad_q_mu + (size_t)b * Mx, oq, sizeof(double) * m);
    std::memcpy(grad_q_sqrt + b * sR, oR, sizeof(double) * m * m);
    info[b] = (int32_t)o[3];
    if (info[b] != 0) ++bad;
  }
  if (bad) return fail(ctx, GPX_NOT_PD, "Kmm + jitter I is not positive definite");
  return GPX_OK;
}

int gpx_svgp_small_predict(gpx_svgp_small* sm, int b, const double* theta, const double* Z, const double* q_mu,
                           const double* q_sqrt, const double* Xnew, int Mn, int add_noise, double* mean,
                           double* var, int32_t* info, void* stream) {
  if (!sm) return GPX_BAD_ARG;
  gpx_ctx* ctx = sm->ctx;
  if (b < 0 || b >= sm->B || sm->n[b] == 0) return fail(ctx, GPX_BAD_ARG, "slot out of range or not bound");
  if (!theta || !Z || !q_mu || !q_sqrt || !Xnew || Mn < 1 || !mean || !var)
    return fail(ctx, GPX_BAD_ARG, "bad predict args");
  const int D = sm->D, m = sm->m[b];
  int rc = check_row(ctx, sm->specs[b], m, D, theta, Z, q_mu, q_sqrt);
  if (rc != GPX_OK) return rc;
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // up: [hdr 4 ints, padded to 16 B][θ 16][Z m·D][q m][q_sqrt m·m][Xnew Mn·D];  down: [mean][var][info]
  const size_t row = GPX_THETA_STRIDE + (size_t)m * D + m + (size_t)m * m;
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
  std::memcpy(r + GPX_THETA_STRIDE + (size_t)m * D, q_mu, sizeof(double) * m);
  std::memcpy(r + GPX_THETA_STRIDE + (size_t)m * D + m, q_sqrt, sizeof(double) * m * m);
  std::memcpy(r + row, Xnew, sizeof(double) * (size_t)Mn * D);
  HIPX(ctx, hipMemcpyAsync(sm->d_px, sm->h_px, sizeof(double) * up, hipMemcpyHostToDevice, s));
  PredArgs a{};
  a.hdr = reinterpret_cast<const int*>(sm->d_px);
  a.meta = sm->d_meta;
  a.in = sm->d_px + 2;
  a.Xnew = sm->d_px + 2 + row;
  a.mean = sm->d_po;
  a.var = sm->d_po + Mn;
  a.info = reinterpret_cast<int*>(sm->d_po + 2 * (size_t)Mn);
  a.Mn = Mn; a.D = D; a.add_noise = add_noise ? 1 : 0;
  launch_small_predict(a, s);
  HIPX(ctx, hipGetLastError());
  HIPX(ctx, hipMemcpyAsync(sm->h_po, sm->d_po, sizeof(double) * down, hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  std::memcpy(mean, sm->h_po, sizeof(double) * Mn);
  std::memcpy(var, sm->h_po + Mn, sizeof(double) * Mn);
  const int inf = *reinterpret_cast<const int*>(sm->h_po + 2 * (size_t)Mn);
  if (info) *info = inf;
  if (inf != 0) return fail(ctx, GPX_NOT_PD, "Kmm + jitter I is not positive definite");
  return GPX_OK;
}

}  // extern "C"
