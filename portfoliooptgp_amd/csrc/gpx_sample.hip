// gpx_sample.hip — batched multivariate-normal sampler (GPflow's sample_mvn(full_cov=True) arithmetic):
//   A = cov + jitter·I,  L = chol(A) (lower),  out[s] = mean + L · white[s].
// One algorithm for every M: a right-looking Cholesky in blocks of 64 over a workspace padded to a
// multiple of 64 with an identity diagonal (padded pivots are 1, padded panel rows 0). Per block
// step one workgroup per problem factors the 64x64 diagonal block in LDS and solves the panel
// below it by forward substitution, one panel row per thread (sample_step_kernel); the trailing
// update A22 −= L21·L21ᵀ is the library's batched fp64 MFMA GEMM on lower tiles. L·whiteᵀ is one
// more GEMM of that kind with the triangular k range, and a small kernel adds the mean. M <= 64 is
// a single factor launch.
//
// Why substitution and not the explicit inverse the dense route's leaf forms (L21 = A21·W11ᵀ): the
// inverse puts κ(L11) into the panel's residual, and the factor here is held to Higham's
// componentwise bound |LLᵀ − A|_ij <= c·(M+1)·u·sqrt(A_ii A_jj), which substitution meets whatever
// the conditioning. The panel is O(M·64²/2) per step against the trailing update's O(M²·64).
//
// A problem's bits depend on its own inputs only: every sum runs in a fixed order (the diagonal
// block and the panel sequentially in k, the GEMMs in 4-wide MFMA chunks ascending in k, which
// gemm()'s tile choice does not change), sample s is row s of the product, and a failed problem
// (first pivot that is not > 0 and finite: info, 1-based) skips its later steps and its output.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>
#include "gpx_host.h"
#include "gpx_leaf.h"

using namespace gpx;

namespace gpx {

constexpr int kSB = 64;   // block size of the factorisation
constexpr int kSS = 65;   // LDS row stride of the diagonal block: lane = row reads are conflict-free
constexpr int kST = 66;   // ... of its transpose (even: the panel's reads of consecutive m pair up)
typedef double sd2 __attribute__((ext_vector_type(2)));

// idx[i] = i: the active list of a call over caller-owned buffers (gpx_sample_mvn)
__global__ void sample_iota_kernel(int* idx, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = i;
}

// Row r of a problem's padded images: rows [0, Mp) of A = tril(cov) + jitter·I (zeros above the
// diagonal, the identity beyond M), rows [Mp, Mp + Sp) of the zero-padded white. Elementwise, so A
// may be cov itself (ldc == Mp).
__global__ __launch_bounds__(256) void sample_load_kernel(SampleArgs a) {
  const int rows = a.Mp + a.Sp;
  const int pa = blockIdx.x / rows, r = blockIdx.x % rows;
  const int b = a.active[pa];
  const int tid = threadIdx.x;
  if (r == 0 && tid == 0) a.info[b] = 0;
  if (r < a.Mp) {
    const double* cov = a.cov + (long long)b * a.sCov;
    double* A = a.A + (long long)b * a.sA;
    for (int c = tid; c < a.Mp; c += 256) {
      double v = (r == c) ? 1.0 : 0.0;
      if (r < a.M && c <= r) {
        v = cov[(long long)r * a.ldc + c];
        if (c == r) v += a.jitter;
      }
      A[(long long)r * a.Mp + c] = v;
    }
  } else {
    const int s = r - a.Mp;
    const double* w = a.white + (long long)b * a.sWhite;
    double* Wp = a.Wp + (long long)b * a.sW;
    for (int c = tid; c < a.Mp; c += 256)
      Wp[(long long)s * a.Mp + c] = (s < a.S && c < a.M) ? w[(long long)s * a.M + c] : 0.0;
  }
}

// Cholesky of the lower 64x64 block in sA (row stride kSS), in place: L with zeros above the
// diagonal. Sixteen columns at a time: wave 0 holds row `lane`'s sixteen entries in registers and
// runs the column steps with lane broadcasts (correctly rounded sqrt and division), then all four
// waves apply the sixteen columns to the rest of the block. *sfail (-1 on entry) gets the first
// pivot that is not > 0 and finite (0-based). 256 threads; ends with a barrier.
__device__ __forceinline__ void chol64_lds(double* __restrict__ sA, int* sfail) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
  for (int cb = 0; cb < kSB / 16; ++cb) {
    const int c0 = cb * 16;
    if (wave == 0) {
      double r[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) r[k] = sA[lane * kSS + c0 + k];
      int fail = -1;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double piv = readlane_d(r[j], c0 + j);
        if (!(piv > 0.0 && piv < INFINITY) && fail < 0) fail = c0 + j;
        const double ljj = sqrt(piv);
        const double q = r[j] / ljj;
        r[j] = (lane > c0 + j) ? q : ((lane == c0 + j) ? ljj : 0.0);
#pragma unroll
        for (int k = j + 1; k < 16; ++k) r[k] = fma(-r[j], readlane_d(r[j], c0 + k), r[k]);
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) sA[lane * kSS + c0 + k] = r[k];
      if (lane == 0 && fail >= 0 && *sfail < 0) *sfail = fail;
    }
    __syncthreads();
    // A_ik −= Σ_j L_ij L_kj over the sixteen columns, rows i and columns k <= i beyond them
    const int t0 = c0 + 16, n = kSB - t0;
    for (int e = tid; e < n * n; e += 256) {
      const int i = t0 + e / n, k = t0 + e % n;
      if (k <= i) {
        double acc = sA[i * kSS + k];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = fma(-sA[i * kSS + c0 + j], sA[k * kSS + c0 + j], acc);
        sA[i * kSS + k] = acc;
      }
    }
    __syncthreads();
  }
}

// One block step at offset o of every listed problem: L11 = chol(A11) in LDS, written back with
// zeros above the diagonal and over the rest of its block row (a 128-tile trailing update of an
// earlier step writes its diagonal tiles whole, and the product GEMM reads that block row up to
// its tile's edge); then the panel rows below, X·L11ᵀ = A21 by forward substitution, one row per
// thread in registers, L11 read from its transposed LDS image (the same address across a wave).
__global__ __launch_bounds__(256) void sample_step_kernel(SampleArgs a, int o) {
  __shared__ __attribute__((aligned(16))) double sA[kSB * kSS];
  __shared__ __attribute__((aligned(16))) double sT[kSB * kST];
  __shared__ int sfail;
  const int b = a.active[blockIdx.x];
  if (a.info[b] != 0) return;  // an earlier step failed: nothing more is computed for this problem
  const int tid = threadIdx.x, Mp = a.Mp;
  double* A = a.A + (long long)b * a.sA;
  for (int e = tid; e < kSB * kSB; e += 256) {
    const int r = e >> 6, c = e & 63;
    sA[r * kSS + c] = (c <= r) ? A[(long long)(o + r) * Mp + o + c] : 0.0;
  }
  if (tid == 0) sfail = -1;
  __syncthreads();
  chol64_lds(sA, &sfail);
  if (sfail >= 0) {
    if (tid == 0) a.info[b] = o + sfail + 1;
    return;
  }
  for (int e = tid; e < kSB * kSB; e += 256) {
    const int r = e >> 6, c = e & 63;
    const double v = sA[r * kSS + c];
    A[(long long)(o + r) * Mp + o + c] = v;
    sT[c * kST + r] = v;
  }
  const int right = Mp - o - kSB;
  for (int e = tid; e < kSB * right; e += 256) {
    const int r = e / right, c = e - r * right;
    A[(long long)(o + r) * Mp + o + kSB + c] = 0.0;
  }
  __syncthreads();
#pragma unroll 1
  for (int r0 = o + kSB; r0 < Mp; r0 += 256) {
    const int row = r0 + tid;
    if (row >= Mp) continue;
    sd2* p = reinterpret_cast<sd2*>(A + (long long)row * Mp + o);
    double x[kSB];
#pragma unroll
    for (int q = 0; q < kSB / 2; ++q) {
      const sd2 v = p[q];
      x[2 * q] = v.x;
      x[2 * q + 1] = v.y;
    }
#pragma unroll
    for (int k = 0; k < kSB; ++k) {
      x[k] = x[k] / sT[k * kST + k];
      // column k's reads wait for x_k (else all 2016 are hoisted: every register and scratch)
      int ck = k * kST;
      asm volatile("" : "+v"(ck) : "v"(x[k]));
#pragma unroll
      for (int m = k + 1; m < kSB; ++m) x[m] = fma(-x[k], sT[ck + m], x[m]);
    }
#pragma unroll
    for (int q = 0; q < kSB / 2; ++q) p[q] = (sd2){x[2 * q], x[2 * q + 1]};
  }
}

// out[b][s][i] = mean[b][i] + P[b][s][i] for the problems whose factorisation succeeded
__global__ __launch_bounds__(256) void sample_out_kernel(SampleArgs a) {
  const int pa = blockIdx.x / a.S, s = blockIdx.x % a.S;
  const int b = a.active[pa];
  if (a.info[b] != 0) return;
  const double* P = a.P + (long long)b * a.sW + (long long)s * a.Mp;
  const double* mean = a.mean + (long long)b * a.sMean;
  double* out = a.out + (long long)b * a.sOut + (long long)s * a.M;
  for (int i = threadIdx.x; i < a.M; i += 256) out[i] = mean[i] + P[i];
}

void launch_sample_iota(int* idx, int n, hipStream_t s) {
  hipLaunchKernelGGL(sample_iota_kernel, dim3((n + 255) / 256), dim3(256), 0, s, idx, n);
}

void launch_sample_chain(const SampleArgs& a, int na, hipStream_t s) {
  const int Mp = a.Mp, Sp = a.Sp;
  hipLaunchKernelGGL(sample_load_kernel, dim3((unsigned)na * (Mp + Sp)), dim3(256), 0, s, a);
  for (int o = 0; o < Mp; o += kSB) {
    hipLaunchKernelGGL(sample_step_kernel, dim3(na), dim3(256), 0, s, a, o);
    const int n2 = Mp - o - kSB;
    if (n2 <= 0) break;
    // A22 −= L21 · L21ᵀ (lower tiles; the tile size as gemm() picks it for store GEMMs)
    const double* l21 = a.A + (long long)(o + kSB) * Mp + o;
    GemmArgs g = gemm_args(l21, Mp, l21, Mp, a.A + (long long)(o + kSB) * Mp + o + kSB, Mp, a.sA, n2, n2, kSB, 0,
                           1, -1.0, 1.0);
    g.active = a.active;
    g.small_tiles = 1;
    launch_gemm(g, EPI_STORE, false, true, na, s);
  }
  // P[s][i] = Σ_{k<=i} white[s][k] L[i][k]  (opB(k, j) = L[j][k], zero for k > j)
  GemmArgs g = gemm_args(a.Wp, Mp, a.A, Mp, a.P, Mp, 0, Sp, Mp, Mp, TRI_KMAX_J, 0, 1.0, 0.0);
  g.sA = a.sW; g.sB = a.sA; g.sC = a.sW;
  g.active = a.active;
  g.small_tiles = 1;
  launch_gemm(g, EPI_STORE, false, true, na, s);
  hipLaunchKernelGGL(sample_out_kernel, dim3((unsigned)na * a.S), dim3(256), 0, s, a);
}

}  // namespace gpx

extern "C" {

int gpx_sample_limits(int* m_max) {
  if (!m_max) return GPX_BAD_ARG;
  *m_max = kSampleMaxM;
  return GPX_OK;
}

int gpx_sample_mvn(gpx_ctx* ctx, int B, int M, int S, const double* mean, const double* cov, const double* white,
                   double jitter, double* out, int32_t* info, void* stream) {
  if (!ctx) return GPX_BAD_ARG;
  if (!mean || !cov || !white || !out || !info) return fail(ctx, GPX_BAD_ARG, "gpx_sample_mvn: null pointer");
  if (B <= 0 || M <= 0 || S <= 0) return fail(ctx, GPX_BAD_ARG, "gpx_sample_mvn: B, M and S must be positive");
  if (M > kSampleMaxM) return fail(ctx, GPX_BAD_ARG, "gpx_sample_mvn: M over the limit (gpx_sample_limits)");
  if (!(jitter >= 0.0) || !std::isfinite(jitter))
    return fail(ctx, GPX_BAD_ARG, "gpx_sample_mvn: jitter must be finite and >= 0");
  const long long Mp = ((long long)M + 63) / 64 * 64, Sp = ((long long)S + 63) / 64 * 64;
  if ((long long)B * (Mp + Sp) > 0x7fffffffLL)
    return fail(ctx, GPX_BAD_ARG, "gpx_sample_mvn: too many problems x rows for one call: split it");
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  gpx_sample_ws* w = &ctx->sample;
  std::lock_guard<std::mutex> lock(w->mu);
  const size_t per = (size_t)(Mp * Mp + 2 * Sp * Mp);
  {
    const int e = ensure(ctx, w->ws, w->cap, per * B);
    if (e != GPX_OK) return e;
  }
  if (w->icap < (size_t)2 * B) {
    if (w->idx) (void)hipFree(w->idx);
    w->idx = nullptr; w->icap = 0;
    HIPX(ctx, hipMalloc(&w->idx, sizeof(int) * 2 * B));
    w->icap = (size_t)2 * B;
  }
  SampleArgs a{};
  a.active = w->idx;
  a.cov = cov; a.sCov = (long long)M * M; a.ldc = M;
  a.white = white; a.sWhite = (long long)S * M;
  a.mean = mean; a.sMean = M;
  a.out = out; a.sOut = (long long)S * M;
  a.A = w->ws; a.sA = (long long)per;
  a.Wp = w->ws + Mp * Mp; a.P = a.Wp + Sp * Mp; a.sW = (long long)per;
  a.info = w->idx + B;
  a.M = M; a.S = S; a.Mp = (int)Mp; a.Sp = (int)Sp; a.jitter = jitter;
  launch_sample_iota(w->idx, B, s);
  launch_sample_chain(a, B, s);
  HIPX(ctx, hipGetLastError());
  std::vector<int> h(B);
  HIPX(ctx, hipMemcpyAsync(h.data(), a.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  int status = GPX_OK;
  for (int b = 0; b < B; ++b) {
    info[b] = h[b];
    if (h[b] != 0) status = GPX_NOT_PD;
  }
  if (status == GPX_NOT_PD) last_error_slot() = "the covariance + jitter*I is not positive definite for some problem";
  return status;
}

}  // extern "C"
