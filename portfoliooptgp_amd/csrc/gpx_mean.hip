// gpx_mean.hip — parametric mean functions on the device (gpx_batch_set_mean): the residual
// r = y − m(X; β) every evaluation route factorises and solves against, ∂logML/∂β = Φᵀα from the
// route's α, and m(X*) added to a prediction's mean. The factorisation kernels are unchanged: they
// read r where they read y (eval_y) and leave α in the batch's α vectors as before.
//
// All three kernels evaluate m through gpx_mean.h (one evaluation order, no pow), so a problem's
// bits depend on its own data and β only — never on what shares its call.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "gpx_host.h"
#include "gpx_mean.h"

namespace gpx {

namespace {
constexpr int kMeanBlock = 256;

// r_j = y_j − m(x_j; β_b) for j < n[b], zero beyond (rows = N_max). A zero-mean slot's y is copied:
// the routes of a batch with any mean read every problem's targets here.
__global__ __launch_bounds__(kMeanBlock) void mean_resid_kernel(MeanArgs a, int nblk) {
  const int b = a.active[blockIdx.x / nblk];
  const int j = (blockIdx.x % nblk) * kMeanBlock + threadIdx.x;
  if (j >= a.rows) return;
  const DevMean m = a.means[b];
  const int n = a.nvalid[b];
  double r = 0.0;
  if (j < n) {
    r = a.Y[(long long)b * a.sY + j];
    if (m.kind != GPX_MEAN_ZERO)
      r = r - mean_eval(m.kind, m.n_coef, a.theta + (long long)b * GPX_THETA_STRIDE + m.off,
                        a.X + (long long)b * a.sX + (long long)j * a.D, a.D);
  }
  a.out[(long long)b * a.sOut + j] = r;
}

// mean[b][i] += m(Xnew[b][i]; β_b), i < rows (= M)
__global__ __launch_bounds__(kMeanBlock) void mean_add_kernel(MeanArgs a, int nblk) {
  const int b = a.active[blockIdx.x / nblk];
  const int i = (blockIdx.x % nblk) * kMeanBlock + threadIdx.x;
  const DevMean m = a.means[b];
  if (i >= a.rows || m.kind == GPX_MEAN_ZERO) return;
  double* o = a.out + (long long)b * a.sOut + i;
  *o = *o + mean_eval(m.kind, m.n_coef, a.theta + (long long)b * GPX_THETA_STRIDE + m.off,
                      a.X + (long long)b * a.sX + (long long)i * a.D, a.D);
}

__device__ __forceinline__ double mean_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// g_k = Σ_{j<n} α_j ∂m(x_j)/∂β_k into results[b][1 + off + k]. One workgroup per problem: thread t
// takes j = t, t + 256, ... (fp64 partials in registers), a butterfly within each wave, then the
// four waves' sums through LDS added in wave order. No atomics: the order is the problem's own.
__global__ __launch_bounds__(kMeanBlock) void mean_grad_kernel(MeanArgs a) {
  const int b = a.active[blockIdx.x];
  const DevMean m = a.means[b];
  if (m.kind == GPX_MEAN_ZERO) return;  // (uniform over the workgroup)
  __shared__ double sred[kMeanBlock / 64][kMeanMaxCoef];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.nvalid[b];
  const double* al = a.alpha + (long long)b * a.sVec;
  const double* x = a.X + (long long)b * a.sX;
  double acc[kMeanMaxCoef];
#pragma unroll
  for (int k = 0; k < kMeanMaxCoef; ++k) acc[k] = 0.0;
  for (int j = tid; j < n; j += kMeanBlock) {
    const double aj = al[j];
    const double* xj = x + (long long)j * a.D;
#pragma unroll
    for (int k = 0; k < kMeanMaxCoef; ++k)
      if (k < m.n_coef) acc[k] = fma(aj, mean_dcoef(m.kind, k, xj, a.D), acc[k]);
  }
#pragma unroll
  for (int k = 0; k < kMeanMaxCoef; ++k) {
    const double v = mean_wave_sum(acc[k]);
    if (lane == 0) sred[wave][k] = v;
  }
  __syncthreads();
  if (tid < m.n_coef)
    a.results[(long long)b * kResStride + 1 + m.off + tid] =
        ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}
}  // namespace

void launch_mean_resid(const MeanArgs& a, int n_active, hipStream_t s) {
  const int nblk = (a.rows + kMeanBlock - 1) / kMeanBlock;
  hipLaunchKernelGGL(mean_resid_kernel, dim3(nblk * n_active), dim3(kMeanBlock), 0, s, a, nblk);
}
void launch_mean_add(const MeanArgs& a, int n_active, hipStream_t s) {
  const int nblk = (a.rows + kMeanBlock - 1) / kMeanBlock;
  hipLaunchKernelGGL(mean_add_kernel, dim3(nblk * n_active), dim3(kMeanBlock), 0, s, a, nblk);
}
void launch_mean_grad(const MeanArgs& a, int n_active, hipStream_t s) {
  hipLaunchKernelGGL(mean_grad_kernel, dim3(n_active), dim3(kMeanBlock), 0, s, a);
}

// ---- the batch's mean state (host) ----------------------------------------------------------
int mean_ncoef(const gpx_batch* bt, int b) { return bt->means.empty() ? 0 : bt->means[b].n_coef; }

// the slot goes back to zero mean (every rebind); the device copy follows with the next call
void mean_reset_slot(gpx_batch* bt, int b) {
  if (bt->means.empty() || bt->means[b].kind == GPX_MEAN_ZERO) return;
  bt->means[b] = gpx_mean_spec{GPX_MEAN_ZERO, 0, 0, 0};
  --bt->n_mean;
  bt->mean_dirty = 1;
}

// the slots' specs and coefficient columns to the device, when they changed (on s, before the
// call's first mean kernel)
int flush_means(gpx_batch* bt, hipStream_t s) {
  if (!bt->mean_dirty) return GPX_OK;
  gpx_ctx* ctx = bt->ctx;
  {  // (an asynchronous predict's transfers have left the pinned blocks)
    const int e = wait_io(bt);
    if (e != GPX_OK) return e;
  }
  for (int b = 0; b < bt->B; ++b) {
    const gpx_mean_spec& m = bt->means[b];
    bt->h_mean[b] = DevMean{m.kind, m.degree, m.n_coef, bt->specs[b].n_params + 1};
  }
  HIPX(ctx, hipMemcpyAsync(bt->d_mean, bt->h_mean, sizeof(DevMean) * bt->B, hipMemcpyHostToDevice, s));
  bt->mean_dirty = 0;
  return GPX_OK;
}

static MeanArgs mean_args(const gpx_batch* bt, const int* d_act) {
  MeanArgs a{};
  a.active = d_act; a.means = bt->d_mean; a.theta = bt->d_theta; a.nvalid = bt->d_n;
  a.X = bt->X; a.sX = (long long)bt->Nmax * bt->D; a.D = bt->D;
  return a;
}

int mean_residuals(gpx_batch* bt, const int* d_act, int na, hipStream_t s) {
  const int e = flush_means(bt, s);
  if (e != GPX_OK) return e;
  MeanArgs a = mean_args(bt, d_act);
  a.Y = bt->Y; a.sY = bt->Nmax; a.out = bt->resid; a.sOut = bt->Nmax; a.rows = bt->Nmax;
  launch_mean_resid(a, na, s);
  return GPX_OK;
}

void mean_gradients(gpx_batch* bt, const int* d_act, int na, hipStream_t s) {
  MeanArgs a = mean_args(bt, d_act);
  a.alpha = bt->alpha; a.sVec = bt->Np; a.results = bt->results;
  launch_mean_grad(a, na, s);
}

void mean_add(gpx_batch* bt, const int* d_act, int na, const double* Xnew, int M, double* mean, hipStream_t s) {
  MeanArgs a = mean_args(bt, d_act);
  a.X = Xnew; a.sX = (long long)M * bt->D; a.out = mean; a.sOut = M; a.rows = M;
  launch_mean_add(a, na, s);
}

}  // namespace gpx

using namespace gpx;

extern "C" int gpx_batch_set_mean(gpx_batch* bt, int b, const gpx_mean_spec* mean) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if (b < 0 || b >= bt->B) return fail(ctx, GPX_BAD_ARG, "gpx_batch_set_mean: slot out of range");
  if (bt->pending_eval) return fail(ctx, GPX_BAD_ARG, "an evaluation is submitted on this batch");
  gpx_mean_spec m{GPX_MEAN_ZERO, 0, 0, 0};
  if (mean && mean->kind != GPX_MEAN_ZERO) m = *mean;
  if (m.kind == GPX_MEAN_ZERO) {
    if (!bt->means.empty() && bt->means[b].kind != GPX_MEAN_ZERO) {
      mean_reset_slot(bt, b);
      bt->fac_valid[b] = 0;
    }
    return GPX_OK;
  }
  if (bt->compact)
    return fail(ctx, GPX_BAD_ARG, "mean functions are not supported on band-storage batches (gpx_batch_create_banded)");
  if (bt->defer_q >= 0 || !bt->slow_out.empty())
    return fail(ctx, GPX_BAD_ARG, "mean functions are not supported with deferred completion (gpx_batch_set_deferred)");
  int want = -1;
  switch (m.kind) {
    case GPX_MEAN_CONSTANT: want = 1; break;
    case GPX_MEAN_LINEAR: want = bt->D + 1; break;
    case GPX_MEAN_POLYNOMIAL:
      if (bt->D != 1) return fail(ctx, GPX_BAD_ARG, "the Polynomial mean needs one input column (D = 1)");
      if (m.degree < 0 || m.degree > kMeanMaxDegree)
        return fail(ctx, GPX_BAD_ARG, "the Polynomial mean's degree must be 0..4");
      want = m.degree + 1;
      break;
    default: return fail(ctx, GPX_BAD_ARG, "unknown mean kind");
  }
  if (m.n_coef != want) return fail(ctx, GPX_BAD_ARG, "mean spec: n_coef does not match its kind");
  if (bt->specs[b].n_params + 1 + m.n_coef > GPX_THETA_STRIDE)
    return fail(ctx, GPX_BAD_ARG,
                "the theta row is too short for this kernel's parameters, the noise and the mean's coefficients "
                "(n_params + 1 + n_coef > GPX_THETA_STRIDE)");
  m.reserved = 0;
  if (!bt->resid) {
    // allocated once and never moved: the captured reduction chains are keyed on the pointers
    // they read (gpx_bcr.hip), the targets' among them
    HIPX(ctx, hipSetDevice(ctx->device));
    HIPX(ctx, hipMalloc(&bt->resid, sizeof(double) * (size_t)bt->B * bt->Nmax));
    HIPX(ctx, hipMalloc(&bt->d_mean, sizeof(DevMean) * bt->B));
    HIPX(ctx, hipHostMalloc(&bt->h_mean, sizeof(DevMean) * bt->B, hipHostMallocDefault));
    bt->means.assign(bt->B, gpx_mean_spec{GPX_MEAN_ZERO, 0, 0, 0});
  }
  if (bt->means[b].kind == GPX_MEAN_ZERO) ++bt->n_mean;
  bt->means[b] = m;
  bt->mean_dirty = 1;
  bt->fac_valid[b] = 0;
  return GPX_OK;
}
