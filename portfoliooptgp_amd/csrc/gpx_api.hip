// gpx_api.hip — C ABI (include/gpx.h) of the exact-GP engine: context and batch lifetime, rebinds
// and slot staging, the setters, timing and the wave trace. The rest of the host side:
//   gpx_dense.hip    the dense recursion below            gpx_route.hip  band tables and routing
//   gpx_eval.hip     submit .. complete, lanes, deferral  gpx_predict.hip  predictions
//   gpx_knobs.hip    every environment variable the library reads
//
// One evaluation of logML and ∂logML/∂θ for B problems (the closure gpflow.optimizers.Scipy
// calls from GPR/model_trainer.py:19) runs, all on one stream:
//   1. K = k(X,X) + σn²I                                      build_kernel
//   2. (L, W = L⁻¹) by recursive blocked Cholesky-and-inverse  leaf + MFMA TRMM/SYRK GEMMs
//        chol_inv(A):  (L11,W11) = chol_inv(A11);  L21 = A21 W11ᵀ;  A22 -= L21 L21ᵀ;
//                      (L22,W22) = chol_inv(A22);  W21 = −W22 (L21 W11)
//   3. z = W y, α = Wᵀ z                                      trmv kernels
//   4. K⁻¹ = WᵀW formed tile by tile and contracted on the fly with (ααᵀ − K⁻¹)∘∂K/∂θ
//   5. logML = −½‖z‖² − Σ log L_ii − (n/2) log 2π;  ∂logML/∂θ = ½ Σ (ααᵀ − K⁻¹)∘∂K/∂θ
// Algorithmic flops per problem: N³/3 (potrf) + N³/3 (trtri) + N³/3 (WᵀW) ≈ N³.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <chrono>
#include <vector>
#include "gpx_host.h"

using namespace gpx;

namespace gpx {

const char* kVersion = "gpx 0.1.0 (gfx950, fp64 MFMA)";

std::string& last_error_slot() {
  static thread_local std::string msg;
  return msg;
}

// Band width <= 2 blocks: the whole sweep per problem in two fused kernels (gpx_band.hip),
// each problem with its own p (d_bandp); K's band is built for the widest.
double band_fused_flops(int Np, int p, bool fwd) {
  const double U = 2.0 * kLeaf * kLeaf * kLeaf;  // one 64³ block product
  const int nb = Np / kLeaf;
  double f = 0.0;
  for (int k = 0; k < nb; ++k) {
    const double q = std::min(p, nb - 1 - k);
    f += fwd ? (2.0 / 3.0 + q + q * (q + 1) / 2.0) * U   // leaf, panels, window update
             : (1.0 + q + q * q + q) * U;               // WᵀW, G, Z panel, Gᵀ Z
  }
  return f;
}

// MFMA flops the band16 sweeps issue per problem (2·16³ per 16x16x16 tile product; the leaves'
// 16x16 factorisations are VALU work and not counted)
double band16_flops(int Np, int Q, bool fwd) {
  const double U = 2.0 * 16 * 16 * 16;
  const int nb = Np / 16;
  double f = 0.0;
  for (int k = 0; k < nb; ++k) {
    const double q = std::min(Q, nb - 1 - k);
    f += fwd ? (q + q * (q + 1) / 2.0) * U          // panels, window update
             : (q + q * q + 1.0 + q) * U;           // G, Z panel, WᵀW, GᵀZ
  }
  return f;
}

// pinned n[] / specs[] mirrors and the dirty flags of the deferred rebinds (first rebind)
int ensure_rebind_meta(gpx_batch* bt) {
  gpx_ctx* ctx = bt->ctx;
  if (!bt->h_nmeta) {
    HIPX(ctx, hipHostMalloc(&bt->h_nmeta, sizeof(int) * bt->B, hipHostMallocNonCoherent));
    HIPX(ctx, hipHostMalloc(&bt->h_specs, sizeof(DevSpec) * bt->B, hipHostMallocNonCoherent));
  }
  if (bt->dirty.empty()) {
    bt->dirty.assign(bt->B, 0);
    bt->n_dirty = 0;
  }
  return GPX_OK;
}

// remember slot b's per-block X boxes (rows of its valid blocks; the rest of the slot's row
// is left as it was)
void keep_slot_box(gpx_batch* bt, int b, const double* box) {
  const int nbx = (bt->Nmax + kBox - 1) / kBox;
  const size_t row = (size_t)nbx * bt->D * 2;
  if (bt->slot_box.empty()) {
    bt->slot_box.assign(row * bt->B, 0.0);
    bt->slot_box_ok.assign(bt->B, 0);
  }
  const int nvb = (bt->n[b] + kBox - 1) / kBox;
  std::memcpy(bt->slot_box.data() + row * b, box, sizeof(double) * (size_t)nvb * bt->D * 2);
  bt->slot_box_ok[b] = 1;
}

// the GPX_SUBMIT_STATS accumulators (SubClock, gpx_host.h)
void print_submit_stats(const gpx_batch* bt) {
  fprintf(stderr, "[gpx submit stats] batch B=%d calls=%lld flush=%.3f route=%.3f upload=%.3f launch=%.3f "
          "download=%.3f complete_sync=%.3f (flush: wait_io=%.3f box_sync=%.3f over %lld syncs) "
          "predict=%.3f (io wait %.3f, shadow slots %.3f, %.0f shadow predicts) s\n", bt->B,
          bt->sub_calls, bt->sub_s[0], bt->sub_s[1], bt->sub_s[2], bt->sub_s[3], bt->sub_s[4], bt->sub_s[5],
          bt->sub_s[6], bt->sub_s[7], bt->box_syncs, bt->sub_s[8], bt->sub_s[9], bt->sub_s[10],
          bt->timing.shadow_predicts);
}

}  // namespace gpx


extern "C" {

const char* gpx_version(void) { return kVersion; }

int gpx_create(int device, gpx_ctx** out) {
  if (!out) return GPX_BAD_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GPX_HIP_ERROR;
  if (device < 0 || device >= ndev) return GPX_BAD_ARG;
  if (hipSetDevice(device) != hipSuccess) return GPX_HIP_ERROR;
  gpx_ctx* c = new gpx_ctx();
  c->device = device;
  const bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
  if (!ok) {
    delete c;
    return GPX_HIP_ERROR;
  }
  *out = c;
  return GPX_OK;
}

int gpx_destroy(gpx_ctx* ctx) {
  if (!ctx) return GPX_BAD_ARG;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->sample.ws) (void)hipFree(ctx->sample.ws);
  if (ctx->sample.idx) (void)hipFree(ctx->sample.idx);
  delete ctx;
  return GPX_OK;
}

const char* gpx_last_error(const gpx_ctx* ctx) {
  (void)ctx;
  return last_error_slot().c_str();
}

int gpx_set_profiling(gpx_ctx* ctx, int enabled) {
  if (!ctx) return GPX_BAD_ARG;
  ctx->profiling = enabled;
  return GPX_OK;
}

static int batch_create(gpx_ctx* ctx, int B, int N_max, int D, const double* X, const double* Y,
                        const int32_t* n, const gpx_kernel_spec* specs, bool compact, gpx_batch** out) {
  if (!ctx || !out) return GPX_BAD_ARG;
  *out = nullptr;
  if (B <= 0 || N_max <= 0 || D <= 0 || D > GPX_MAX_DIM || !X || !Y || !n || !specs)
    return fail(ctx, GPX_BAD_ARG, "bad batch dimensions or null pointer");
  for (int b = 0; b < B; ++b) {
    if (n[b] < 1 || n[b] > N_max) return fail(ctx, GPX_BAD_ARG, "n[b] must be in [1, N_max]");
    if (const char* why = spec_error(specs[b], D)) return fail(ctx, GPX_BAD_ARG, why);
  }
  if (((long long)N_max + kLeaf - 1) / kLeaf * kLeaf > kGemmMaxLd)
    return fail(ctx, GPX_BAD_ARG, "N_max exceeds the GEMM buffer-load window (kGemmMaxLd)");
  if (compact && (N_max < 8 * kLeaf - (kLeaf - 1) || N_max > 8192))
    return fail(ctx, GPX_BAD_ARG, "band storage needs 449 <= N_max <= 8192 (8 to 128 64-blocks)");
  HIPX(ctx, hipSetDevice(ctx->device));
  gpx_batch* bt = new gpx_batch();
  bt->ctx = ctx; bt->B = B; bt->Nmax = N_max; bt->D = D;
  bt->Np = ((N_max + kLeaf - 1) / kLeaf) * kLeaf;
  bt->X = X; bt->Y = Y;
  bt->n.assign(n, n + B);
  bt->specs.assign(specs, specs + B);
  // band storage: rows of ldm + 1 doubles holding columns i − 64·(kBandStoreP+1) .. i + 63
  // (band_c0 = the column offset of the diagonal in a row), plus a 64-double guard
  const long long band_c0 = 64LL * kBandStoreP + 64;
  if (compact) {
    bt->compact = 1;
    bt->ldm = 64 * (kBandStoreP + 2);
    bt->smat = (long long)bt->Np * (bt->ldm + 1);
  }
  const size_t mat = ((size_t)B * mat_stride(bt) + (compact ? 64 : 0)) * sizeof(double);
  const size_t vec = (size_t)B * bt->Np * sizeof(double);
  const int t64 = bt->Np / 64;
  // the dense contraction writes one row of partials per lower 64-tile; the fused band
  // sweeps (band storage's only path) one row per problem
  bt->partial_stride = compact ? GPX_THETA_STRIDE : (long long)t64 * (t64 + 1) / 2 * GPX_THETA_STRIDE;
  auto cleanup = [&](const std::string& m) {
    gpx_batch_destroy(bt);
    return fail(ctx, GPX_HIP_ERROR, m);
  };
  if (hipMalloc(&bt->K, mat) != hipSuccess || hipMalloc(&bt->L, mat) != hipSuccess ||
      hipMalloc(&bt->W, mat) != hipSuccess)
    return cleanup("out of device memory for K/L/W workspace");
  if (hipMalloc(&bt->z, vec) != hipSuccess || hipMalloc(&bt->alpha, vec) != hipSuccess ||
      hipMalloc(&bt->ldiag, vec) != hipSuccess ||
      hipMalloc(&bt->partial, (size_t)B * bt->partial_stride * sizeof(double)) != hipSuccess ||
      hipMalloc(&bt->d_n, sizeof(int) * B) != hipSuccess ||
      hipMalloc(&bt->d_orow, sizeof(int) * B) != hipSuccess ||
      hipMalloc(&bt->d_specs, sizeof(DevSpec) * B) != hipSuccess)
    return cleanup("out of device memory for batch vectors");
  {
    const size_t ints = ((size_t)B * sizeof(int) + 7) / 8 * 8;
    bt->io_info_off = ints;
    bt->io_bandp_off = 2 * ints;
    bt->io_theta_off = 3 * ints;
    bt->io_res_off = bt->io_theta_off + (size_t)B * GPX_THETA_STRIDE * sizeof(double);
    bt->io_flag_off = bt->io_res_off + (size_t)B * kResStride * sizeof(double);
    bt->io_bytes = bt->io_flag_off + ints;
    if (hipMalloc(&bt->d_io, bt->io_bytes) != hipSuccess ||
        hipHostMalloc(&bt->h_io, bt->io_bytes, hipHostMallocNonCoherent) != hipSuccess)
      return cleanup("out of memory for the batch I/O block");
    std::memset(bt->h_io, 0, bt->io_bytes);
    bt->d_active = reinterpret_cast<int*>(bt->d_io);
    bt->d_info = reinterpret_cast<int*>(bt->d_io + bt->io_info_off);
    bt->d_bandp = reinterpret_cast<int*>(bt->d_io + bt->io_bandp_off);
    bt->h_bandp = reinterpret_cast<int*>(bt->h_io + bt->io_bandp_off);
    bt->d_theta = reinterpret_cast<double*>(bt->d_io + bt->io_theta_off);
    bt->results = reinterpret_cast<double*>(bt->d_io + bt->io_res_off);
    bt->h_info = reinterpret_cast<int*>(bt->h_io + bt->io_info_off);
    bt->h_results = reinterpret_cast<double*>(bt->h_io + bt->io_res_off);
  }
  // W and L upper triangles must read as exact zeros (never written afterwards)
  if (hipMemset(bt->W, 0, mat) != hipSuccess || hipMemset(bt->L, 0, mat) != hipSuccess ||
      hipMemset(bt->K, 0, mat) != hipSuccess)
    return cleanup("memset failed");
  if (compact) {
    bt->Kraw = bt->K; bt->Lraw = bt->L; bt->Wraw = bt->W;
    bt->K += band_c0; bt->L += band_c0; bt->W += band_c0;
  }
  for (int g = 0; g < kAux; ++g)
    if (hipStreamCreateWithFlags(&bt->aux[g], hipStreamNonBlocking) != hipSuccess)
      return cleanup("stream creation failed");
  for (int e = 0; e < kEvents; ++e)
    if (hipEventCreateWithFlags(&bt->ev[e], hipEventDisableTiming) != hipSuccess)
      return cleanup("event creation failed");
  std::vector<DevSpec> ds(B);
  for (int b = 0; b < B; ++b) std::memcpy(&ds[b], &specs[b], sizeof(DevSpec));
  static_assert(sizeof(DevSpec) == sizeof(gpx_kernel_spec), "spec layout");
  if (hipMemcpy(bt->d_specs, ds.data(), sizeof(DevSpec) * B, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(bt->d_n, n, sizeof(int) * B, hipMemcpyHostToDevice) != hipSuccess)
    return cleanup("upload failed");
  bt->fac_theta.assign((size_t)B * GPX_THETA_STRIDE, 0.0);
  bt->fac_valid.assign(B, 0);
  bt->fac_band.assign(B, 0);
  bt->band_rmin.assign((size_t)B * GPX_MAX_TERMS * (bt->Np / kLeaf), INFINITY);
  bt->band_tail.assign((size_t)B * GPX_MAX_TERMS, bt->Np / kLeaf);
  if (bt->Np <= kBand16MaxNp) {
    bt->band_rmin16.assign((size_t)B * GPX_MAX_TERMS * (bt->Np / kBox), INFINITY);
    bt->band_tail16.assign((size_t)B * GPX_MAX_TERMS, bt->Np / kBox);
  }
  if (band_shape(bt)) {
    std::vector<double> hx((size_t)B * N_max * D);
    if (hipMemcpy(hx.data(), X, sizeof(double) * hx.size(), hipMemcpyDeviceToHost) != hipSuccess)
      return cleanup("upload failed");
    for (int b = 0; b < B; ++b) band_tables(bt, b, hx.data() + (size_t)b * N_max * D);
  }
  if (compact) {
    // the dense fallback: kShadowSlots ordinary slots with their own X / Y rows
    const size_t nx = (size_t)kShadowSlots * N_max * D, ny = (size_t)kShadowSlots * N_max;
    if (hipMalloc(&bt->shX, nx * sizeof(double)) != hipSuccess ||
        hipMalloc(&bt->shY, ny * sizeof(double)) != hipSuccess ||
        hipMemset(bt->shX, 0, nx * sizeof(double)) != hipSuccess ||
        hipMemset(bt->shY, 0, ny * sizeof(double)) != hipSuccess)
      return cleanup("out of device memory for the dense fallback slots");
    std::vector<int32_t> n1(kShadowSlots, 1);
    std::vector<gpx_kernel_spec> sp1(kShadowSlots, specs[0]);
    const int rc = batch_create(ctx, kShadowSlots, N_max, D, bt->shX, bt->shY, n1.data(), sp1.data(), false,
                                &bt->shadow);
    if (rc != GPX_OK) {
      const std::string m = last_error_slot();
      gpx_batch_destroy(bt);
      return fail(ctx, rc, "dense fallback slots: " + m);
    }
    bt->shadow->force_dense = 1;
  }
  *out = bt;
  return GPX_OK;
}

int gpx_batch_create(gpx_ctx* ctx, int B, int N_max, int D, const double* X, const double* Y,
                     const int32_t* n, const gpx_kernel_spec* specs, gpx_batch** out) {
  return batch_create(ctx, B, N_max, D, X, Y, n, specs, false, out);
}

int gpx_batch_create_banded(gpx_ctx* ctx, int B, int N_max, int D, const double* X, const double* Y,
                            const int32_t* n, const gpx_kernel_spec* specs, gpx_batch** out) {
  return batch_create(ctx, B, N_max, D, X, Y, n, specs, true, out);
}

int gpx_batch_destroy(gpx_batch* bt) {
  if (!bt) return GPX_BAD_ARG;
  (void)hipSetDevice(bt->ctx->device);
  if (bt->pending_eval) {  // a submitted evaluation still reads and writes the buffers below
    (void)hipStreamSynchronize(bt->pending_eval->s);
    bt->pending_eval.reset();
  }
  if (submit_stats_on() && bt->sub_calls > 0) print_submit_stats(bt);
  if (!bt->slow_out.empty() || bt->slow_s || bt->d_slow_res) {  // deferred slow parts use the buffers below
    for (auto& r : bt->slow_out) (void)hipEventSynchronize(r->done);
    if (bt->slow_s) (void)hipStreamSynchronize(bt->slow_s);
    bt->slow_out.clear();
    bt->slow_pool.clear();
    if (bt->slow_s) (void)hipStreamDestroy(bt->slow_s);
    for (hipEvent_t e : {bt->slow_in, bt->slow_up, bt->bulk_ev})
      if (e) (void)hipEventDestroy(e);
    for (void* q : {(void*)bt->d_slow_act, (void*)bt->d_slow_theta, (void*)bt->d_slow_bandp, (void*)bt->d_slow_info,
                    (void*)bt->d_slow_res, (void*)bt->d_slow_info_c})
      if (q) (void)hipFree(q);
  }
  if (bt->shadow) gpx_batch_destroy(bt->shadow);  // waits for its own submitted evaluation
  if (bt->shadow_s) (void)hipStreamDestroy(bt->shadow_s);
  if (bt->shadow_ev) (void)hipEventDestroy(bt->shadow_ev);
  for (auto& w : bt->rebind_waits) (void)hipEventDestroy(w.ev);
  if (bt->io_ev) {
    (void)hipEventSynchronize(bt->io_ev);
    (void)hipEventDestroy(bt->io_ev);
  }
  if (bt->compact && bt->Kraw) {  // K/L/W point into the raw allocations (band storage's row offset)
    bt->K = bt->Kraw; bt->L = bt->Lraw; bt->W = bt->Wraw;
  }
  for (void* p : {(void*)bt->shX, (void*)bt->shY, (void*)bt->d_wtrace, (void*)bt->d_wtrace_n})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)bt->K, (void*)bt->L, (void*)bt->W, (void*)bt->z, (void*)bt->alpha,
                  (void*)bt->ldiag, (void*)bt->partial, (void*)bt->d_io, (void*)bt->d_n, (void*)bt->d_orow,
                  (void*)bt->d_specs, (void*)bt->kxs, (void*)bt->pvp, (void*)bt->abuf, (void*)bt->covw,
                  (void*)bt->samp, (void*)bt->d_sinfo, (void*)bt->bres, (void*)bt->bcr_ws, (void*)bt->bcr_ws_slow})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : bt->bcr_ev)
    if (e) (void)hipEventDestroy(e);
  bcr_graph_cache_free(bt->bcr_graphs);  // (every stream of the batch has drained above)
  bt->bcr_graphs = nullptr;
  if (bt->h_io) (void)hipHostFree(bt->h_io);
  if (bt->h_sio) (void)hipHostFree(bt->h_sio);
  if (bt->h_io_pred) (void)hipHostFree(bt->h_io_pred);
  if (bt->h_stage) (void)hipHostFree(bt->h_stage);
  if (bt->h_rdesc) (void)hipHostFree(bt->h_rdesc);
  if (bt->h_box) (void)hipHostFree(bt->h_box);
  if (bt->d_box) (void)hipFree(bt->d_box);
  if (bt->h_nmeta) (void)hipHostFree(bt->h_nmeta);
  if (bt->h_specs) (void)hipHostFree(bt->h_specs);
  if (bt->resid) (void)hipFree(bt->resid);
  if (bt->d_mean) (void)hipFree(bt->d_mean);
  if (bt->h_mean) (void)hipHostFree(bt->h_mean);
  for (int g = 0; g < kAux; ++g)
    if (bt->aux[g]) (void)hipStreamDestroy(bt->aux[g]);
  if (bt->hp) (void)hipStreamDestroy(bt->hp);
  for (int g = 0; g < kGroups; ++g) {
    if (bt->workers[g]) (void)hipStreamDestroy(bt->workers[g]);
    if (bt->join[g]) (void)hipEventDestroy(bt->join[g]);
  }
  if (bt->fork) (void)hipEventDestroy(bt->fork);
  for (int e = 0; e < kEvents; ++e)
    if (bt->ev[e]) (void)hipEventDestroy(bt->ev[e]);
  delete bt;
  return GPX_OK;
}

static int check_rebind(gpx_batch* bt, int b, int n, const gpx_kernel_spec* spec) {
  gpx_ctx* ctx = bt->ctx;
  if (b < 0 || b >= bt->B || n < 1 || n > bt->Nmax || !spec)
    return fail(ctx, GPX_BAD_ARG, "bad rebind arguments");
  if (const char* why = spec_error(*spec, bt->D)) return fail(ctx, GPX_BAD_ARG, why);
  if (!bt->deferred.empty() && b >= 0 && b < bt->B && bt->deferred[b])
    return fail(ctx, GPX_BAD_ARG, "slot has a deferred evaluation in flight (gpx_batch_deferred_wait)");
  return GPX_OK;
}

int gpx_batch_rebind(gpx_batch* bt, int b, int n, const gpx_kernel_spec* spec) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  int rc = check_rebind(bt, b, n, spec);
  if (rc != GPX_OK) return rc;
  const gpx_kernel_spec& sp = *spec;
  HIPX(ctx, hipSetDevice(ctx->device));
  bt->n[b] = n;
  bt->specs[b] = sp;
  bt->fac_valid[b] = 0;
  mean_reset_slot(bt, b);  // (every rebind leaves the slot zero-mean: gpx_batch_set_mean)
  bt->fac_band[b] = 0;
  if (!bt->dirty.empty() && bt->dirty[b]) {  // the caller's own device data supersedes a staged one
    bt->dirty[b] = 0;
    --bt->n_dirty;
  }
  for (size_t i = 0; i < bt->pend.size(); ++i)
    if (bt->pend[i].b == b) {
      bt->pend.erase(bt->pend.begin() + i);
      break;
    }
  HIPX(ctx, hipMemcpy(bt->d_n + b, &n, sizeof(int), hipMemcpyHostToDevice));
  HIPX(ctx, hipMemcpy(bt->d_specs + b, &sp, sizeof(DevSpec), hipMemcpyHostToDevice));
  if (band_shape(bt)) {
    std::vector<double> hx((size_t)n * bt->D);
    HIPX(ctx, hipMemcpy(hx.data(), bt->X + (size_t)b * bt->Nmax * bt->D, sizeof(double) * hx.size(),
                        hipMemcpyDeviceToHost));
    band_tables(bt, b, hx.data());
  }
  return GPX_OK;
}

static int stage_slot(gpx_batch* bt, int b, double** hx, double** hy) {
  gpx_ctx* ctx = bt->ctx;
  const size_t nx = (size_t)bt->Nmax * bt->D, ny = bt->Nmax;
  constexpr size_t kSpecDoubles = (sizeof(DevSpec) + sizeof(double) - 1) / sizeof(double);
  if (!bt->h_stage) {
    bt->stage_stride = nx + ny + 1 + kSpecDoubles;
    HIPX(ctx, hipHostMalloc(&bt->h_stage, sizeof(double) * bt->stage_stride * bt->B, hipHostMallocNonCoherent));
  }
  const int rc = ensure_rebind_meta(bt);
  if (rc != GPX_OK) return rc;
  *hx = bt->h_stage + (size_t)b * bt->stage_stride;
  *hy = *hx + nx;
  return GPX_OK;
}

int gpx_batch_rebind_device(gpx_batch* bt, int b, int n, const double* X, const double* Y,
                            const gpx_kernel_spec* spec, void* stream) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if (!X || !Y) return fail(ctx, GPX_BAD_ARG, "null device inputs");
  int rc = check_rebind(bt, b, n, spec);
  if (rc != GPX_OK) return rc;
  // recorded only: the next device call's flush_rebinds gathers every pending slot in one
  // kernel on that call's stream (X and Y must stay valid until then). X and Y are ready in
  // the order of `stream` (the caller's current stream, where their producers ran): an event
  // recorded on it now orders the gather after them, whichever stream the gather runs on
  if (stream) {
    HIPX(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)stream;
    gpx_batch::RebindWait* w = nullptr;
    for (auto& x : bt->rebind_waits)
      if (x.s == s) w = &x;
    if (!w) {
      hipEvent_t ev;
      HIPX(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      bt->rebind_waits.push_back(gpx_batch::RebindWait{s, ev, false});
      w = &bt->rebind_waits.back();
    }
    HIPX(ctx, hipEventRecord(w->ev, s));
    w->armed = true;
  }
  bt->n[b] = n;
  bt->specs[b] = *spec;
  bt->fac_valid[b] = 0;
  mean_reset_slot(bt, b);
  bt->fac_band[b] = 0;
  if (!bt->dirty.empty() && bt->dirty[b]) {  // supersedes a host-staged rebind of the slot
    bt->dirty[b] = 0;
    --bt->n_dirty;
  }
  if (!bt->slot_box_ok.empty()) bt->slot_box_ok[b] = 0;
  for (auto& e : bt->pend)
    if (e.b == b) {
      e = gpx_batch::PendingRebind{b, n, X, Y, false};
      return GPX_OK;
    }
  bt->pend.push_back(gpx_batch::PendingRebind{b, n, X, Y, false});
  return GPX_OK;
}

int gpx_batch_rebind_device_boxed(gpx_batch* bt, int b, int n, const double* X, const double* Y,
                                  const gpx_kernel_spec* spec, const double* box, void* stream) {
  if (!bt) return GPX_BAD_ARG;
  if (!box) return fail(bt->ctx, GPX_BAD_ARG, "null boxes");
  const int rc = gpx_batch_rebind_device(bt, b, n, X, Y, spec, stream);
  if (rc != GPX_OK) return rc;
  for (auto& e : bt->pend)
    if (e.b == b) e.boxed = true;
  if (band_shape(bt)) {  // the band tables now, from the caller's boxes: no download at the gather
    band_tables_boxes(bt, b, box);
    keep_slot_box(bt, b, box);
  }
  return GPX_OK;
}

int gpx_batch_slot_boxes(const gpx_batch* bt, int b, double* out) {
  if (!bt || !out || b < 0 || b >= bt->B) return GPX_BAD_ARG;
  if (bt->slot_box_ok.empty() || !bt->slot_box_ok[b] || !bt->pend.empty()) return GPX_BAD_ARG;
  const int nbx = (bt->Nmax + kBox - 1) / kBox;
  const size_t row = (size_t)nbx * bt->D * 2;
  const int nvb = (bt->n[b] + kBox - 1) / kBox;
  std::memcpy(out, bt->slot_box.data() + row * b, sizeof(double) * (size_t)nvb * bt->D * 2);
  return GPX_OK;
}

int gpx_batch_rebind_host(gpx_batch* bt, int b, int n, const double* X, const double* Y,
                          const gpx_kernel_spec* spec, void* stream) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if (!X || !Y) return fail(ctx, GPX_BAD_ARG, "null host inputs");
  int rc = check_rebind(bt, b, n, spec);
  if (rc != GPX_OK) return rc;
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const size_t nx = (size_t)bt->Nmax * bt->D, ny = bt->Nmax;
  double *hx, *hy;
  rc = stage_slot(bt, b, &hx, &hy);
  if (rc != GPX_OK) return rc;
  for (size_t i = 0; i < bt->pend.size(); ++i)
    if (bt->pend[i].b == b) {
      bt->pend.erase(bt->pend.begin() + i);
      break;
    }
  if (hx != X) std::memcpy(hx, X, sizeof(double) * (size_t)n * bt->D);
  std::memset(hx + (size_t)n * bt->D, 0, sizeof(double) * (nx - (size_t)n * bt->D));
  if (hy != Y) std::memcpy(hy, Y, sizeof(double) * n);
  std::memset(hy + n, 0, sizeof(double) * (ny - n));
  // the copies go out with the next device call (flush_rebinds)
  bt->n[b] = n;
  bt->specs[b] = *spec;
  bt->fac_valid[b] = 0;
  mean_reset_slot(bt, b);
  bt->fac_band[b] = 0;
  if (!bt->dirty[b]) {
    bt->dirty[b] = 1;
    ++bt->n_dirty;
  }
  (void)s;
  if (!bt->slot_box_ok.empty()) bt->slot_box_ok[b] = 0;
  if (band_shape(bt)) band_tables(bt, b, hx);
  return GPX_OK;
}

int gpx_batch_reset_timing(gpx_batch* bt) {
  if (!bt) return GPX_BAD_ARG;
  bt->timing = gpx_timing{};
  for (double& v : bt->sub_s) v = 0.0;
  bt->sub_calls = bt->box_syncs = 0;
  return GPX_OK;
}

int gpx_batch_last_timing(const gpx_batch* bt, gpx_timing* out) {
  if (!bt || !out) return GPX_BAD_ARG;
  *out = bt->timing;
  return GPX_OK;
}

int gpx_batch_set_deferred(gpx_batch* bt, int q) {
  if (!bt) return GPX_BAD_ARG;
  if (q < 0 && !bt->slow_out.empty())
    return fail(bt->ctx, GPX_BAD_ARG, "deferred evaluations in flight (gpx_batch_deferred_wait first)");
  if (q >= 0 && bt->n_mean > 0)
    return fail(bt->ctx, GPX_BAD_ARG, "deferred completion is not supported on a batch with a mean function");
  bt->defer_q = q < 0 ? -1 : q;
  if (bt->deferred.size() != (size_t)bt->B) bt->deferred.assign(bt->B, 0);
  return GPX_OK;
}

int gpx_batch_set_band_route(gpx_batch* bt, int route) {
  if (!bt) return GPX_BAD_ARG;
  if (route != GPX_BAND_ROUTE_SWEEPS && route != GPX_BAND_ROUTE_BCR && route != GPX_BAND_ROUTE_AUTO)
    return fail(bt->ctx, GPX_BAD_ARG, "unknown band route");
  if (bt->pending_eval) return fail(bt->ctx, GPX_BAD_ARG, "an evaluation is submitted on this batch");
  bt->band_route = route;
  return GPX_OK;
}

// Diagnostic: the band16 sweeps' per-wavefront residency records (BandFusedArgs::wtrace)
int gpx_batch_wave_trace(gpx_batch* bt, unsigned int cap) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  HIPX(ctx, hipSetDevice(ctx->device));
  HIPX(ctx, hipDeviceSynchronize());  // no sweep is writing the old buffer
  if (bt->d_wtrace) (void)hipFree(bt->d_wtrace);
  if (bt->d_wtrace_n) (void)hipFree(bt->d_wtrace_n);
  bt->d_wtrace = nullptr;
  bt->d_wtrace_n = nullptr;
  bt->wtrace_cap = 0;
  if (cap == 0) return GPX_OK;
  HIPX(ctx, hipMalloc(&bt->d_wtrace, sizeof(unsigned long long) * 3 * (size_t)cap));
  HIPX(ctx, hipMalloc(&bt->d_wtrace_n, sizeof(unsigned int)));
  HIPX(ctx, hipMemset(bt->d_wtrace_n, 0, sizeof(unsigned int)));
  bt->wtrace_cap = cap;
  return GPX_OK;
}

int gpx_batch_wave_trace_read(gpx_batch* bt, unsigned long long* out, unsigned int cap, unsigned int* n_out) {
  if (!bt || !n_out || (cap > 0 && !out)) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  *n_out = 0;
  if (!bt->d_wtrace) return GPX_OK;
  HIPX(ctx, hipSetDevice(ctx->device));
  HIPX(ctx, hipDeviceSynchronize());
  unsigned int n = 0;
  HIPX(ctx, hipMemcpy(&n, bt->d_wtrace_n, sizeof(n), hipMemcpyDeviceToHost));
  n = std::min(n, std::min(cap, bt->wtrace_cap));
  if (n > 0) HIPX(ctx, hipMemcpy(out, bt->d_wtrace, sizeof(unsigned long long) * 3 * (size_t)n, hipMemcpyDeviceToHost));
  HIPX(ctx, hipMemset(bt->d_wtrace_n, 0, sizeof(unsigned int)));
  *n_out = n;
  return GPX_OK;
}

}  // extern "C"
