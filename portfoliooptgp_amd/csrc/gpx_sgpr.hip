// gpx_sgpr.hip — C ABI and host orchestration of the SGPR collapsed bound / gradient / predict
// path (gpflow.models.SGPR 2.9.1; the reference's cell at test_scripts/SVGP.py:395: SE kernel,
// 10 inducing points, Scipy().minimize(model.training_loss, ...), predict_y). Gaussian likelihood
// with variance s = σ², zero mean, one output.
//
// With Kmm = k(Z,Z) + 1e-6 I, L = chol(Kmm), W = L⁻¹, Kmn = k(Z,X):
//   G = Kmn Kmnᵀ,  w = Kmn y,  Ĝ = W G Wᵀ,  â = W w
//   B = I + Ĝ/s,   LB = chol(B),  WB = LB⁻¹,  B⁻¹ = WBᵀ WB,  γ = B⁻¹ â = WBᵀ (WB â)
//   F = −N/2 log 2π − N/2 log s − Σ log LB_ii − yᵀy/(2s) + âᵀγ/(2s²) − Σ k_nn/(2s) + tr(Ĝ)/(2s)
//   H = (I − B⁻¹)/s − γγᵀ/s³,              K̄mn = (Wᵀ H W) Kmn + (Wᵀγ/s²) yᵀ
//   K̄mm = Wᵀ [½(I − B⁻¹) − γγᵀ/(2s²) − Ĝ/(2s)] W,   k̄_nn = −1/(2s)
//   ∂F/∂s = −N/(2s) + yᵀy/(2s²) − âᵀγ/s³ + Σk_nn/(2s²) − tr(Ĝ)/(2s²) + tr(B⁻¹Ĝ)/(2s²) + γᵀĜγ/(2s⁴)
//   ∂F/∂θ = Σ K̄mn ∘ ∂Kmn + Σ K̄mm ∘ ∂Kmm + k̄_nn Σ ∂k_nn;   ∂F/∂Z likewise (K̄mm symmetric: factor 2)
// (GPflow's own form is A = L⁻¹Kmn/σ, AAT = AAᵀ, c = LB⁻¹Ay/σ; tests/sgpr_numpy.py restates both
// and pins the gradients by finite differences.) Prediction at X*, A* = W k(Z,X*):
//   mean = k(Z,X*)ᵀ Wᵀγ/s,   var = k** − Σ_m A*² + Σ_m (WB A*)²  (+ s for predict_y)
//
// The data-size work is the SVGP path's: the Kmn build, the split-K MFMA SYRK for G, the GEMM
// Y = (WᵀHW) Kmn and the rows contraction, plus two O(MN)/O(N) streams (w, the k_nn pass). B is
// factored by the same recursive Cholesky-and-inverse as Kmm, in a second B = 1 batch.
//
// Out of scope: mean functions, multi-output Y, full_cov, upper_bound, other likelihoods (those are
// gpx_vgp.hip's), and row-sharding over GPUs (K̄mn depends on the all-reduced B, so shards would need two passes —
// one for G and w, one for the contraction — which the gpx_svgp_partials protocol does not give).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "gpx_host.h"

using namespace gpx;

namespace {
constexpr double kJitter = 1e-6;  // gpflow.config.default_jitter()
constexpr int kTraces = 4;        // tr(Ĝ), Σ B⁻¹∘Ĝ, γᵀĜγ, âᵀγ
}  // namespace

struct gpx_sgpr {
  gpx_ctx* ctx = nullptr;
  int N = 0, M = 0, D = 0, Mp = 0, Ncols = 0, nc = 1, chunkK = 64, rows_chunk = 64;
  const double* X = nullptr;
  const double* Y = nullptr;
  gpx_kernel_spec spec{};
  gpx_batch* kmm = nullptr;  // Kmm factorisation (B = 1, X = Z)
  gpx_batch* bb = nullptr;   // B = I + Ĝ/s factorisation (its K buffer is written directly)
  double *dZ = nullptr, *dYdummy = nullptr, *d_theta = nullptr;
  double *G = nullptr, *T = nullptr, *Gh = nullptr, *Binv = nullptr, *H = nullptr, *Mid = nullptr;
  double *P = nullptr, *Sb = nullptr, *V = nullptr;                        // [Mp][Mp]
  double *w = nullptr, *ahat = nullptr, *t1 = nullptr, *gam = nullptr, *gs = nullptr, *u = nullptr;  // [Mp]
  double *Kmn = nullptr, *Ybuf = nullptr, *Gpart = nullptr;
  double *pdiag = nullptr, *pdot = nullptr, *ptr = nullptr, *fin = nullptr;
  double *pth = nullptr, *pz = nullptr;
  size_t pth_cap = 0, pz_cap = 0;
  int* d_iota = nullptr;
  // fin layout (one download): θ of K̄mn | θ of K̄mm | the N-row pass [kResidW] | traces | Σ log LB_ii
  // | ∂Z of K̄mn [Mp*D] | ∂Z of K̄mm [Mp*D]
  long long off_thn = 0, off_thm = 0, off_diag = 0, off_tr = 0, off_ld = 0, off_zn = 0, off_zm = 0, fin_len = 0;
  // predict workspace
  double *Kms = nullptr, *pA = nullptr, *pB = nullptr;
  size_t kms_cap = 0, pa_cap = 0, pb_cap = 0;
  std::vector<double> h_theta, h_fin;
  int h_info[2] = {0, 0};
};

namespace {

int rows_alloc(gpx_sgpr* sg, const RowsArgs& ra) {
  int e = ensure(sg->ctx, sg->pth, sg->pth_cap, (size_t)rows_blocks(ra) * GPX_THETA_STRIDE);
  if (e != GPX_OK) return e;
  return ensure(sg->ctx, sg->pz, sg->pz_cap, (size_t)rows_chunks(ra) * sg->Mp * sg->D);
}

void sum_into(const double* src, long long stride, int nb, long long width, double* dst, hipStream_t s) {
  SumArgs a{src, stride, nb, width, dst, 0};
  launch_sum(a, s);
}

TrmvArgs trmv_args(const gpx_sgpr* sg, const double* Wm, const double* x, double* y) {
  TrmvArgs t{};
  t.active = sg->kmm->d_active; t.Wm = Wm; t.sW = 0; t.ld = sg->Mp; t.x = x; t.sx = 0;
  t.nvalid = nullptr; t.y = y; t.sy = 0; t.rows = t.cols = sg->Mp; t.lower = 1;
  return t;
}

// theta check + uploads shared by the bound and predict paths (all on stream s)
int prelude(gpx_sgpr* sg, const double* theta, const double* Z, hipStream_t s) {
  gpx_ctx* ctx = sg->ctx;
  if (!theta || !Z) return fail(ctx, GPX_BAD_ARG, "null sgpr argument");
  const int np = sg->spec.n_params;
  for (int p = 0; p <= np; ++p)
    if (!(theta[p] > 0.0) || !std::isfinite(theta[p]))
      return fail(ctx, GPX_BAD_ARG, "theta must be finite and > 0 (constrained space)");
  for (int e = 0; e < sg->M * sg->D; ++e)
    if (!std::isfinite(Z[e])) return fail(ctx, GPX_BAD_ARG, "Z must be finite");
  sg->h_theta.assign(theta, theta + GPX_THETA_STRIDE);
  std::vector<double> th_kmm(sg->h_theta);
  th_kmm[np] = kJitter;
  const int32_t act0 = 0;
  int rc = upload_common(sg->kmm, 1, &act0, th_kmm.data(), s);
  if (rc != GPX_OK) return rc;
  rc = upload_common(sg->bb, 1, &act0, th_kmm.data(), s);  // its active list and a zeroed info
  if (rc != GPX_OK) return rc;
  HIPX(ctx, hipMemcpyAsync(sg->d_theta, sg->h_theta.data(), sizeof(double) * GPX_THETA_STRIDE,
                           hipMemcpyHostToDevice, s));
  HIPX(ctx, hipMemcpyAsync(sg->dZ, Z, sizeof(double) * sg->M * sg->D, hipMemcpyHostToDevice, s));
  return GPX_OK;
}

// Steps 2-6 of an evaluation, shared with predict: Kmn, G (split-K SYRK) and w on s while the
// Kmm chain runs on the aux stream; then Ĝ, â, B and its factor, B⁻¹ pieces: WB, γ.
int forward(gpx_sgpr* sg, hipStream_t s) {
  gpx_ctx* ctx = sg->ctx;
  const int M = sg->M, Mp = sg->Mp, Nc = sg->Ncols, D = sg->D;
  const double s2 = sg->h_theta[sg->spec.n_params];
  const Run r{sg->kmm, sg->kmm->d_active, 1, s};
  double* W = sg->kmm->W;
  hipStream_t sa = sg->kmm->aux[0];
  hipEvent_t e_up = sg->kmm->ev[kEvents - 2], e_m = sg->kmm->ev[kEvents - 1];
  HIPX(ctx, hipEventRecord(e_up, s));
  // Kmn = k(Z, X) (rows ≥ M and columns ≥ N are zero)
  BuildArgs ba{};
  ba.active = sg->kmm->d_active; ba.specs = sg->kmm->d_specs; ba.theta = sg->d_theta;
  ba.nvalid = sg->kmm->d_n; ba.X = sg->dZ; ba.sX = 0; ba.X2 = sg->X; ba.sX2 = 0; ba.D = D;
  ba.m2 = sg->N; ba.out = sg->Kmn; ba.sOut = 0; ba.ldo = Nc; ba.rows = Mp; ba.cols = Nc;
  ba.symmetric = 0; ba.rows_valid = 0;
  launch_build(ba, 1, s);
  // G = Kmn Kmnᵀ (lower), split-K over nc column chunks, then summed
  {
    const Run rk{sg->kmm, sg->d_iota, sg->nc, s};
    GemmArgs gg = gemm_args(sg->Kmn, Nc, sg->Kmn, Nc, sg->Gpart, Mp, 0, Mp, Mp, sg->chunkK, 0, 1, 1.0, 0.0);
    gg.sA = sg->chunkK; gg.sB = sg->chunkK; gg.sC = (long long)Mp * Mp;
    gemm(rk, gg, EPI_STORE, false, true);
    sum_into(sg->Gpart, (long long)Mp * Mp, sg->nc, (long long)Mp * Mp, sg->G, s);
  }
  // w = Kmn y
  SgprRowDotArgs rd{};
  rd.A = sg->Kmn; rd.ld = Nc; rd.rows = Mp; rd.cols = sg->N; rd.x = sg->Y; rd.part = sg->pdot;
  launch_sgpr_rowdot(rd, s);
  sum_into(sg->pdot, Mp, sgpr_rowdot_chunks(sg->N), Mp, sg->w, s);
  // The Kmm chain (latency-bound recursive factorisation) runs on an auxiliary stream beside the
  // big launches above (enqueued first, so its many small launches do not delay them).
  HIPX(ctx, hipStreamWaitEvent(sa, e_up, 0));
  factor(Run{sg->kmm, sg->kmm->d_active, 1, sa});
  HIPX(ctx, hipEventRecord(e_m, sa));
  HIPX(ctx, hipStreamWaitEvent(s, e_m, 0));
  // Ĝ = W G Wᵀ,  â = W w
  launch_symmetrize_lower(sg->G, Mp, M, s);
  gemm(r, gemm_args(W, Mp, sg->G, Mp, sg->T, Mp, 0, Mp, Mp, Mp, TRI_KMAX_I, 0, 1.0, 0.0), EPI_STORE, false, false);
  gemm(r, gemm_args(sg->T, Mp, W, Mp, sg->Gh, Mp, 0, Mp, Mp, Mp, TRI_KMAX_J, 0, 1.0, 0.0), EPI_STORE,
       false, true);
  launch_trmv_n(trmv_args(sg, W, sg->w, sg->ahat), 1, s);
  // B = I + Ĝ/s (identity padding) into the second batch's K, factored in place: WB = LB⁻¹
  SgprBmatArgs bm{};
  bm.Gh = sg->Gh; bm.ld = Mp; bm.m = M; bm.np = Mp; bm.s = s2; bm.B = sg->bb->K;
  launch_sgpr_bmat(bm, s);
  chol_inv(Run{sg->bb, sg->bb->d_active, 1, s}, 0, Mp);
  // γ = WBᵀ (WB â)
  double* WB = sg->bb->W;
  launch_trmv_n(trmv_args(sg, WB, sg->ahat, sg->t1), 1, s);
  launch_trmv_t(trmv_args(sg, WB, sg->t1, sg->gam), 1, s);
  return GPX_OK;
}

int check_info(gpx_sgpr* sg, int32_t* info, hipStream_t s) {
  gpx_ctx* ctx = sg->ctx;
  HIPX(ctx, hipMemcpyAsync(&sg->h_info[0], sg->kmm->d_info, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipMemcpyAsync(&sg->h_info[1], sg->bb->d_info, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  if (info) { info[0] = sg->h_info[0]; info[1] = sg->h_info[1]; }
  if (sg->h_info[0] != 0) return fail(ctx, GPX_NOT_PD, "Kmm + jitter I is not positive definite");
  if (sg->h_info[1] != 0) return fail(ctx, GPX_NOT_PD, "B = I + W G Wᵀ/s is not positive definite");
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_sgpr_create(gpx_ctx* ctx, int N, int M, int D, const double* X, const double* Y,
                    const gpx_kernel_spec* spec, gpx_sgpr** out) {
  if (!ctx || !out) return GPX_BAD_ARG;
  *out = nullptr;
  if (N < 1 || M < 1 || D < 1 || D > GPX_MAX_DIM || !X || !Y || !spec)
    return fail(ctx, GPX_BAD_ARG, "bad sgpr dimensions or null pointer");
  if (ard_spec(*spec)) return fail(ctx, GPX_BAD_ARG, "ARD terms (GPX_TERM_ARD) are served by the gpx_batch_* entry points only");
  if (coreg_spec(*spec)) return fail(ctx, GPX_BAD_ARG, kCoregBatchOnlyMsg);
  HIPX(ctx, hipSetDevice(ctx->device));
  gpx_sgpr* sg = new gpx_sgpr();
  sg->ctx = ctx; sg->N = N; sg->M = M; sg->D = D; sg->X = X; sg->Y = Y; sg->spec = *spec;
  sg->Mp = ((M + kLeaf - 1) / kLeaf) * kLeaf;
  const int Mp = sg->Mp;
  // split-K chunks for G = Kmn Kmnᵀ: enough (problem, tile) pairs to fill the chip
  const long long n64 = ((long long)N + 63) / 64 * 64;
  sg->nc = (int)std::max(1LL, std::min(32LL, n64 / 1024));
  sg->chunkK = (int)(((n64 + sg->nc - 1) / sg->nc + 63) / 64 * 64);
  const long long ncols = (long long)sg->nc * sg->chunkK;
  if (ncols > kGemmMaxLd || Mp > kGemmMaxLd) {
    delete sg;
    return fail(ctx, GPX_BAD_ARG, "sgpr data too large for the GEMM buffer-load window (N <= ~2.1M rows)");
  }
  sg->Ncols = (int)ncols;
  sg->rows_chunk = rows_chunk_for(D);
  auto bail = [&](const std::string& m) {
    gpx_sgpr_destroy(sg);
    return fail(ctx, GPX_HIP_ERROR, m);
  };
  if (hipMalloc(&sg->dZ, sizeof(double) * Mp * D) != hipSuccess ||
      hipMalloc(&sg->dYdummy, sizeof(double) * Mp) != hipSuccess)
    return bail("out of device memory");
  if (hipMemset(sg->dZ, 0, sizeof(double) * Mp * D) != hipSuccess ||
      hipMemset(sg->dYdummy, 0, sizeof(double) * Mp) != hipSuccess)
    return bail("memset failed");
  const int32_t nM = M;
  for (gpx_batch** b : {&sg->kmm, &sg->bb}) {
    const int rc = gpx_batch_create(ctx, 1, M, D, sg->dZ, sg->dYdummy, &nM, spec, b);
    if (rc != GPX_OK) {
      gpx_sgpr_destroy(sg);
      return rc;
    }
    (*b)->small_tiles = 1;  // every M x M launch here is one problem: size tiles to fill the chip
  }
  const size_t mm = (size_t)Mp * Mp;
  double** mats[] = {&sg->G, &sg->T, &sg->Gh, &sg->Binv, &sg->H, &sg->Mid, &sg->P, &sg->Sb, &sg->V};
  for (double** p : mats)
    if (hipMalloc(p, sizeof(double) * mm) != hipSuccess || hipMemset(*p, 0, sizeof(double) * mm) != hipSuccess)
      return bail("out of device memory for M x M workspace");
  double** vecs[] = {&sg->w, &sg->ahat, &sg->t1, &sg->gam, &sg->gs, &sg->u};
  for (double** p : vecs)
    if (hipMalloc(p, sizeof(double) * Mp) != hipSuccess || hipMemset(*p, 0, sizeof(double) * Mp) != hipSuccess)
      return bail("out of device memory for M vectors");
  sg->off_thn = 0;
  sg->off_thm = sg->off_thn + GPX_THETA_STRIDE;
  sg->off_diag = sg->off_thm + GPX_THETA_STRIDE;
  sg->off_tr = sg->off_diag + kResidW;
  sg->off_ld = sg->off_tr + kTraces;
  sg->off_zn = sg->off_ld + 1;
  sg->off_zm = sg->off_zn + (long long)Mp * D;
  sg->fin_len = sg->off_zm + (long long)Mp * D;
  const size_t mn = (size_t)Mp * sg->Ncols;
  if (hipMalloc(&sg->Kmn, sizeof(double) * mn) != hipSuccess ||
      hipMalloc(&sg->Ybuf, sizeof(double) * mn) != hipSuccess ||
      hipMalloc(&sg->Gpart, sizeof(double) * mm * sg->nc) != hipSuccess ||
      hipMalloc(&sg->pdiag, sizeof(double) * sgpr_diag_blocks(N) * kResidW) != hipSuccess ||
      hipMalloc(&sg->pdot, sizeof(double) * sgpr_rowdot_chunks(N) * Mp) != hipSuccess ||
      hipMalloc(&sg->ptr, sizeof(double) * sgpr_final_blocks(M) * kTraces) != hipSuccess ||
      hipMalloc(&sg->fin, sizeof(double) * sg->fin_len) != hipSuccess ||
      hipMalloc(&sg->d_theta, sizeof(double) * GPX_THETA_STRIDE) != hipSuccess ||
      hipMalloc(&sg->d_iota, sizeof(int) * sg->nc) != hipSuccess)
    return bail("out of device memory for N-sized workspace");
  // upper tiles of the split-K partials are never written: keep them zero
  if (hipMemset(sg->Gpart, 0, sizeof(double) * mm * sg->nc) != hipSuccess) return bail("memset failed");
  std::vector<int> iota(sg->nc);
  for (int i = 0; i < sg->nc; ++i) iota[i] = i;
  if (hipMemcpy(sg->d_iota, iota.data(), sizeof(int) * sg->nc, hipMemcpyHostToDevice) != hipSuccess)
    return bail("upload failed");
  *out = sg;
  return GPX_OK;
}

int gpx_sgpr_destroy(gpx_sgpr* sg) {
  if (!sg) return GPX_BAD_ARG;
  (void)hipSetDevice(sg->ctx->device);
  if (sg->kmm) gpx_batch_destroy(sg->kmm);
  if (sg->bb) gpx_batch_destroy(sg->bb);
  for (void* p : {(void*)sg->dZ, (void*)sg->dYdummy, (void*)sg->d_theta, (void*)sg->G, (void*)sg->T,
                  (void*)sg->Gh, (void*)sg->Binv, (void*)sg->H, (void*)sg->Mid, (void*)sg->P, (void*)sg->Sb,
                  (void*)sg->V, (void*)sg->w, (void*)sg->ahat, (void*)sg->t1, (void*)sg->gam, (void*)sg->gs,
                  (void*)sg->u, (void*)sg->Kmn, (void*)sg->Ybuf, (void*)sg->Gpart, (void*)sg->pdiag,
                  (void*)sg->pdot, (void*)sg->ptr, (void*)sg->fin, (void*)sg->pth, (void*)sg->pz,
                  (void*)sg->d_iota, (void*)sg->Kms, (void*)sg->pA, (void*)sg->pB})
    if (p) (void)hipFree(p);
  delete sg;
  return GPX_OK;
}

int gpx_sgpr_elbo_grad(gpx_sgpr* sg, const double* theta, const double* Z, double* elbo,
                       double* grad_theta, double* grad_Z, int32_t* info, void* stream) {
  if (!sg) return GPX_BAD_ARG;
  gpx_ctx* ctx = sg->ctx;
  if (!elbo || !grad_theta || !grad_Z) return fail(ctx, GPX_BAD_ARG, "null output");
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  int rc = prelude(sg, theta, Z, s);
  if (rc != GPX_OK) return rc;
  const int M = sg->M, Mp = sg->Mp, Nc = sg->Ncols, D = sg->D, np = sg->spec.n_params;
  const double s2 = theta[np];
  const Run r{sg->kmm, sg->kmm->d_active, 1, s};
  double* W = sg->kmm->W;
  double* WB = sg->bb->W;
  // the N-row pass: Σ y², Σ k_nn, k̄_nn Σ ∂k_nn/∂θ
  SgprDiagArgs da{};
  da.X = sg->X; da.Y = sg->Y; da.D = D; da.n = sg->N; da.spec = sg->kmm->d_specs; da.theta = sg->d_theta;
  da.part = sg->pdiag;
  launch_sgpr_diag(da, s);
  sum_into(sg->pdiag, kResidW, sgpr_diag_blocks(sg->N), kResidW, sg->fin + sg->off_diag, s);
  rc = forward(sg, s);
  if (rc != GPX_OK) return rc;
  sum_into(sg->bb->ldiag, 1, Mp, 1, sg->fin + sg->off_ld, s);
  // B⁻¹ = WBᵀ WB, then H, the K̄mm middle matrix and the traces in one launch
  gemm(r, gemm_args(WB, Mp, WB, Mp, sg->Binv, Mp, 0, Mp, Mp, Mp, TRI_KMIN_I | TRI_KMIN_J, 0, 1.0, 0.0),
       EPI_STORE, true, false);
  SgprFinalArgs fa{};
  fa.Binv = sg->Binv; fa.Gh = sg->Gh; fa.gam = sg->gam; fa.ahat = sg->ahat; fa.s = s2; fa.m = M; fa.ld = Mp;
  fa.H = sg->H; fa.Mid = sg->Mid; fa.part = sg->ptr;
  launch_sgpr_final(fa, s);
  sum_into(sg->ptr, kTraces, sgpr_final_blocks(M), kTraces, sg->fin + sg->off_tr, s);
  // P = Wᵀ H W,  Y = P Kmn,  u = Wᵀ γ/s²
  gemm(r, gemm_args(sg->H, Mp, W, Mp, sg->T, Mp, 0, Mp, Mp, Mp, TRI_KMIN_J, 0, 1.0, 0.0), EPI_STORE,
       false, false);
  gemm(r, gemm_args(W, Mp, sg->T, Mp, sg->P, Mp, 0, Mp, Mp, Mp, TRI_KMIN_I, 0, 1.0, 0.0), EPI_STORE,
       true, false);
  gemm(r, gemm_args(sg->P, Mp, sg->Kmn, Nc, sg->Ybuf, Nc, 0, Mp, Nc, Mp, 0, 0, 1.0, 0.0), EPI_STORE,
       false, false);
  launch_vscale(sg->gam, sg->gs, Mp, 1.0 / (s2 * s2), s);
  launch_trmv_t(trmv_args(sg, W, sg->gs, sg->u), 1, s);
  // K̄mn = u yᵀ + Y contracted with ∂Kmn/∂θ and ∂Kmn/∂Z
  RowsArgs ro{};
  ro.Zr = sg->dZ; ro.Xc = sg->X; ro.D = D; ro.nrows = M; ro.ncols = sg->N; ro.Y = sg->Ybuf; ro.ldy = Nc;
  ro.sym = 0; ro.u = sg->u; ro.g = sg->Y; ro.zscale = 1.0; ro.spec = sg->kmm->d_specs;
  ro.theta = sg->d_theta; ro.chunk = sg->rows_chunk; ro.Mp = Mp;
  rc = rows_alloc(sg, ro);
  if (rc != GPX_OK) return rc;
  ro.part_theta = sg->pth; ro.part_z = sg->pz; ro.part_w = nullptr;
  HIPX(ctx, hipMemsetAsync(sg->pz, 0, sizeof(double) * rows_chunks(ro) * Mp * D, s));
  launch_rows(ro, sg->spec.n_terms == 1, s);
  sum_into(sg->pth, GPX_THETA_STRIDE, rows_blocks(ro), GPX_THETA_STRIDE, sg->fin + sg->off_thn, s);
  sum_into(sg->pz, (long long)Mp * D, rows_chunks(ro), (long long)Mp * D, sg->fin + sg->off_zn, s);
  // K̄mm = Wᵀ Mid W contracted with ∂Kmm/∂θ and ∂Kmm/∂Z (symmetric: factor 2 on Z)
  gemm(r, gemm_args(sg->Mid, Mp, W, Mp, sg->T, Mp, 0, Mp, Mp, Mp, TRI_KMIN_J, 0, 1.0, 0.0), EPI_STORE,
       false, false);
  gemm(r, gemm_args(W, Mp, sg->T, Mp, sg->Sb, Mp, 0, Mp, Mp, Mp, TRI_KMIN_I, 0, 1.0, 0.0), EPI_STORE,
       true, false);
  RowsArgs rm{};
  rm.Zr = sg->dZ; rm.Xc = sg->dZ; rm.D = D; rm.nrows = M; rm.ncols = M; rm.Y = sg->Sb; rm.ldy = Mp;
  rm.sym = 1; rm.u = nullptr; rm.g = nullptr; rm.zscale = 2.0; rm.spec = sg->kmm->d_specs;
  rm.theta = sg->d_theta; rm.chunk = sg->rows_chunk; rm.Mp = Mp;
  rc = rows_alloc(sg, rm);  // (grows only when M > N; hipFree then waits for the reads above)
  if (rc != GPX_OK) return rc;
  rm.part_theta = sg->pth; rm.part_z = sg->pz; rm.part_w = nullptr;
  HIPX(ctx, hipMemsetAsync(sg->pz, 0, sizeof(double) * rows_chunks(rm) * Mp * D, s));
  launch_rows(rm, sg->spec.n_terms == 1, s);
  sum_into(sg->pth, GPX_THETA_STRIDE, rows_blocks(rm), GPX_THETA_STRIDE, sg->fin + sg->off_thm, s);
  sum_into(sg->pz, (long long)Mp * D, rows_chunks(rm), (long long)Mp * D, sg->fin + sg->off_zm, s);
  HIPX(ctx, hipGetLastError());
  sg->h_fin.resize(sg->fin_len);
  HIPX(ctx, hipMemcpyAsync(sg->h_fin.data(), sg->fin, sizeof(double) * sg->fin_len, hipMemcpyDeviceToHost, s));
  rc = check_info(sg, info, s);  // (synchronises s)
  if (rc != GPX_OK) return rc;
  const double* f = sg->h_fin.data();
  const double* thn = f + sg->off_thn;
  const double* thm = f + sg->off_thm;
  const double* dg = f + sg->off_diag;
  const double yy = dg[16], knn = dg[17];
  const double trG = f[sg->off_tr], trBG = f[sg->off_tr + 1], gGg = f[sg->off_tr + 2], ag = f[sg->off_tr + 3];
  const double n = (double)sg->N;
  *elbo = -0.5 * n * std::log(2.0 * M_PI) - 0.5 * n * std::log(s2) - f[sg->off_ld] - yy / (2.0 * s2) +
          ag / (2.0 * s2 * s2) - knn / (2.0 * s2) + trG / (2.0 * s2);
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) grad_theta[p] = (p < np) ? thn[p] + thm[p] + dg[p] : 0.0;
  grad_theta[np] = -n / (2.0 * s2) + yy / (2.0 * s2 * s2) - ag / (s2 * s2 * s2) + knn / (2.0 * s2 * s2) -
                   trG / (2.0 * s2 * s2) + trBG / (2.0 * s2 * s2) + gGg / (2.0 * s2 * s2 * s2 * s2);
  const double* zn = f + sg->off_zn;
  const double* zm = f + sg->off_zm;
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < D; ++d) grad_Z[(size_t)m * D + d] = zn[(size_t)m * D + d] + zm[(size_t)m * D + d];
  return GPX_OK;
}

int gpx_sgpr_predict(gpx_sgpr* sg, const double* theta, const double* Z, const double* Xnew, int Mn,
                     int add_noise, double* mean, double* var, int32_t* info, void* stream) {
  if (!sg) return GPX_BAD_ARG;
  gpx_ctx* ctx = sg->ctx;
  if (!Xnew || Mn < 1 || !mean || !var) return fail(ctx, GPX_BAD_ARG, "bad predict args");
  if (((long long)Mn + 63) / 64 * 64 > kGemmMaxLd)
    return fail(ctx, GPX_BAD_ARG, "too many prediction points for one call (kGemmMaxLd): split Xnew");
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  int rc = prelude(sg, theta, Z, s);
  if (rc != GPX_OK) return rc;
  rc = forward(sg, s);
  if (rc != GPX_OK) return rc;
  const int Mp = sg->Mp, D = sg->D;
  const int Mnp = (Mn + 63) / 64 * 64;
  const double s2 = sg->h_theta[sg->spec.n_params];
  const Run r{sg->kmm, sg->kmm->d_active, 1, s};
  double* W = sg->kmm->W;
  double* WB = sg->bb->W;
  // V = WB W (both lower: k runs over j..i), so that WB A* = V Kms;  u = Wᵀ γ/s
  gemm(r, gemm_args(WB, Mp, W, Mp, sg->V, Mp, 0, Mp, Mp, Mp, TRI_KMAX_I | TRI_KMIN_J, 0, 1.0, 0.0),
       EPI_STORE, false, false);
  launch_vscale(sg->gam, sg->gs, Mp, 1.0 / s2, s);
  launch_trmv_t(trmv_args(sg, W, sg->gs, sg->u), 1, s);
  rc = ensure(ctx, sg->Kms, sg->kms_cap, (size_t)Mp * Mnp);
  if (rc != GPX_OK) return rc;
  BuildArgs ba{};
  ba.active = sg->kmm->d_active; ba.specs = sg->kmm->d_specs; ba.theta = sg->d_theta;
  ba.nvalid = sg->kmm->d_n; ba.X = sg->dZ; ba.sX = 0; ba.X2 = Xnew; ba.sX2 = 0; ba.D = D;
  ba.m2 = Mn; ba.out = sg->Kms; ba.sOut = 0; ba.ldo = Mnp; ba.rows = Mp; ba.cols = Mnp;
  ba.symmetric = 0; ba.rows_valid = 0;
  launch_build(ba, 1, s);
  TrmvArgs t = trmv_args(sg, sg->Kms, sg->u, mean);
  t.ld = Mnp; t.rows = Mp; t.cols = Mn; t.lower = 0;
  launch_trmv_t(t, 1, s);
  // column sums of squares of A* = W Kms and V Kms
  GemmArgs ga = gemm_args(W, Mp, sg->Kms, Mnp, nullptr, Mnp, 0, Mp, Mnp, Mp, TRI_KMAX_I, 0, 1.0, 0.0);
  ga.small_tiles = sg->kmm->small_tiles;  // the tile size gemm() will launch with
  const int nrt = Mp / gemm_tile(ga, 1);
  rc = ensure(ctx, sg->pA, sg->pa_cap, (size_t)nrt * Mnp);
  if (rc != GPX_OK) return rc;
  rc = ensure(ctx, sg->pB, sg->pb_cap, (size_t)nrt * Mnp);
  if (rc != GPX_OK) return rc;
  ga.partial = sg->pA; ga.sPartial = 0;
  gemm(r, ga, EPI_COLSUMSQ, false, false);
  GemmArgs gb = gemm_args(sg->V, Mp, sg->Kms, Mnp, nullptr, Mnp, 0, Mp, Mnp, Mp, TRI_KMAX_I, 0, 1.0, 0.0);
  gb.partial = sg->pB; gb.sPartial = 0;
  gemm(r, gb, EPI_COLSUMSQ, false, false);
  SvgpPredVarArgs pv{};
  pv.pA = sg->pA; pv.pB = sg->pB; pv.nrt = nrt; pv.ldp = Mnp; pv.Xnew = Xnew; pv.D = D; pv.M = Mn;
  pv.spec = sg->kmm->d_specs; pv.theta = sg->d_theta; pv.add_noise = add_noise; pv.var = var;
  launch_svgp_predvar(pv, s);
  HIPX(ctx, hipGetLastError());
  return check_info(sg, info, s);
}

}  // extern "C"
