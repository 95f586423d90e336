// gpx_vgp.hip — C ABI and host orchestration of the VGP ELBO / gradient / predict path
// (gpflow.models.VGP 2.9.1 with GPflow's defaults; the reference's cell at
// test_scripts/SVGP.py:402-437: SE kernel, StudentT likelihood, Scipy().minimize(model.training_loss,
// ...), predict_y). Whitened, full q_sqrt, zero mean, one output; the likelihood is Gaussian
// (variance s) or Student-t (scale, fixed df).
//
// With K̃ = k(X,X) + 1e-6 I, L = chol(K̃), W = L⁻¹, q = q_mu, R = tril(q_sqrt):
//   μ = L q,   A = L R,   v_n = Σ_j A_nj²
//   E = Σ_n ve(μ_n, v_n, y_n),   KL = ½(qᵀq + ‖R‖²_F − N − Σ log R_ii²),   ELBO = E − KL
//   g_μ = ∂E/∂μ,  g_v = ∂E/∂v,  g_φ = ∂E/∂φ  (φ: the Gaussian variance / the Student-t scale)
//   C = Lᵀ (g_v ∘ A),   t = Lᵀ g_μ
//   ∂q = t − q,   ∂R = tril(2C − R + diag(1/R_ii))
//   Lᵀ L̄ = t qᵀ + 2 C Rᵀ,   K̄ = sym(Wᵀ Φ(Lᵀ L̄) W),   ∂θ = Σ K̄ ∘ ∂K̃/∂θ
// ve is GPflow's variational expectation: closed form for the Gaussian, the 20-point
// Gauss–Hermite rule for Student-t (vgp_quad_kernel). Prediction at X*, A* = W k(X, X*):
//   mean = A*ᵀ q,   var = k** − Σ A*² + Σ (Rᵀ A*)²   (+ the likelihood's variance for predict_y)
//
// L explicitly: the factorisation keeps only W (and panels of L scattered over the recursion's
// buffers), so L is recovered as tril(K̃ Wᵀ) — K̃ rebuilt, one triangular GEMM, one pass that
// zeroes the upper triangle and puts the identity on the padding. In exact arithmetic K̃ Wᵀ = L;
// in fp64 its error is eps·cond(L) relative, the error W itself carries.
//
// Everything N×N runs on the fp64 MFMA GEMM with its triangular k-ranges; padding (rows and
// columns >= N): L and R the identity, q, g_μ and g_v zero, so it adds exactly nothing to any sum.
//
// Out of scope: mean functions, multi-output Y, full_cov, sharding, several VGPs per call.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "gpx_host.h"

using namespace gpx;

namespace {
constexpr double kJitter = 1e-6;  // gpflow.config.default_jitter()
}  // namespace

struct gpx_vgp {
  gpx_ctx* ctx = nullptr;
  int N = 0, D = 0, Np = 0, lik = 0, rows_chunk = 64;
  double df = 3.0, c0 = 0.0;
  const double* X = nullptr;
  const double* Y = nullptr;
  gpx_kernel_spec spec{};
  gpx_batch* kmm = nullptr;  // K̃ factorisation (B = 1 over X itself)
  double* d_theta = nullptr;
  double *Kt = nullptr, *Lm = nullptr, *A = nullptr, *GA = nullptr, *C = nullptr, *CRt = nullptr;
  double *Phi = nullptr, *T = nullptr, *Sb = nullptr, *dR = nullptr;             // [Np][Np]
  double *dq = nullptr, *mu = nullptr, *v = nullptr, *gmu = nullptr, *gv = nullptr, *u = nullptr;  // [Np]
  double *pq = nullptr, *pth = nullptr, *pz = nullptr;
  size_t pth_cap = 0, pz_cap = 0;
  // fin layout (one download): ∂R [N][N] | t = Lᵀg_μ [Np] | θ sums [16] | E, g_φ | info
  double* fin = nullptr;
  long long off_t = 0, off_th = 0, off_sc = 0, off_info = 0, fin_len = 0;
  // predict workspace
  double *Kms = nullptr, *pA = nullptr, *pB = nullptr;
  size_t kms_cap = 0, pa_cap = 0, pb_cap = 0;
  // host staging (pinned)
  double* h_R = nullptr;    // [Np][Np] q_sqrt: upper part zero, identity padding
  double* h_fin = nullptr;  // [fin_len]
  std::vector<double> h_q, h_theta, h_thdev;
  int h_info = 0;
};

namespace {

void sum_into(const double* src, long long stride, int nb, long long width, double* dst, hipStream_t s) {
  SumArgs a{src, stride, nb, width, dst, 0};
  launch_sum(a, s);
}

TrmvArgs trmv_args(const gpx_vgp* vg, const double* Wm, const double* x, double* y) {
  TrmvArgs t{};
  t.active = vg->kmm->d_active; t.Wm = Wm; t.sW = 0; t.ld = vg->Np; t.x = x; t.sx = 0;
  t.nvalid = nullptr; t.y = y; t.sy = 0; t.rows = t.cols = vg->Np; t.lower = 1;
  return t;
}

// argument checks + uploads shared by the ELBO and predict paths (all on stream s). slot is what
// the device θ row carries at n_params: the likelihood parameter, or predict_y's added variance.
int prelude(gpx_vgp* vg, const double* theta, const double* q_mu, const double* q_sqrt, double slot,
            hipStream_t s) {
  gpx_ctx* ctx = vg->ctx;
  if (!theta || !q_mu || !q_sqrt) return fail(ctx, GPX_BAD_ARG, "null vgp argument");
  const int np = vg->spec.n_params, N = vg->N, Np = vg->Np;
  for (int p = 0; p <= np; ++p)
    if (!(theta[p] > 0.0) || !std::isfinite(theta[p]))
      return fail(ctx, GPX_BAD_ARG, "theta must be finite and > 0 (constrained space)");
  for (int i = 0; i < N; ++i) {
    if (!std::isfinite(q_mu[i])) return fail(ctx, GPX_BAD_ARG, "q_mu must be finite");
    for (int j = 0; j <= i; ++j)
      if (!std::isfinite(q_sqrt[(size_t)i * N + j])) return fail(ctx, GPX_BAD_ARG, "q_sqrt must be finite");
    if (!(q_sqrt[(size_t)i * N + i] != 0.0)) return fail(ctx, GPX_BAD_ARG, "q_sqrt has a zero diagonal");
  }
  vg->h_theta.assign(theta, theta + GPX_THETA_STRIDE);
  std::vector<double> th_kmm(vg->h_theta);
  th_kmm[np] = kJitter;
  const int32_t act0 = 0;
  int rc = upload_common(vg->kmm, 1, &act0, th_kmm.data(), s);
  if (rc != GPX_OK) return rc;
  vg->h_thdev = vg->h_theta;
  vg->h_thdev[np] = slot;
  HIPX(ctx, hipMemcpyAsync(vg->d_theta, vg->h_thdev.data(), sizeof(double) * GPX_THETA_STRIDE,
                           hipMemcpyHostToDevice, s));
  vg->h_q.assign(Np, 0.0);
  std::memcpy(vg->h_q.data(), q_mu, sizeof(double) * N);
  for (int i = 0; i < N; ++i)
    std::memcpy(&vg->h_R[(size_t)i * Np], q_sqrt + (size_t)i * N, sizeof(double) * (i + 1));
  HIPX(ctx, hipMemcpyAsync(vg->dq, vg->h_q.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
  HIPX(ctx, hipMemcpyAsync(vg->dR, vg->h_R, sizeof(double) * Np * Np, hipMemcpyHostToDevice, s));
  return GPX_OK;
}

BuildArgs cross_build(const gpx_vgp* vg, const double* X2, int m2, double* out, int cols) {
  BuildArgs ba{};
  ba.active = vg->kmm->d_active; ba.specs = vg->kmm->d_specs; ba.theta = vg->d_theta;
  ba.nvalid = vg->kmm->d_n; ba.X = vg->X; ba.sX = 0; ba.X2 = X2; ba.sX2 = 0; ba.D = vg->D;
  ba.m2 = m2; ba.out = out; ba.sOut = 0; ba.ldo = cols; ba.rows = vg->Np; ba.cols = cols;
  ba.symmetric = 0; ba.rows_valid = 0;
  return ba;
}

}  // namespace

extern "C" {

int gpx_vgp_create(gpx_ctx* ctx, int N, int D, const double* X, const double* Y,
                   const gpx_kernel_spec* spec, int likelihood, double df, gpx_vgp** out) {
  if (!ctx || !out) return GPX_BAD_ARG;
  *out = nullptr;
  if (N < 1 || D < 1 || D > GPX_MAX_DIM || !X || !Y || !spec)
    return fail(ctx, GPX_BAD_ARG, "bad vgp dimensions or null pointer");
  if (ard_spec(*spec)) return fail(ctx, GPX_BAD_ARG, "ARD terms (GPX_TERM_ARD) are served by the gpx_batch_* entry points only");
  if (coreg_spec(*spec)) return fail(ctx, GPX_BAD_ARG, kCoregBatchOnlyMsg);
  if (likelihood != GPX_LIK_GAUSSIAN && likelihood != GPX_LIK_STUDENT_T)
    return fail(ctx, GPX_BAD_ARG, "unknown vgp likelihood");
  if (likelihood == GPX_LIK_STUDENT_T && (!(df > 0.0) || !std::isfinite(df)))
    return fail(ctx, GPX_BAD_ARG, "StudentT df must be finite and > 0");
  const long long np64 = ((long long)N + kLeaf - 1) / kLeaf * kLeaf;
  if (np64 > kGemmMaxLd)
    return fail(ctx, GPX_BAD_ARG, "vgp data too large for the GEMM buffer-load window");
  HIPX(ctx, hipSetDevice(ctx->device));
  gpx_vgp* vg = new gpx_vgp();
  vg->ctx = ctx; vg->N = N; vg->D = D; vg->X = X; vg->Y = Y; vg->spec = *spec;
  vg->lik = likelihood; vg->df = df; vg->Np = (int)np64;
  vg->c0 = likelihood == GPX_LIK_GAUSSIAN
               ? -0.5 * std::log(2.0 * M_PI)
               : std::lgamma(0.5 * (df + 1.0)) - std::lgamma(0.5 * df) - 0.5 * (std::log(df) + std::log(M_PI));
  vg->rows_chunk = rows_chunk_for(D);
  const int Np = vg->Np;
  auto bail = [&](const std::string& m) {
    gpx_vgp_destroy(vg);
    return fail(ctx, GPX_HIP_ERROR, m);
  };
  const int32_t nN = N;
  const int rc = gpx_batch_create(ctx, 1, N, D, X, Y, &nN, spec, &vg->kmm);
  if (rc != GPX_OK) {
    gpx_vgp_destroy(vg);
    return rc;
  }
  vg->kmm->small_tiles = 1;  // every N x N launch here is one problem: size tiles to fill the chip
  const size_t mm = (size_t)Np * Np;
  double** mats[] = {&vg->Kt, &vg->Lm, &vg->A, &vg->GA, &vg->C, &vg->CRt, &vg->Phi, &vg->T, &vg->Sb, &vg->dR};
  for (double** p : mats)
    if (hipMalloc(p, sizeof(double) * mm) != hipSuccess || hipMemset(*p, 0, sizeof(double) * mm) != hipSuccess)
      return bail("out of device memory for N x N workspace");
  double** vecs[] = {&vg->dq, &vg->mu, &vg->v, &vg->gmu, &vg->gv, &vg->u};
  for (double** p : vecs)
    if (hipMalloc(p, sizeof(double) * Np) != hipSuccess || hipMemset(*p, 0, sizeof(double) * Np) != hipSuccess)
      return bail("out of device memory for N vectors");
  vg->off_t = (long long)N * N;
  vg->off_th = vg->off_t + Np;
  vg->off_sc = vg->off_th + GPX_THETA_STRIDE;
  vg->off_info = vg->off_sc + 2;
  vg->fin_len = vg->off_info + 1;
  if (hipMalloc(&vg->fin, sizeof(double) * vg->fin_len) != hipSuccess ||
      hipMalloc(&vg->pq, sizeof(double) * vgp_quad_blocks(Np) * 2) != hipSuccess ||
      hipMalloc(&vg->d_theta, sizeof(double) * GPX_THETA_STRIDE) != hipSuccess)
    return bail("out of device memory");
  if (hipHostMalloc(&vg->h_R, sizeof(double) * mm, hipHostMallocNonCoherent) != hipSuccess ||
      hipHostMalloc(&vg->h_fin, sizeof(double) * vg->fin_len, hipHostMallocNonCoherent) != hipSuccess)
    return bail("out of pinned host memory");
  std::memset(vg->h_R, 0, sizeof(double) * mm);
  for (int i = N; i < Np; ++i) vg->h_R[(size_t)i * Np + i] = 1.0;
  *out = vg;
  return GPX_OK;
}

int gpx_vgp_destroy(gpx_vgp* vg) {
  if (!vg) return GPX_BAD_ARG;
  (void)hipSetDevice(vg->ctx->device);
  if (vg->kmm) gpx_batch_destroy(vg->kmm);
  if (vg->h_R) (void)hipHostFree(vg->h_R);
  if (vg->h_fin) (void)hipHostFree(vg->h_fin);
  for (void* p : {(void*)vg->d_theta, (void*)vg->Kt, (void*)vg->Lm, (void*)vg->A, (void*)vg->GA, (void*)vg->C,
                  (void*)vg->CRt, (void*)vg->Phi, (void*)vg->T, (void*)vg->Sb, (void*)vg->dR, (void*)vg->dq,
                  (void*)vg->mu, (void*)vg->v, (void*)vg->gmu, (void*)vg->gv, (void*)vg->u, (void*)vg->pq,
                  (void*)vg->pth, (void*)vg->pz, (void*)vg->fin, (void*)vg->Kms, (void*)vg->pA, (void*)vg->pB})
    if (p) (void)hipFree(p);
  delete vg;
  return GPX_OK;
}

int gpx_vgp_elbo_grad(gpx_vgp* vg, const double* theta, const double* q_mu, const double* q_sqrt,
                      double* elbo, double* grad_theta, double* grad_qmu, double* grad_qsqrt,
                      int32_t* info, void* stream) {
  if (!vg) return GPX_BAD_ARG;
  gpx_ctx* ctx = vg->ctx;
  if (!elbo || !grad_theta || !grad_qmu || !grad_qsqrt) return fail(ctx, GPX_BAD_ARG, "null output");
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const int N = vg->N, Np = vg->Np, D = vg->D, np = vg->spec.n_params;
  int rc = prelude(vg, theta, q_mu, q_sqrt, theta ? theta[np] : 0.0, s);
  if (rc != GPX_OK) return rc;
  const Run r{vg->kmm, vg->kmm->d_active, 1, s};
  double* W = vg->kmm->W;
  // W = L⁻¹ from K̃ (destroyed by the factorisation), then K̃ again and L = tril(K̃ Wᵀ)
  factor(r);
  launch_build(cross_build(vg, vg->X, N, vg->Kt, Np), 1, s);
  launch_diag_add(vg->Kt, Np, N, kJitter, s);
  gemm(r, gemm_args(vg->Kt, Np, W, Np, vg->Lm, Np, 0, Np, Np, Np, TRI_KMAX_J, 1, 1.0, 0.0), EPI_STORE,
       false, true);
  VgpLtriArgs lt{vg->Lm, N, Np};
  launch_vgp_ltri(lt, s);
  // A = L R (both lower: k runs over j..i),  μ = L q,  v_n = Σ_j A_nj²
  gemm(r, gemm_args(vg->Lm, Np, vg->dR, Np, vg->A, Np, 0, Np, Np, Np, TRI_KMAX_I | TRI_KMIN_J, 1, 1.0, 0.0),
       EPI_STORE, false, false);
  launch_trmv_n(trmv_args(vg, vg->Lm, vg->dq, vg->mu), 1, s);
  VgpRowsqArgs rs{};
  rs.A = vg->A; rs.ld = Np; rs.rows = Np; rs.gv = nullptr; rs.v = vg->v; rs.GA = nullptr;
  launch_vgp_rowsq(rs, s);
  // the variational expectations: E, g_μ, g_v, g_φ
  VgpQuadArgs qa{};
  qa.mu = vg->mu; qa.v = vg->v; qa.y = vg->Y; qa.n = N; qa.npad = Np; qa.lik = vg->lik;
  qa.phi = theta[np]; qa.df = vg->df; qa.c0 = vg->c0; qa.gmu = vg->gmu; qa.gv = vg->gv; qa.part = vg->pq;
  launch_vgp_quad(qa, s);
  sum_into(vg->pq, 2, vgp_quad_blocks(Np), 2, vg->fin + vg->off_sc, s);
  // C = Lᵀ (g_v ∘ A),  t = Lᵀ g_μ,  C Rᵀ (lower)
  rs.gv = vg->gv; rs.v = nullptr; rs.GA = vg->GA;
  launch_vgp_rowsq(rs, s);
  gemm(r, gemm_args(vg->Lm, Np, vg->GA, Np, vg->C, Np, 0, Np, Np, Np, TRI_KMIN_I | TRI_KMIN_J, 0, 1.0, 0.0),
       EPI_STORE, true, false);
  launch_trmv_t(trmv_args(vg, vg->Lm, vg->gmu, vg->fin + vg->off_t), 1, s);
  gemm(r, gemm_args(vg->C, Np, vg->dR, Np, vg->CRt, Np, 0, Np, Np, Np, TRI_KMAX_J, 1, 1.0, 0.0), EPI_STORE,
       false, true);
  VgpFinalArgs fa{};
  fa.C = vg->C; fa.CRt = vg->CRt; fa.t = vg->fin + vg->off_t; fa.q = vg->dq; fa.R = vg->dR; fa.n = N; fa.ld = Np;
  fa.Phi = vg->Phi; fa.Rbar = vg->fin; fa.info = vg->kmm->d_info; fa.info_out = vg->fin + vg->off_info;
  launch_vgp_final(fa, s);
  // K̄' = Wᵀ Φ W (symmetrised inside the contraction), ∂θ = Σ K̄ ∘ ∂K̃/∂θ
  gemm(r, gemm_args(W, Np, vg->Phi, Np, vg->T, Np, 0, Np, Np, Np, TRI_KMIN_I | TRI_KMIN_J, 0, 1.0, 0.0),
       EPI_STORE, true, false);
  gemm(r, gemm_args(vg->T, Np, W, Np, vg->Sb, Np, 0, Np, Np, Np, TRI_KMIN_J, 0, 1.0, 0.0), EPI_STORE,
       false, false);
  RowsArgs ro{};
  ro.Zr = vg->X; ro.Xc = vg->X; ro.D = D; ro.nrows = N; ro.ncols = N; ro.Y = vg->Sb; ro.ldy = Np;
  ro.sym = 1; ro.u = nullptr; ro.g = nullptr; ro.zscale = 0.0; ro.spec = vg->kmm->d_specs;
  ro.theta = vg->d_theta; ro.chunk = vg->rows_chunk; ro.Mp = Np;
  rc = ensure(ctx, vg->pth, vg->pth_cap, (size_t)rows_blocks(ro) * GPX_THETA_STRIDE);
  if (rc != GPX_OK) return rc;
  rc = ensure(ctx, vg->pz, vg->pz_cap, (size_t)rows_chunks(ro) * Np * D);  // (X is data: written, never read)
  if (rc != GPX_OK) return rc;
  ro.part_theta = vg->pth; ro.part_z = vg->pz; ro.part_w = nullptr;
  launch_rows(ro, vg->spec.n_terms == 1, s);
  sum_into(vg->pth, GPX_THETA_STRIDE, rows_blocks(ro), GPX_THETA_STRIDE, vg->fin + vg->off_th, s);
  HIPX(ctx, hipGetLastError());
  HIPX(ctx, hipMemcpyAsync(vg->h_fin, vg->fin, sizeof(double) * vg->fin_len, hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  const double* f = vg->h_fin;
  vg->h_info = (int)f[vg->off_info];
  if (info) *info = vg->h_info;
  if (vg->h_info != 0) return fail(ctx, GPX_NOT_PD, "K(X,X) + jitter I is not positive definite");
  double kl = -(double)N;
  for (int i = 0; i < N; ++i) {
    kl += vg->h_q[i] * vg->h_q[i];
    for (int j = 0; j <= i; ++j) {
      const double x = vg->h_R[(size_t)i * Np + j];
      kl += x * x;
    }
    kl -= std::log(vg->h_R[(size_t)i * Np + i] * vg->h_R[(size_t)i * Np + i]);
  }
  kl *= 0.5;
  *elbo = f[vg->off_sc] - kl;
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) grad_theta[p] = (p < np) ? f[vg->off_th + p] : 0.0;
  grad_theta[np] = f[vg->off_sc + 1];
  for (int i = 0; i < N; ++i) grad_qmu[i] = f[vg->off_t + i] - vg->h_q[i];
  std::memcpy(grad_qsqrt, f, sizeof(double) * (size_t)N * N);
  return GPX_OK;
}

int gpx_vgp_predict(gpx_vgp* vg, const double* theta, const double* q_mu, const double* q_sqrt,
                    const double* Xnew, int Mn, int predict_y, double* mean, double* var,
                    int32_t* info, void* stream) {
  if (!vg) return GPX_BAD_ARG;
  gpx_ctx* ctx = vg->ctx;
  if (!Xnew || Mn < 1 || !mean || !var) return fail(ctx, GPX_BAD_ARG, "bad predict args");
  if (((long long)Mn + 63) / 64 * 64 > kGemmMaxLd)
    return fail(ctx, GPX_BAD_ARG, "too many prediction points for one call (kGemmMaxLd): split Xnew");
  if (predict_y && vg->lik == GPX_LIK_STUDENT_T && !(vg->df > 2.0))
    return fail(ctx, GPX_BAD_ARG, "StudentT predict_y needs df > 2 (the variance is scale² df/(df − 2))");
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const int Np = vg->Np, D = vg->D, np = vg->spec.n_params;
  // the variance predict_y adds, in the θ row's noise slot (svgp_predvar_kernel reads it there)
  double add = 0.0;
  if (theta) add = vg->lik == GPX_LIK_GAUSSIAN ? theta[np] : theta[np] * theta[np] * vg->df / (vg->df - 2.0);
  int rc = prelude(vg, theta, q_mu, q_sqrt, predict_y ? add : 0.0, s);
  if (rc != GPX_OK) return rc;
  const Run r{vg->kmm, vg->kmm->d_active, 1, s};
  double* W = vg->kmm->W;
  factor(r);
  // u = Wᵀ q (mean = k(X, X*)ᵀ u),  V = Rᵀ W (so that Rᵀ A* = V k(X, X*))
  launch_trmv_t(trmv_args(vg, W, vg->dq, vg->u), 1, s);
  double* V = vg->C;
  gemm(r, gemm_args(vg->dR, Np, W, Np, V, Np, 0, Np, Np, Np, TRI_KMIN_I | TRI_KMIN_J, 0, 1.0, 0.0),
       EPI_STORE, true, false);
  const int Mnp = (Mn + 63) / 64 * 64;
  rc = ensure(ctx, vg->Kms, vg->kms_cap, (size_t)Np * Mnp);
  if (rc != GPX_OK) return rc;
  launch_build(cross_build(vg, Xnew, Mn, vg->Kms, Mnp), 1, s);
  TrmvArgs t = trmv_args(vg, vg->Kms, vg->u, mean);
  t.ld = Mnp; t.rows = Np; t.cols = Mn; t.lower = 0;
  launch_trmv_t(t, 1, s);
  // column sums of squares of A* = W Kms and V Kms
  GemmArgs ga = gemm_args(W, Np, vg->Kms, Mnp, nullptr, Mnp, 0, Np, Mnp, Np, TRI_KMAX_I, 0, 1.0, 0.0);
  ga.small_tiles = vg->kmm->small_tiles;  // the tile size gemm() will launch with
  const int nrt = Np / gemm_tile(ga, 1);
  rc = ensure(ctx, vg->pA, vg->pa_cap, (size_t)nrt * Mnp);
  if (rc != GPX_OK) return rc;
  rc = ensure(ctx, vg->pB, vg->pb_cap, (size_t)nrt * Mnp);
  if (rc != GPX_OK) return rc;
  ga.partial = vg->pA; ga.sPartial = 0;
  gemm(r, ga, EPI_COLSUMSQ, false, false);
  GemmArgs gb = gemm_args(V, Np, vg->Kms, Mnp, nullptr, Mnp, 0, Np, Mnp, Np, 0, 0, 1.0, 0.0);
  gb.partial = vg->pB; gb.sPartial = 0;
  gemm(r, gb, EPI_COLSUMSQ, false, false);
  SvgpPredVarArgs pv{};
  pv.pA = vg->pA; pv.pB = vg->pB; pv.nrt = nrt; pv.ldp = Mnp; pv.Xnew = Xnew; pv.D = D; pv.M = Mn;
  pv.spec = vg->kmm->d_specs; pv.theta = vg->d_theta; pv.add_noise = predict_y ? 1 : 0; pv.var = var;
  launch_svgp_predvar(pv, s);
  HIPX(ctx, hipGetLastError());
  HIPX(ctx, hipMemcpyAsync(&vg->h_info, vg->kmm->d_info, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPX(ctx, hipStreamSynchronize(s));
  if (info) *info = vg->h_info;
  if (vg->h_info != 0) return fail(ctx, GPX_NOT_PD, "K(X,X) + jitter I is not positive definite");
  return GPX_OK;
}

}  // extern "C"
