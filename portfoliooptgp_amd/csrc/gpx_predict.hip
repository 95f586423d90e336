// gpx_predict.hip — predictions from a batch's cached factors (re-factorising where θ moved):
// predict_impl and the predict entry points.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include "gpx_host.h"

using namespace gpx;

// gpx_batch_predict_samples' part of a predict call: the covariance stays in the batch's workspace
// and the sampler (gpx_sample.hip) runs on it behind the prediction, on the same stream, before the
// call's one synchronise. white / out are indexed by slot like mean. failed: bit 0 some K + σn²I,
// bit 1 some posterior covariance + jitter·I (which one gpx_last_error names)
struct SampleTail {
  int S; const double* white; double jitter; double* out;
  int failed;
};

extern "C" {

// Shared body of gpx_batch_predict (var != nullptr), gpx_batch_predict_full_cov (cov != nullptr)
// and gpx_batch_predict_samples (st != nullptr).
static int predict_impl(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                        const double* Xnew, int M, int add_noise, double* mean, double* var,
                        double* cov, int32_t* info, void* stream, bool train = false, bool rows = false,
                        SampleTail* st = nullptr) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if ((!train && (!Xnew || M <= 0)) || !mean || !(var || cov || st) || !info)
    return fail(ctx, GPX_BAD_ARG, "bad predict args");
  if (!train && ((long long)M + 63) / 64 * 64 > kGemmMaxLd)
    return fail(ctx, GPX_BAD_ARG, "too many prediction points for one call (kGemmMaxLd): split Xnew");
  if (!bt->deferred.empty() && active)
    for (int i = 0; i < n_active; ++i)
      if (active[i] >= 0 && active[i] < bt->B && bt->deferred[active[i]])
        return fail(ctx, GPX_BAD_ARG, "a problem has a deferred evaluation in flight");
  HIPX(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  SubClock pclk(bt);
  struct PredLap {  // (GPX_SUBMIT_STATS: the call's host time, whatever path it returns by)
    SubClock& c;
    ~PredLap() { c.lap(8); }
  } plap{pclk};
  // band storage: only predict at the training inputs from a cached banded factor at exactly
  // this θ stays here; every other problem is predicted on the dense fallback slots, one by one
  std::vector<int32_t> keep;
  int shadow_status = GPX_OK;
  // rows (train only): outputs [n_active, Nmax], row i for active[i]; orow[b] = i
  std::vector<int32_t> orow;
  if (rows) {
    if (!train || n_active <= 0 || n_active > bt->B || !active) return fail(ctx, GPX_BAD_ARG, "bad active set");
    orow.assign(bt->B, -1);
    for (int i = 0; i < n_active; ++i) {
      if (active[i] < 0 || active[i] >= bt->B) return fail(ctx, GPX_BAD_ARG, "active index out of range");
      // a slot listed twice would leave an earlier output row unwritten (uninitialised memory
      // returned as a prediction)
      if (orow[active[i]] >= 0) return fail(ctx, GPX_BAD_ARG, "a slot appears twice in the active set");
      orow[active[i]] = i;
    }
    for (int& o : orow) o = std::max(o, 0);  // (rows not in the call are never read)
  }
  auto out_row = [&](int b) -> size_t { return rows ? (size_t)orow[b] : (size_t)b; };
  if (bt->compact) {
    if (n_active <= 0 || n_active > bt->B || !active || !theta)
      return fail(ctx, GPX_BAD_ARG, "bad active set / theta");
    gpx_batch* sh = bt->shadow;
    const size_t nx = (size_t)bt->Nmax * bt->D;
    std::vector<double> th((size_t)kShadowSlots * GPX_THETA_STRIDE, 1.0);
    std::vector<int32_t> inf(kShadowSlots, 0);
    const int32_t act0 = 0;
    for (int i = 0; i < n_active; ++i) {
      const int b = active[i];
      if (b < 0 || b >= bt->B) return fail(ctx, GPX_BAD_ARG, "active index out of range");
      const bool cached = train && bt->fac_valid[b] && bt->fac_band[b] &&
                          std::memcmp(&bt->fac_theta[(size_t)b * GPX_THETA_STRIDE],
                                      theta + (size_t)b * GPX_THETA_STRIDE,
                                      sizeof(double) * GPX_THETA_STRIDE) == 0;
      if (cached) {
        keep.push_back(b);
        continue;
      }
      int rc = gpx_batch_rebind_device(sh, 0, bt->n[b], bt->X + b * nx, bt->Y + (size_t)b * bt->Nmax,
                                       &bt->specs[b], s);
      if (rc != GPX_OK) return rc;
      std::memcpy(th.data(), theta + (size_t)b * GPX_THETA_STRIDE, sizeof(double) * GPX_THETA_STRIDE);
      inf[0] = 0;
      if (train)
        rc = predict_impl(sh, 1, &act0, th.data(), nullptr, 0, add_noise, mean + out_row(b) * bt->Nmax,
                          var + out_row(b) * bt->Nmax, nullptr, inf.data(), s, true);
      else if (st) {
        // (the shadow's slot 0 stands for problem b: its white / out rows by offset)
        SampleTail sb{st->S, st->white + (size_t)b * st->S * M, st->jitter, st->out + (size_t)b * st->S * M, 0};
        rc = predict_impl(sh, 1, &act0, th.data(), Xnew + (size_t)b * M * bt->D, M, add_noise,
                          mean + (size_t)b * M, nullptr, nullptr, inf.data(), s, false, false, &sb);
        st->failed |= sb.failed;
      } else
        rc = predict_impl(sh, 1, &act0, th.data(), Xnew + (size_t)b * M * bt->D, M, add_noise,
                          mean + (size_t)b * M, var ? var + (size_t)b * M : nullptr,
                          cov ? cov + (size_t)b * M * M : nullptr, inf.data(), s);
      if (rc != GPX_OK && rc != GPX_NOT_PD) return rc;
      bt->timing.shadow_predicts += 1;
      info[b] = inf[0];
      if (rc == GPX_NOT_PD) shadow_status = GPX_NOT_PD;
    }
    if (n_active > (int)keep.size()) {
      SubClock sc2(bt);
      sc2.t = pclk.t;
      sc2.lap(10);  // (from the call's start: the shadow slots' synchronous predicts)
    }
    if (keep.empty()) return shadow_status;
    active = keep.data();
    n_active = (int)keep.size();
  }
  int rc = upload_common(bt, n_active, active, theta, s, true);
  if (rc != GPX_OK) return rc;
  if (bt->n_mean > 0) {
    rc = flush_means(bt, s);
    if (rc != GPX_OK) return rc;
  }
  // re-factorise the problems whose cached factor is not at exactly this theta. A cached
  // block-banded factorisation (gpx_band.hip) serves predict at the training inputs (it holds
  // α and the diagonal of K⁻¹); any other predict re-factorises densely.
  std::vector<int> refac, band_cached;
  for (int i = 0; i < n_active; ++i) {
    const int b = active[i];
    const bool same = bt->fac_valid[b] &&
                      std::memcmp(&bt->fac_theta[(size_t)b * GPX_THETA_STRIDE],
                                  theta + (size_t)b * GPX_THETA_STRIDE,
                                  sizeof(double) * GPX_THETA_STRIDE) == 0;
    if (!same || (bt->fac_band[b] && !train)) refac.push_back(b);
    else if (bt->fac_band[b]) band_cached.push_back(b);
  }
  // the asynchronous case (see below) records no phase events: destroying an event the device
  // has not reached yet would wait for it
  const bool async = train && refac.empty() && stream;
  PhaseTimer pt(ctx->profiling != 0 && !async, s);
  bt->flops_acc = 0.0;
  pt.mark();
  // device active list: [dense-factored problems | band-cached problems]
  std::vector<int32_t> order;
  order.reserve(n_active);
  for (int i = 0; i < n_active; ++i)
    if (std::find(band_cached.begin(), band_cached.end(), active[i]) == band_cached.end())
      order.push_back(active[i]);
  const int n_dense = (int)order.size();
  // specs with ARD terms last in each list, those with a Coregion term behind them: their K builds
  // and k** are the ARD / Coregion kernels' (n_ard counts both, as Run::n_ard)
  const auto iso_first = [&](int32_t b) { return dense_class(bt->specs[b]) == 0; };
  const auto not_cg = [&](int32_t b) { return dense_class(bt->specs[b]) != 2; };
  const int n_ard = (int)(order.end() - std::stable_partition(order.begin(), order.end(), iso_first));
  const int n_cg = (int)(order.end() - std::stable_partition(order.end() - n_ard, order.end(), not_cg));
  order.insert(order.end(), band_cached.begin(), band_cached.end());
  if (!refac.empty()) {
    const int r_ard = (int)(refac.end() - std::stable_partition(refac.begin(), refac.end(), iso_first));
    const int r_iso = (int)refac.size() - r_ard;
    const int r_cg = (int)(refac.end() - std::stable_partition(refac.end() - r_ard, refac.end(), not_cg));
    HIPX(ctx, hipMemcpyAsync(bt->d_active, refac.data(), sizeof(int) * refac.size(),
                             hipMemcpyHostToDevice, s));
    if (bt->n_mean > 0) {  // the re-factorised problems' α is solved against y − m(X; β) at this β
      const int e = mean_residuals(bt, bt->d_active, (int)refac.size(), s);
      if (e != GPX_OK) return e;
    }
    if (small64_on(bt)) {
      if (r_iso > 0) small64_eval(Run{bt, bt->d_active, r_iso, s}, false);
      if (r_ard > 0) {  // (an ARD problem of these sizes: the launch chain, as its evaluations)
        Run ra{bt, bt->d_active + r_iso, r_ard, s};
        ra.n_ard = r_ard;
        ra.n_cg = r_cg;
        factor(ra);
        alpha_solve(ra);
      }
    } else {
      Run rr{bt, bt->d_active, (int)refac.size(), s};
      rr.n_ard = r_ard;
      rr.n_cg = r_cg;
      factor(rr);
      alpha_solve(rr);
    }
  }
  if (!refac.empty() || n_dense < n_active || n_ard > 0)
    HIPX(ctx, hipMemcpyAsync(bt->d_active, order.data(), sizeof(int) * n_active, hipMemcpyHostToDevice, s));
  pt.mark();
  const int Np = bt->Np;
  if (train) {
    TrainPredArgs ta{};
    ta.active = bt->d_active; ta.W = bt->W; ta.sW = mat_stride(bt); ta.ld = Np;
    // (the original targets, with a mean function too: α then solves the residual, and
    // y − σn²α = m(X) + (r − σn²α) is already the mean of f at the training inputs)
    ta.alpha = bt->alpha; ta.sVec = Np; ta.Y = bt->Y; ta.sY = bt->Nmax; ta.nvalid = bt->d_n;
    ta.specs = bt->d_specs; ta.theta = bt->d_theta; ta.add_noise = add_noise;
    ta.mean = mean; ta.var = var; ta.sOut = bt->Nmax;
    if (rows) {
      HIPX(ctx, hipMemcpyAsync(bt->d_orow, orow.data(), sizeof(int) * bt->B, hipMemcpyHostToDevice, s));
      ta.orow = bt->d_orow;
    }
    if (n_dense > 0) launch_train_pred(ta, n_dense, Np, s);
    if (n_dense < n_active) {
      // banded: diag(K⁻¹) from the selected inverse in K's diagonal blocks
      TrainPredArgs tb = ta;
      tb.active = bt->d_active + n_dense; tb.W = bt->K; tb.ld = mat_ld(bt);
      launch_band_train_pred(tb, n_active - n_dense, Np, s);
    }
  } else {
  const int Mp = ((M + 63) / 64) * 64;
  // cross-covariance workspace [B][Np][Mp]
  const size_t need = (size_t)bt->B * Np * Mp;
  double* kxs;
  if ((size_t)Mp <= (size_t)Np) {
    kxs = bt->L;  // L is dead once W is formed
  } else {
    const int e = ensure(ctx, bt->kxs, bt->kxs_cap, need);
    if (e != GPX_OK) return e;
    kxs = bt->kxs;
  }
  const long long skx = (long long)Np * Mp;
  BuildArgs ba{};
  ba.active = bt->d_active; ba.specs = bt->d_specs; ba.theta = bt->d_theta; ba.nvalid = bt->d_n;
  ba.X = bt->X; ba.sX = (long long)bt->Nmax * bt->D; ba.X2 = Xnew; ba.sX2 = (long long)M * bt->D;
  ba.D = bt->D; ba.m2 = M; ba.out = kxs; ba.sOut = skx; ba.ldo = Mp; ba.rows = Np; ba.cols = Mp;
  ba.symmetric = 0;
  build_range(ba, n_active, n_ard, n_cg, s);
  // mean = Kxsᵀ α
  TrmvArgs t{};
  t.active = bt->d_active; t.Wm = kxs; t.sW = skx; t.ld = Mp; t.x = bt->alpha; t.sx = Np;
  t.nvalid = nullptr; t.y = mean; t.sy = M; t.rows = Np; t.cols = M; t.lower = 0;
  launch_trmv_t(t, n_active, s);
  // + m(X*) (the variances below are the zero-mean model's on the residual data)
  if (bt->n_mean > 0) mean_add(bt, bt->d_active, n_active, Xnew, M, mean, s);
  if (cov || st) {
    // A = W · Kxs stored; cov = K(X*,X*) − AᵀA (padded rows/cols of A are exactly zero)
    double* abuf;
    if ((size_t)Mp <= (size_t)Np) {
      abuf = bt->K;  // K is dead once W is formed
    } else {
      const int e = ensure(ctx, bt->abuf, bt->abuf_cap, need);
      if (e != GPX_OK) return e;
      abuf = bt->abuf;
    }
    const long long scv = (long long)Mp * Mp;
    {
      const int e = ensure(ctx, bt->covw, bt->covw_cap, (size_t)bt->B * scv);
      if (e != GPX_OK) return e;
    }
    BuildArgs kb = ba;
    kb.X = Xnew; kb.sX = (long long)M * bt->D; kb.rows_valid = M; kb.out = bt->covw; kb.sOut = scv;
    kb.ldo = Mp; kb.rows = Mp; kb.cols = Mp;
    build_range(kb, n_active, n_ard, n_cg, s);
    const Run rr{bt, bt->d_active, n_active, s};
    GemmArgs ga = gemm_args(bt->W, Np, kxs, Mp, abuf, Mp, 0, Np, Mp, Np, TRI_KMAX_I, 0, 1.0, 0.0);
    ga.sA = mat_stride(bt); ga.sB = skx; ga.sC = skx;
    gemm(rr, ga, EPI_STORE, false, false);
    GemmArgs gc = gemm_args(abuf, Mp, abuf, Mp, bt->covw, Mp, 0, Mp, Mp, Np, 0, 0, -1.0, 1.0);
    gc.sA = skx; gc.sB = skx; gc.sC = scv;
    gemm(rr, gc, EPI_STORE, true, false);
    for (int i = 0; cov && i < n_active; ++i) {
      const int b = active[i];
      HIPX(ctx, hipMemcpy2DAsync(cov + (size_t)b * M * M, sizeof(double) * M,
                                 bt->covw + (size_t)b * scv, sizeof(double) * Mp,
                                 sizeof(double) * M, M, hipMemcpyDeviceToDevice, s));
    }
    if (st) {
      // the sampler on the padded covariance where it lies (factored in place), no copy-out
      const long long Sp = ((long long)st->S + 63) / 64 * 64;
      {
        const int e = ensure(ctx, bt->samp, bt->samp_cap, (size_t)bt->B * 2 * Sp * Mp);
        if (e != GPX_OK) return e;
      }
      if (!bt->d_sinfo) HIPX(ctx, hipMalloc(&bt->d_sinfo, sizeof(int) * bt->B));
      SampleArgs sa{};
      sa.active = bt->d_active;
      sa.cov = bt->covw; sa.sCov = scv; sa.ldc = Mp;
      sa.white = st->white; sa.sWhite = (long long)st->S * M;
      sa.mean = mean; sa.sMean = M;
      sa.out = st->out; sa.sOut = (long long)st->S * M;
      sa.A = bt->covw; sa.sA = scv;
      sa.Wp = bt->samp; sa.P = bt->samp + Sp * Mp; sa.sW = 2 * Sp * Mp;
      sa.info = bt->d_sinfo;
      sa.M = M; sa.S = st->S; sa.Mp = Mp; sa.Sp = (int)Sp; sa.jitter = st->jitter;
      launch_sample_chain(sa, n_active, s);
    }
  } else {
  // A = W · Kxs with fused column sum of squares
  GemmArgs g = gemm_args(bt->W, Np, kxs, Mp, nullptr, Mp, 0, Np, Mp, Np, TRI_KMAX_I, 0, 1.0, 0.0);
  g.sA = mat_stride(bt); g.sB = skx; g.sC = 0;
  g.small_tiles = bt->small_tiles;  // the tile size gemm() will launch with
  const int bm = gemm_tile(g, n_active);
  const int nrt = Np / bm;
  const size_t pneed = (size_t)bt->B * nrt * Mp;
  {
    const int e = ensure(ctx, bt->pvp, bt->pvp_cap, pneed);
    if (e != GPX_OK) return e;
  }
  g.partial = bt->pvp; g.sPartial = (long long)nrt * Mp;
  gemm(Run{bt, bt->d_active, n_active, s}, g, EPI_COLSUMSQ, false, false);
  PredVarArgs pv{};
  pv.active = bt->d_active; pv.partial = bt->pvp; pv.sPartial = (long long)nrt * Mp;
  pv.nrowtiles = nrt; pv.ldp = Mp; pv.Xnew = Xnew; pv.sXnew = (long long)M * bt->D; pv.D = bt->D;
  pv.specs = bt->d_specs; pv.theta = bt->d_theta; pv.M = M; pv.add_noise = add_noise;
  pv.var = var; pv.sVar = M;
  if (n_active > n_ard) launch_predvar(pv, n_active - n_ard, s);
  if (n_ard > n_cg) {
    pv.active = bt->d_active + (n_active - n_ard);
    launch_predvar_ard(pv, n_ard - n_cg, s);
  }
  if (n_cg > 0) {
    pv.active = bt->d_active + (n_active - n_cg);
    launch_predvar_coreg(pv, n_cg, s);
  }
  }
  }
  pt.mark();
  HIPX(ctx, hipGetLastError());
  if (async) {
    // every problem predicted from its cached factor at exactly this θ (the fit's last
    // evaluation): nothing can fail, so the call returns without waiting for the device — the
    // outputs are ready in the order of the CALLER's stream (not with stream == NULL: the
    // library's own non-blocking stream is not ordered with the caller's default stream);
    // the upload out of h_io is fenced by io_ev
    if (!bt->io_ev) HIPX(ctx, hipEventCreateWithFlags(&bt->io_ev, hipEventDisableTiming));
    HIPX(ctx, hipEventRecord(bt->io_ev, s));
    bt->io_pending = true;
    bt->io_stream = s;
    for (int i = 0; i < n_active; ++i) info[active[i]] = 0;
    if (shadow_status == GPX_NOT_PD) last_error_slot() = "K + noise*I is not positive definite for some problem";
    return shadow_status;
  }
  HIPX(ctx, hipMemcpyAsync(bt->h_info, bt->d_info, sizeof(int) * bt->B, hipMemcpyDeviceToHost, s));
  std::vector<int> sinfo;
  if (st) {
    sinfo.assign(bt->B, 0);
    HIPX(ctx, hipMemcpyAsync(sinfo.data(), bt->d_sinfo, sizeof(int) * bt->B, hipMemcpyDeviceToHost, s));
  }
  HIPX(ctx, hipStreamSynchronize(s));
  if (pt.on) {
    bt->timing.factor_ms = pt.ms(0, 1);
    bt->timing.alpha_ms = 0.0;
    bt->timing.grad_ms = 0.0;
    bt->timing.predict_ms = pt.ms(1, 2);
    bt->timing.total_ms = pt.ms(0, 2);
    bt->timing.gemm_flops = bt->flops_acc;
  }
  int status = GPX_OK;
  for (int i = 0; i < n_active; ++i) {
    const int b = active[i];
    // info is only (re)computed for re-factorised problems; cached ones were OK
    const bool was_refac = std::find(refac.begin(), refac.end(), b) != refac.end();
    info[b] = was_refac ? bt->h_info[b] : 0;
    if (info[b] != 0) {
      status = GPX_NOT_PD;
      bt->fac_valid[b] = 0;
      if (st) st->failed |= 1;
    } else if (was_refac) {
      std::memcpy(&bt->fac_theta[(size_t)b * GPX_THETA_STRIDE], theta + (size_t)b * GPX_THETA_STRIDE,
                  sizeof(double) * GPX_THETA_STRIDE);
      bt->fac_valid[b] = 1;
      bt->fac_band[b] = 0;
    }
    if (st && info[b] == 0 && sinfo[b] != 0) {  // (K's factor is good and stays cached)
      info[b] = sinfo[b];
      status = GPX_NOT_PD;
      st->failed |= 2;
    }
  }
  if (shadow_status == GPX_NOT_PD) status = GPX_NOT_PD;
  if (status == GPX_NOT_PD) last_error_slot() = "K + noise*I is not positive definite for some problem";
  return status;
}

int gpx_batch_predict(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                      const double* Xnew, int M, int add_noise, double* mean, double* var,
                      int32_t* info, void* stream) {
  if (!var) return bt ? fail(bt->ctx, GPX_BAD_ARG, "bad predict args") : GPX_BAD_ARG;
  return predict_impl(bt, n_active, active, theta, Xnew, M, add_noise, mean, var, nullptr, info,
                      stream);
}

int gpx_batch_predict_train(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                            int add_noise, double* mean, double* var, int32_t* info, void* stream) {
  return predict_impl(bt, n_active, active, theta, nullptr, 0, add_noise, mean, var, nullptr, info,
                      stream, true);
}

int gpx_batch_predict_train_rows(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                                 int add_noise, double* mean, double* var, int32_t* info, void* stream) {
  return predict_impl(bt, n_active, active, theta, nullptr, 0, add_noise, mean, var, nullptr, info,
                      stream, true, true);
}

int gpx_batch_predict_full_cov(gpx_batch* bt, int n_active, const int32_t* active,
                               const double* theta, const double* Xnew, int M, double* mean,
                               double* cov, int32_t* info, void* stream) {
  if (!cov) return bt ? fail(bt->ctx, GPX_BAD_ARG, "bad predict args") : GPX_BAD_ARG;
  return predict_impl(bt, n_active, active, theta, Xnew, M, 0, mean, nullptr, cov, info, stream);
}

int gpx_batch_predict_samples(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                              const double* Xnew, int M, int S, const double* white, double jitter,
                              double* mean, double* out, int32_t* info, void* stream) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if (!active || !theta || !Xnew || !white || !mean || !out || !info)
    return fail(ctx, GPX_BAD_ARG, "gpx_batch_predict_samples: null pointer");
  if (M <= 0 || S <= 0) return fail(ctx, GPX_BAD_ARG, "gpx_batch_predict_samples: M and S must be positive");
  if (M > kSampleMaxM)
    return fail(ctx, GPX_BAD_ARG, "gpx_batch_predict_samples: M over the limit (gpx_sample_limits)");
  if (!(jitter >= 0.0) || !std::isfinite(jitter))
    return fail(ctx, GPX_BAD_ARG, "gpx_batch_predict_samples: jitter must be finite and >= 0");
  const long long rows = ((long long)M + 63) / 64 * 64 + ((long long)S + 63) / 64 * 64;
  if (n_active <= 0 || n_active > bt->B || (long long)n_active * rows > 0x7fffffffLL)
    return fail(ctx, GPX_BAD_ARG, "gpx_batch_predict_samples: bad active set, or too many problems x rows for one call");
  SampleTail st{S, white, jitter, out, 0};
  const int rc = predict_impl(bt, n_active, active, theta, Xnew, M, 0, mean, nullptr, nullptr, info, stream, false,
                              false, &st);
  if (rc == GPX_NOT_PD) {
    const char* k = "K + noise*I is not positive definite for some problem";
    const char* p = "the posterior covariance + jitter*I is not positive definite for some problem";
    last_error_slot() = (st.failed & 1) ? ((st.failed & 2) ? std::string(k) + "; " + p : std::string(k)) : std::string(p);
  }
  return rc;
}

}  // extern "C"
