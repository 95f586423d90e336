// gpx_eval.hip — one evaluation call from submit to delivery: the per-block band class, the lanes
// of the fused classes (band_fused_eval), the upload and the rebind flush, band storage's
// fallback slots, the deferred slow parts, and the submit / complete / query / deferred_* entry
// points. Host code only.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "gpx_host.h"

using namespace gpx;

namespace gpx {

void band_eval(const Run& r, int p, int max_terms) {
  gpx_batch* bt = r.bt;
  const int Np = bt->Np, nb = Np / kLeaf;
  const long long st = mat_stride(bt);
  const long long rowb = (long long)kLeaf * Np;  // one block row
  BuildArgs ba{};
  ba.active = r.d_act; ba.specs = bt->d_specs; ba.theta = bt->d_theta; ba.nvalid = bt->d_n;
  ba.X = bt->X; ba.sX = (long long)bt->Nmax * bt->D; ba.X2 = bt->X; ba.sX2 = ba.sX; ba.D = bt->D;
  ba.m2 = 0; ba.out = bt->K; ba.sOut = st; ba.ldo = Np; ba.rows = ba.cols = Np;
  ba.symmetric = 1; ba.band1 = p + 1;
  launch_build(ba, r.na, r.s);
  // forward: right-looking block Cholesky over the band; W_kk = L_kk⁻¹ from the leaf
  LeafArgs la{};
  la.active = r.d_act; la.K = bt->K; la.W = bt->W; la.sMat = st; la.ld = Np;
  la.ldiag = bt->ldiag; la.sVec = Np; la.info = bt->d_info;
  for (int k = 0; k < nb; ++k) {
    la.off = k * kLeaf;
    launch_leaf(la, r.na, r.s);
    const int q = std::min(p, nb - 1 - k);
    if (q == 0) continue;
    const long long okk = k * rowb + k * kLeaf, opan = (k + 1) * rowb + k * kLeaf,
                    owin = (k + 1) * rowb + (k + 1) * kLeaf;
    // L_panel = A_panel · W_kkᵀ
    gemm(r, gemm_args(bt->K + opan, Np, bt->W + okk, Np, bt->L + opan, Np, st, q * kLeaf, kLeaf, kLeaf,
                      TRI_KMAX_J, 0, 1.0, 0.0), EPI_STORE, false, true);
    // A_window −= L_panel L_panelᵀ (lower tiles)
    gemm(r, gemm_args(bt->L + opan, Np, bt->L + opan, Np, bt->K + owin, Np, st, q * kLeaf, q * kLeaf,
                      kLeaf, 0, 1, -1.0, 1.0), EPI_STORE, false, true);
  }
  BandSolveArgs sa{};
  sa.active = r.d_act; sa.W = bt->W; sa.L = bt->L; sa.sMat = st; sa.ld = Np;
  sa.Y = eval_y(bt); sa.sY = bt->Nmax; sa.nvalid = bt->d_n; sa.z = bt->z; sa.alpha = bt->alpha; sa.sVec = Np;
  sa.Np = Np; sa.p = p;
  launch_band_solve(sa, r.na, r.s);
  // backward: selected inversion into K's band blocks (K is dead after the leaves read it)
  //   G = L_panel W_kk (in place over the panel), Z_panel = −Z_window G,
  //   Z_kk = W_kkᵀ W_kk − Gᵀ Z_panel, and the panel mirrored above the diagonal
  BandTransposeArgs ta{};
  ta.active = r.d_act; ta.Z = bt->K; ta.sMat = st; ta.ld = Np;
  for (int k = nb - 1; k >= 0; --k) {
    const int q = std::min(p, nb - 1 - k);
    const long long okk = k * rowb + k * kLeaf, opan = (k + 1) * rowb + k * kLeaf,
                    owin = (k + 1) * rowb + (k + 1) * kLeaf;
    gemm(r, gemm_args(bt->W + okk, Np, bt->W + okk, Np, bt->K + okk, Np, st, kLeaf, kLeaf, kLeaf, 0, 0,
                      1.0, 0.0), EPI_STORE, true, false);
    if (q == 0) continue;
    gemm(r, gemm_args(bt->L + opan, Np, bt->W + okk, Np, bt->L + opan, Np, st, q * kLeaf, kLeaf, kLeaf,
                      TRI_KMIN_J, 0, 1.0, 0.0), EPI_STORE, false, false);
    gemm(r, gemm_args(bt->K + owin, Np, bt->L + opan, Np, bt->K + opan, Np, st, q * kLeaf, kLeaf,
                      q * kLeaf, 0, 0, -1.0, 0.0), EPI_STORE, false, false);
    ta.k = k;
    launch_band_transpose(ta, q, r.na, r.s);
    gemm(r, gemm_args(bt->L + opan, Np, bt->K + opan, Np, bt->K + okk, Np, st, kLeaf, kLeaf, q * kLeaf,
                      0, 0, -1.0, 1.0), EPI_STORE, true, false);
  }
  BandContractArgs ca{};
  ca.active = r.d_act; ca.Z = bt->K; ca.sMat = st; ca.ld = Np; ca.alpha = bt->alpha; ca.sVec = Np;
  ca.X = bt->X; ca.sX = (long long)bt->Nmax * bt->D; ca.D = bt->D; ca.specs = bt->d_specs;
  ca.theta = bt->d_theta; ca.nvalid = bt->d_n; ca.partial = bt->partial; ca.sPartial = bt->partial_stride;
  ca.Np = Np; ca.p = p;
  // column sums of K∘Z for the band check (the batch-wide buffer is grown on first use;
  // gpx_batch_lml_grad checked the allocation before launching anything)
  (void)hipMemsetAsync(bt->bres, 0, sizeof(double) * (size_t)bt->B * Np, r.s);
  ca.colsum = bt->bres; ca.sCol = Np;
  launch_band_contract(ca, max_terms, r.na, r.s);
  launch_band_check(r.d_act, bt->bres, Np, bt->d_n, bt->results, r.na, Np, r.s);
  ReduceArgs ra{};
  ra.active = r.d_act; ra.partial = bt->partial; ra.sPartial = bt->partial_stride;
  ra.ntiles = (p + 1) * nb; ra.z = bt->z; ra.sVec = Np; ra.ldiag = bt->ldiag;
  ra.nvalid = bt->d_n; ra.specs = bt->d_specs; ra.results = bt->results; ra.Np = Np;
  launch_reduce(ra, r.na, r.s);
}

// stream-order markers in the wave trace (diagnostic; no-op unless gpx_batch_wave_trace is on):
// 38 submit reached the device, 39 rebind gather done, 40 band16 work starts, 43 a lane's K band
// built, 41 the lanes joined, 42 reduce done, 44 the results' download done
static void trace_mark(gpx_batch* bt, int kind, hipStream_t s) {
  if (bt->d_wtrace) launch_wave_marker(bt->d_wtrace, bt->d_wtrace_n, bt->wtrace_cap, kind, s);
}

// ---- the lanes of a fused range ----
// r's active range is [band16 problems (n16, by width group) | p <= 1 problems (n1) | p = 2
// problems]. The width classes of the call are independent: each class's chain (its K band build,
// then its sweeps) is a *lane*, and the lanes run concurrently — the largest on the call's stream,
// the others on the batch's auxiliary streams, joined before the reduction. Serialised on one
// stream (GPX_BAND_LANES=0, the round-3 order) every class's sweeps — about the same latency
// whatever their problem count — followed each other, so a call lasted ~2 sweeps per class
// while the small classes held few waves.
LanePlan plan_lanes(int n_g16, const int* g16_q, const int* g16_n, int n16, int n1, int na, bool se1, int bcr_q,
                    int wide_from, const LaneLimits& lim, int Nmax) {
  LanePlan P;
  Lane* lanes = P.lanes;
  int& nl = P.nl;
  int off = 0;
  long long wso = 0;  // (the reduction lanes' workspace offsets, in group order)
  auto follows = [&](LaneKind k) { return nl > 0 && lanes[nl - 1].kind == k; };
  auto extend = [&](int g) {
    lanes[nl - 1].n += g16_n[g];
    lanes[nl - 1].g_end = g + 1;
  };
  // (bcr_q: each band16 width group as a block-cyclic-reduction chain of its own width,
  // gpx_bcr.hip: a problem's arithmetic depends on its own width only, not on the call's mix)
  int g = 0;
  for (; g < n_g16 && bcr_q > 0 && g16_q[g] <= kBcrMaxQ; ++g) {
    lanes[nl++] = Lane{LaneKind::Bcr, g, g + 1, g16_n[g], off, wso};
    off += g16_n[g];
    wso += (long long)g16_n[g] * bcr_ws_doubles(g16_q[g], Nmax);
  }
  for (; g < n_g16; ++g) {
    if (lim.wide_bcr && g16_q[g] > kBcrMaxQ) {
      // the widths 6..8 (always the tail of the groups) as ONE reduction chain of block size 128
      if (follows(LaneKind::BcrWide)) extend(g);
      else lanes[nl++] = Lane{LaneKind::BcrWide, g, g + 1, g16_n[g], off, wso};
      wso += (long long)g16_n[g] * bcr_ws_doubles(g16_q[g], Nmax);
      P.bcr_wide_evals += g16_n[g];
    } else if (wide_from > 0 && se1 && g16_q[g] >= std::max(wide_from, 4) && g16_q[g] <= lim.wide_qmax) {
      // (wide_from: the SE1 groups of width 4 and up as one lane, one band16_wide_kernel launch)
      if (follows(LaneKind::Wide16)) extend(g);
      else lanes[nl++] = Lane{LaneKind::Wide16, g, g + 1, g16_n[g], off, 0};
    } else {
      lanes[nl++] = Lane{LaneKind::Band16, g, g + 1, g16_n[g], off, 0};
    }
    off += g16_n[g];
  }
  if (n1 > 0) lanes[nl++] = Lane{LaneKind::Fused1, 0, 0, n1, n16, 0};
  if (n16 + n1 < na) lanes[nl++] = Lane{LaneKind::Fused2, 0, 0, na - n16 - n1, n16 + n1, 0};
  // the reduction lanes' workspace (their offsets were laid out in group order)
  for (int i = 0; i < nl; ++i) {
    const Lane& l = lanes[i];
    if (l.kind == LaneKind::Bcr || l.kind == LaneKind::BcrWide)
      P.ws_need = std::max(P.ws_need, l.wso + (long long)l.n * bcr_ws_doubles(l.kind == LaneKind::BcrWide ? kBcrWideQ
                                                                                                          : g16_q[l.g], Nmax));
  }
  std::sort(lanes, lanes + nl, [](const Lane& x, const Lane& y) { return x.n > y.n; });
  // GPX_LANE_ORDER=1: the small (slow-class) lanes are enqueued first, ahead of the bulk lane,
  // so their wavefronts reach the dispatcher before the bulk lane's fill the chip
  if (lim.lane_order == 1 && nl > 1) std::rotate(lanes, lanes + 1, lanes + nl);  // bulk lane last (on an aux stream)
  return P;
}

namespace {
// K's band is built per class on that class's stream (2 block diagonals for p <= 1, 3 for
// p = 2), so the p <= 1 build does not pay for the wider class and the two overlap
BuildArgs band_build_args(const Run& r) {
  gpx_batch* bt = r.bt;
  BuildArgs ba{};
  ba.active = r.d_act; ba.specs = bt->d_specs; ba.theta = r.theta ? r.theta : bt->d_theta; ba.nvalid = bt->d_n;
  ba.X = bt->X; ba.sX = (long long)bt->Nmax * bt->D; ba.X2 = bt->X; ba.sX2 = ba.sX; ba.D = bt->D;
  ba.m2 = 0; ba.out = bt->K; ba.sOut = mat_stride(bt); ba.ldo = mat_ld(bt); ba.rows = ba.cols = bt->Np;
  ba.symmetric = 1;
  return ba;
}

BandFusedArgs band_fused_args(const Run& r) {
  gpx_batch* bt = r.bt;
  BandFusedArgs fa{};
  fa.active = r.d_act; fa.bandp = r.bandp ? r.bandp : bt->d_bandp; fa.K = bt->K; fa.L = bt->L; fa.W = bt->W;
  fa.sMat = mat_stride(bt);
  fa.Y = eval_y(bt); fa.sY = bt->Nmax; fa.nvalid = bt->d_n; fa.z = bt->z; fa.alpha = bt->alpha;
  fa.ldiag = bt->ldiag; fa.sVec = bt->Np; fa.X = bt->X; fa.sX = (long long)bt->Nmax * bt->D; fa.D = bt->D;
  fa.specs = bt->d_specs; fa.theta = r.theta ? r.theta : bt->d_theta; fa.partial = bt->partial;
  fa.sPartial = bt->partial_stride;
  fa.info = r.info ? r.info : bt->d_info; fa.results = bt->results; fa.Np = bt->Np; fa.ld = mat_ld(bt);
  fa.wtrace = bt->d_wtrace; fa.wtrace_n = bt->d_wtrace_n; fa.wtrace_cap = bt->wtrace_cap;
  return fa;
}

// a reduction lane's chain of width qc (workspace: the lane's problems in slots of its layout, at
// the lane's offset)
BcrArgs bcr_args(const Run& r, const Lane& l, int qc) {
  gpx_batch* bt = r.bt;
  BcrArgs ca{};
  ca.active = r.d_act + l.off; ca.specs = bt->d_specs; ca.theta = r.theta ? r.theta : bt->d_theta; ca.nvalid = bt->d_n;
  ca.X = bt->X; ca.sX = (long long)bt->Nmax * bt->D; ca.D = bt->D; ca.Y = eval_y(bt); ca.sY = bt->Nmax;
  ca.sWs = bcr_ws_doubles(qc, bt->Nmax);
  ca.ws = *r.bcr_wsp + l.wso; ca.info = r.info ? r.info : bt->d_info;
  ca.z = bt->z; ca.ldiag = bt->ldiag; ca.alpha = bt->alpha; ca.sVec = bt->Np; ca.Np = bt->Np;
  ca.Kd = bt->K; ca.sMat = mat_stride(bt); ca.ld = mat_ld(bt);
  ca.partial = bt->partial; ca.sPartial = bt->partial_stride; ca.results = bt->results;
  return ca;
}

// what every lane of one band_fused_eval call shares
struct LaneCall {
  const Run& r;
  const int* g16_q;
  const int* g16_n;
  bool se1;
  int kband16, n1, max_terms;
  hipEvent_t* ev;
  hipEvent_t (*ev16)[4];
  BuildArgs ba;
  BandFusedArgs fa;
  hipEvent_t* ev16_of(int g) const { return ev16 ? ev16[g - r.ev16_g0] : nullptr; }
};

// Band16: K's band as the sweeps read it (the 16-row tiles (m, m − d), d <= Q; kband16 — 2, or 3
// when the class holds p = 2 problems — still tells the sweeps which entries are exact zeros by
// the 64-row bound), then the group's sweeps.
// Which SE1 band16 sweeps compute their K tiles from X (b16_inline_k: bit 0 forward, bit 1
// backward): a sweep that does not reads K's band — written by band16_build_kernel when the
// forward reads it too, by the forward itself when only the backward reads it (1: each K tile's
// exp once, the band through HBM once each way). Same bits every way.
void run_band16_lane(const LaneCall& c, const Lane& l, hipStream_t ls) {
  const int q = c.g16_q[l.g], kin = b16_inline_k();
  // SE1 classes compute their K tiles inside the sweeps (band16 KIN): no build launch (a
  // forward computing them while the backward reads the band writes the band itself). The
  // Q > kBand16MaxQAny classes hold SE1 problems only and always compute K inline, whatever
  // the rest of the call holds (se1 is the whole call's), so they never need the build.
  if (!(c.se1 && (kin & 1)) && q <= kBand16MaxQAny) {
    BuildArgs bg = c.ba;
    bg.active = c.r.d_act + l.off;
    launch_band16_build(bg, q, l.n, ls);
    trace_mark(c.r.bt, 43, ls);
  }
  BandFusedArgs f16 = c.fa;
  f16.kband = c.kband16;
  f16.active = c.r.d_act + l.off;
  f16.kstore = c.se1 && (kin & 1) && !(kin & 2);
  launch_band16(f16, q, c.max_terms, c.se1, kin, l.n, ls, c.ev16_of(l.g));
}

// Wide16: the wide SE1 groups' K bands (unless computed in the sweeps), then one launch. (The
// Q = 4, 5 classes of a deferred part, one wavefront per SIMD: there the exp on each sweep's chain
// costs more than a build launch; b16_inline_k_wide.) Every group's timing events span the launch.
void run_wide16_lane(const LaneCall& c, const Lane& l, hipStream_t ls) {
  const int kin_wide = b16_inline_k_wide();
  int goff = l.off;
  for (int g = l.g; g < l.g_end; ++g) {
    if (!(kin_wide & 1)) {
      BuildArgs bg = c.ba;
      bg.active = c.r.d_act + goff;
      launch_band16_build(bg, c.g16_q[g], c.g16_n[g], ls);
    }
    goff += c.g16_n[g];
  }
  BandFusedArgs f16 = c.fa;
  f16.kband = c.kband16;
  f16.active = c.r.d_act + l.off;
  f16.kstore = (kin_wide & 1) && !(kin_wide & 2);
  if (c.ev16)
    for (int g = l.g + 1; g < l.g_end; ++g) (void)hipEventRecord(c.ev16_of(g)[0], ls);
  launch_band16_wide(f16, kin_wide, l.n, ls, c.ev16_of(l.g), c.g16_q[l.g_end - 1]);
  if (c.ev16)
    for (int g = l.g + 1; g < l.g_end; ++g)
      for (int e = 1; e < 4; ++e) (void)hipEventRecord(c.ev16_of(g)[e], ls);
}

// Bcr / BcrWide: a reduction chain of the group's width, or of the widths 6..8 at block size 128
void run_bcr_lane(const LaneCall& c, const Lane& l, hipStream_t ls) {
  gpx_batch* bt = c.r.bt;
  const int qc = l.kind == LaneKind::BcrWide ? kBcrWideQ : c.g16_q[l.g];
  launch_bcr(bcr_args(c.r, l, qc), qc, c.max_terms, l.n, bt->Nmax, ls, &bt->bcr_graphs);
}

// Fused1 / Fused2: the 64-row classes (two 64-block diagonals of K for p <= 1, three for p = 2);
// the timed launch pair is the p <= 1 class's when there is one, else the p = 2 class's
void run_fused64_lane(const LaneCall& c, const Lane& l, hipStream_t ls) {
  const bool p2 = l.kind == LaneKind::Fused2;
  BuildArgs b = c.ba;
  b.active = c.r.d_act + l.off;
  b.band1 = p2 ? 3 : 2;
  launch_build(b, l.n, ls);
  BandFusedArgs f = c.fa;
  f.active = c.r.d_act + l.off;
  if (p2) launch_band_fused(f, c.max_terms, l.n, ls, c.n1 == 0 ? c.ev : nullptr);
  else launch_band_fused1(f, c.max_terms, l.n, ls, c.ev);
}

void run_lane(const LaneCall& c, const Lane& l, hipStream_t ls) {
  switch (l.kind) {
    case LaneKind::Band16: return run_band16_lane(c, l, ls);
    case LaneKind::Wide16: return run_wide16_lane(c, l, ls);
    case LaneKind::Bcr:
    case LaneKind::BcrWide: return run_bcr_lane(c, l, ls);
    case LaneKind::Fused1:
    case LaneKind::Fused2: return run_fused64_lane(c, l, ls);
  }
}

// the fused classes' one partial row per problem -> results
void reduce_fused(const Run& r) {
  gpx_batch* bt = r.bt;
  ReduceArgs ra{};
  ra.active = r.d_act; ra.partial = bt->partial; ra.sPartial = bt->partial_stride;
  ra.ntiles = 1; ra.z = bt->z; ra.sVec = bt->Np; ra.ldiag = bt->ldiag;
  ra.nvalid = bt->d_n; ra.specs = bt->d_specs; ra.results = bt->results; ra.Np = bt->Np;
  launch_reduce(ra, r.na, r.s);
}
}  // namespace

int band_fused_eval(const Run& r, int n16, int n_g16, const int* g16_q, const int* g16_n, bool se1, int kband16,
                     int n1, int max_terms, hipEvent_t* ev, hipEvent_t (*ev16)[4]) {
  gpx_batch* bt = r.bt;
  // plan
  const LaneLimits lim{wide_qmax(se1), wide_bcr_on(r.bcr_q > 0), knob_int(Knob::LaneOrder)};
  const LanePlan plan = plan_lanes(n_g16, g16_q, g16_n, n16, n1, r.na, se1, r.bcr_q, r.wide_from, lim, bt->Nmax);
  if (bt->ctx->profiling) bt->timing.bcr_wide_evals += plan.bcr_wide_evals;
  // grow the reduction lanes' workspace (with headroom: each regrowth frees, which synchronises)
  if (plan.ws_need > 0 && (size_t)plan.ws_need > *r.bcr_capp) {
    const int e = ensure(bt->ctx, *r.bcr_wsp, *r.bcr_capp, (size_t)plan.ws_need * 3 / 2);
    if (e != GPX_OK) return e;
  }
  trace_mark(bt, 40, r.s);
  // fork: GPX_BAND_LANE_STREAMS streams the lanes are spread over (the bulk lane alone on the
  // call's stream, the others round-robin on the rest). A process gets GPU_MAX_HW_QUEUES hardware
  // queues (the bench: 2, so that 8 processes stay within the 16 the GPU maps without
  // time-slicing) and streams beyond that share queues, where their kernels run in order
  const int nstreams = (knob_on(Knob::BandLanes) && !r.one_stream)
                           ? std::min(std::min(plan.nl, 1 + kAux), knob_int(Knob::BandLaneStreams)) : 1;
  auto lane_stream = [&](int i) { return (i == 0 || nstreams == 1) ? r.s : bt->aux[(i - 1) % (nstreams - 1)]; };
  const bool bcr_timed = r.bcr_q > 0 && bt->ctx->profiling && bt->bcr_ev[0];
  if (bcr_timed) (void)hipEventRecord(bt->bcr_ev[0], r.s);
  if (nstreams > 1) {
    (void)hipEventRecord(bt->ev[kEvents - 2], r.s);   // the call's uploads are in
    for (int i = 1; i < nstreams; ++i) (void)hipStreamWaitEvent(bt->aux[i - 1], bt->ev[kEvents - 2], 0);
  }
  // dispatch
  const LaneCall c{r, g16_q, g16_n, se1, kband16, n1, max_terms, ev, ev16, band_build_args(r), band_fused_args(r)};
  for (int i = 0; i < plan.nl; ++i) run_lane(c, plan.lanes[i], lane_stream(i));
  // join
  for (int i = 1; i < nstreams; ++i) {
    (void)hipEventRecord(bt->ev[kEvents - 4 - i], bt->aux[i - 1]);
    (void)hipStreamWaitEvent(r.s, bt->ev[kEvents - 4 - i], 0);
  }
  if (bcr_timed) (void)hipEventRecord(bt->bcr_ev[1], r.s);
  trace_mark(bt, 41, r.s);
  // reduce
  reduce_fused(r);
  trace_mark(bt, 42, r.s);
  return GPX_OK;
}

// The batch's auxiliary streams (the forked T products of the recursion) take the priority of
// the stream the caller evaluates on, so a batch submitted on a high-priority stream is high
// priority throughout. Called at the start of an evaluation, when the aux streams are idle (the
// previous evaluation joined them before returning).
static int match_aux_priority(gpx_batch* bt, hipStream_t s) {
  int p = 0;
  if (hipStreamGetPriority(s, &p) != hipSuccess) p = 0;
  if (p == bt->aux_priority) return GPX_OK;
  for (int g = 0; g < kAux; ++g) {
    if (bt->aux[g]) HIPX(bt->ctx, hipStreamDestroy(bt->aux[g]));
    bt->aux[g] = nullptr;
    HIPX(bt->ctx, hipStreamCreateWithPriority(&bt->aux[g], hipStreamNonBlocking, p));
  }
  bt->aux_priority = p;
  return GPX_OK;
}
int wait_io(gpx_batch* bt) {
  if (!bt->io_pending) return GPX_OK;
  gpx_ctx* ctx = bt->ctx;
  HIPX(ctx, hipEventSynchronize(bt->io_ev));
  bt->io_pending = false;
  return GPX_OK;
}

// An asynchronous predict (predict_impl, `async`) left kernels in flight on bt->io_stream that
// read the batch's device I/O block, n / specs and the predicted slots' factors. Every later
// writer of that state on another stream (the uploads and rebind gathers of the next call, and
// through their order that call's kernels, which overwrite the factors of rebound slots) first
// waits for those kernels on the device — no host synchronisation. On the same stream the order
// is already the stream's.
int fence_io(gpx_batch* bt, hipStream_t s) {
  if (!bt->io_pending || bt->io_stream == s) return GPX_OK;
  HIPX(bt->ctx, hipStreamWaitEvent(s, bt->io_ev, 0));
  return GPX_OK;
}

int flush_rebinds(gpx_batch* bt, hipStream_t s) {
  if (bt->n_dirty == 0 && bt->pend.empty()) return GPX_OK;
  gpx_ctx* ctx = bt->ctx;
  {
    const int e = fence_io(bt, s);
    if (e != GPX_OK) return e;
  }
  SubClock fc(bt);
  {
    const int e = wait_io(bt);
    if (e != GPX_OK) return e;
  }
  fc.lap(6);
  {
    const int rc = ensure_rebind_meta(bt);
    if (rc != GPX_OK) return rc;
  }
  const size_t nx = (size_t)bt->Nmax * bt->D, ny = bt->Nmax;
  const int nbx = (bt->Nmax + kBox - 1) / kBox;
  if (!bt->h_rdesc) {
    HIPX(ctx, hipHostMalloc(&bt->h_rdesc, sizeof(RebindDesc) * bt->B, hipHostMallocCoherent));
    HIPX(ctx, hipMalloc(&bt->d_box, sizeof(double) * (size_t)bt->B * nbx * bt->D * 2));
    HIPX(ctx, hipHostMalloc(&bt->h_box, sizeof(double) * (size_t)bt->B * nbx * bt->D * 2, hipHostMallocNonCoherent));
  }
  // host-staged slots: DMA from their pinned regions (non-coherent host memory: DMA, not
  // kernel reads, is what sees the CPU's writes whole)
  for (int b = 0; b < bt->B && bt->n_dirty > 0; ++b) {
    if (!bt->dirty[b]) continue;
    const double* hx = bt->h_stage + (size_t)b * bt->stage_stride;
    HIPX(ctx, hipMemcpyAsync(const_cast<double*>(bt->X) + (size_t)b * nx, hx, sizeof(double) * nx,
                             hipMemcpyHostToDevice, s));
    HIPX(ctx, hipMemcpyAsync(const_cast<double*>(bt->Y) + (size_t)b * ny, hx + nx, sizeof(double) * ny,
                             hipMemcpyHostToDevice, s));
    bt->dirty[b] = 0;
    --bt->n_dirty;
  }
  bt->n_dirty = 0;
  // device sources: one gather kernel for all of them (descriptors in coherent pinned memory),
  // which also returns their X boxes for the band tables
  int m = 0;
  const bool tables = band_shape(bt);
  int nbox = 0;
  for (const auto& e : bt->pend)
    bt->h_rdesc[m++] = RebindDesc{e.x, e.y, const_cast<double*>(bt->X) + (size_t)e.b * nx,
                                  const_cast<double*>(bt->Y) + (size_t)e.b * ny, e.n,
                                  tables && !e.boxed ? nbox++ : -1};
  for (auto& w : bt->rebind_waits)  // the device sources' producers (gpx_batch_rebind_device)
    if (w.armed) {
      if (w.s != s) HIPX(ctx, hipStreamWaitEvent(s, w.ev, 0));
      w.armed = false;
    }
  if (m > 0) {
    launch_rebind_gather(bt->h_rdesc, m, bt->Nmax, bt->D, bt->d_box, s);
    HIPX(ctx, hipGetLastError());
  }
  if (nbox > 0) {
    const size_t row = (size_t)nbx * bt->D * 2;
    HIPX(ctx, hipMemcpyAsync(bt->h_box, bt->d_box, sizeof(double) * row * nbox, hipMemcpyDeviceToHost, s));
    fc.skip();
    HIPX(ctx, hipStreamSynchronize(s));
    fc.lap(7);
    ++bt->box_syncs;
    int i = 0;
    for (const auto& e : bt->pend) {
      if (e.boxed) continue;
      const double* box = bt->h_box + row * i++;
      band_tables_boxes(bt, e.b, box);
      keep_slot_box(bt, e.b, box);
    }
  }
  bt->pend.clear();
  for (int b = 0; b < bt->B; ++b) {
    bt->h_nmeta[b] = bt->n[b];
    std::memcpy(&bt->h_specs[b], &bt->specs[b], sizeof(DevSpec));
  }
  HIPX(ctx, hipMemcpyAsync(bt->d_n, bt->h_nmeta, sizeof(int) * bt->B, hipMemcpyHostToDevice, s));
  HIPX(ctx, hipMemcpyAsync(bt->d_specs, bt->h_specs, sizeof(DevSpec) * bt->B, hipMemcpyHostToDevice, s));
  return GPX_OK;
}

// the active set and every active row's θ (kernel parameters + σn²: finite and > 0)
static int check_active_theta(gpx_batch* bt, int n_active, const int32_t* active, const double* theta) {
  gpx_ctx* ctx = bt->ctx;
  if (n_active <= 0 || n_active > bt->B || !active || !theta)
    return fail(ctx, GPX_BAD_ARG, "bad active set / theta");
  for (int i = 0; i < n_active; ++i)
    if (active[i] < 0 || active[i] >= bt->B) return fail(ctx, GPX_BAD_ARG, "active index out of range");
  for (int i = 0; i < n_active; ++i) {
    const int b = active[i];
    const int np = bt->specs[b].n_params;
    const unsigned sgn = signed_slot_mask(bt->specs[b]);  // (a Coregion term's W: any finite value)
    for (int p = 0; p <= np; ++p) {
      const double v = theta[(size_t)b * GPX_THETA_STRIDE + p];
      if ((!(v > 0.0) && !((sgn >> p) & 1u)) || !std::isfinite(v))
        return fail(ctx, GPX_BAD_ARG, "theta must be finite and > 0 (constrained space; a Coregion W: finite)");
    }
    // (a mean function's coefficients, behind the noise: any finite value, zero and negative too)
    for (int p = np + 1, e = np + 1 + mean_ncoef(bt, b); p < e; ++p)
      if (!std::isfinite(theta[(size_t)b * GPX_THETA_STRIDE + p]))
        return fail(ctx, GPX_BAD_ARG, "mean-function coefficients must be finite");
  }
  return GPX_OK;
}

int upload_common(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                  hipStream_t s, bool predict_block) {
  gpx_ctx* ctx = bt->ctx;
  {
    const int e = check_active_theta(bt, n_active, active, theta);
    if (e != GPX_OK) return e;
  }
  {
    const int e = flush_rebinds(bt, s);
    if (e != GPX_OK) return e;
  }
  {  // (the rebind flush above host-waits for it when it had work; here without rebinds)
    const int e = fence_io(bt, s);
    if (e != GPX_OK) return e;
  }
  // a deferred slow part copies the active list, θ and band widths it runs on out of the I/O
  // block on its own stream: this upload may overwrite them only after those copies
  if (bt->slow_in_armed) HIPX(bt->ctx, hipStreamWaitEvent(s, bt->slow_in, 0));
  char* hio = bt->h_io;
  if (predict_block) {  // (the last asynchronous predict's upload out of it has completed)
    SubClock pc(bt);
    const int e = wait_io(bt);
    pc.lap(9);
    if (e != GPX_OK) return e;
    if (!bt->h_io_pred) HIPX(ctx, hipHostMalloc(&bt->h_io_pred, bt->io_bytes, hipHostMallocNonCoherent));
    hio = bt->h_io_pred;
  }
  // one DMA from the pinned block (allocated non-coherent: the host reads and writes it as
  // ordinary cached memory, the DMAs at the call boundaries see it whole):
  // [active | info = 0 | bandp | theta] (every call ends with a stream synchronize, so the previous call's transfers out of h_io have completed; bandp is
  // written into h_bandp by gpx_batch_lml_grad before this)
  std::memcpy(hio, active, sizeof(int) * n_active);
  std::memset(hio + bt->io_info_off, 0, sizeof(int) * bt->B);
  std::memcpy(hio + bt->io_theta_off, theta, sizeof(double) * GPX_THETA_STRIDE * bt->B);
  HIPX(ctx, hipMemcpyAsync(bt->d_io, hio, bt->io_res_off, hipMemcpyHostToDevice, s));
  return GPX_OK;
}

}  // namespace gpx

extern "C" {

// Band storage's dense fallback: problem b of bt is rebound to a slot of bt->shadow (its X / Y
// rows gathered device to device by the shadow's next call) and evaluated there, in chunks of
// kShadowSlots; outputs land at row b as gpx_batch_lml_grad writes them.
static int shadow_lml_grad(gpx_batch* bt, const std::vector<int32_t>& ids, const double* theta,
                           double* lml, double* grad, int32_t* info, hipStream_t s) {
  gpx_batch* sh = bt->shadow;
  const size_t nx = (size_t)bt->Nmax * bt->D;
  std::vector<double> th((size_t)kShadowSlots * GPX_THETA_STRIDE, 1.0), l(kShadowSlots);
  std::vector<double> g((size_t)kShadowSlots * GPX_THETA_STRIDE);
  std::vector<int32_t> inf(kShadowSlots), act(kShadowSlots);
  int status = GPX_OK;
  for (size_t c = 0; c < ids.size(); c += kShadowSlots) {
    const int cnt = (int)std::min<size_t>(kShadowSlots, ids.size() - c);
    for (int k = 0; k < cnt; ++k) {
      const int b = ids[c + k];
      const int rc = gpx_batch_rebind_device(sh, k, bt->n[b], bt->X + b * nx, bt->Y + (size_t)b * bt->Nmax,
                                             &bt->specs[b], s);
      if (rc != GPX_OK) return rc;
      std::memcpy(&th[(size_t)k * GPX_THETA_STRIDE], theta + (size_t)b * GPX_THETA_STRIDE,
                  sizeof(double) * GPX_THETA_STRIDE);
      act[k] = k;
    }
    const int rc = gpx_batch_lml_grad(sh, cnt, act.data(), th.data(), l.data(), g.data(), inf.data(), s);
    if (rc != GPX_OK && rc != GPX_NOT_PD) return rc;
    bt->timing.shadow_evals += cnt;
    for (int k = 0; k < cnt; ++k) {
      const int b = ids[c + k];
      info[b] = inf[k];
      if (inf[k] != 0) status = GPX_NOT_PD;
      lml[b] = l[k];
      for (int p = 0; p <= bt->specs[b].n_params; ++p)
        grad[(size_t)b * GPX_THETA_STRIDE + p] = g[(size_t)k * GPX_THETA_STRIDE + p];
      bt->fac_valid[b] = 0;  // no factor of b is kept in bt
      bt->fac_band[b] = 0;
    }
  }
  if (status == GPX_NOT_PD) last_error_slot() = "K + noise*I is not positive definite for some problem";
  return status;
}

// Band storage: up to kShadowSlots fallback problems are submitted on the batch's fallback
// stream at _submit (after the call's rebind gather on s, which their inputs come from), so the
// dense evaluation runs beside the band sweeps; _complete collects it.
static int shadow_submit(gpx_batch* bt, const std::vector<int32_t>& ids, const double* theta, hipStream_t s) {
  gpx_ctx* ctx = bt->ctx;
  gpx_batch* sh = bt->shadow;
  if (!bt->shadow_s) {
    HIPX(ctx, hipStreamCreateWithFlags(&bt->shadow_s, hipStreamNonBlocking));
    HIPX(ctx, hipEventCreateWithFlags(&bt->shadow_ev, hipEventDisableTiming));
  }
  HIPX(ctx, hipEventRecord(bt->shadow_ev, s));
  HIPX(ctx, hipStreamWaitEvent(bt->shadow_s, bt->shadow_ev, 0));
  const size_t nx = (size_t)bt->Nmax * bt->D;
  std::vector<double> th((size_t)kShadowSlots * GPX_THETA_STRIDE, 1.0);
  std::vector<int32_t> act(ids.size());
  for (size_t k = 0; k < ids.size(); ++k) {
    const int b = ids[k];
    const int rc = gpx_batch_rebind_device(sh, (int)k, bt->n[b], bt->X + b * nx, bt->Y + (size_t)b * bt->Nmax,
                                           &bt->specs[b], bt->shadow_s);
    if (rc != GPX_OK) return rc;
    std::memcpy(&th[k * GPX_THETA_STRIDE], theta + (size_t)b * GPX_THETA_STRIDE, sizeof(double) * GPX_THETA_STRIDE);
    act[k] = (int32_t)k;
  }
  return gpx_batch_lml_grad_submit(sh, (int)ids.size(), act.data(), th.data(), bt->shadow_s);
}

static int shadow_collect(gpx_batch* bt, const std::vector<int32_t>& ids, double* lml, double* grad,
                          int32_t* info) {
  gpx_batch* sh = bt->shadow;
  std::vector<double> l(kShadowSlots), g((size_t)kShadowSlots * GPX_THETA_STRIDE);
  std::vector<int32_t> inf(kShadowSlots);
  const int rc = gpx_batch_lml_grad_complete(sh, l.data(), g.data(), inf.data());
  if (rc != GPX_OK && rc != GPX_NOT_PD) return rc;
  bt->timing.shadow_evals += (double)ids.size();
  int status = GPX_OK;
  for (size_t k = 0; k < ids.size(); ++k) {
    const int b = ids[k];
    info[b] = inf[k];
    if (inf[k] != 0) status = GPX_NOT_PD;
    lml[b] = l[k];
    for (int p = 0; p <= bt->specs[b].n_params; ++p)
      grad[(size_t)b * GPX_THETA_STRIDE + p] = g[k * GPX_THETA_STRIDE + p];
    bt->fac_valid[b] = 0;
    bt->fac_band[b] = 0;
  }
  return status;
}

// ---- deferred completion of the slow classes (gpx_batch_set_deferred) ----
// By default the slow part runs on a stream of its own, from copies of the call's inputs, so the
// next call's work does not queue behind it (the C2 bench: +14-18 % over the same-stream variant
// once the driver's calls are on a stream of their own). GPX_DEFER_STREAM=0: it
// follows the call's own work on the call's stream, after the call's download (the call
// completes at an event there), and delays the next call.
static bool defer_own_stream() { return knob_on(Knob::DeferStream); }
// GPX_SLOW_DIRECT (default 0 until measured): a deferred part's results written by its gather
// kernel into coherent pinned host buffers instead of two copy-engine downloads
static bool slow_direct() { return knob_on(Knob::SlowDirect); }

static int slow_setup(gpx_batch* bt) {
  gpx_ctx* ctx = bt->ctx;
  const size_t B = bt->B;
  if (!bt->d_slow_res) {
    HIPX(ctx, hipMalloc(&bt->d_slow_res, sizeof(double) * B * kResStride));
    HIPX(ctx, hipMalloc(&bt->d_slow_info_c, sizeof(int) * B));
  }
  if (!bt->slow_in) HIPX(ctx, hipEventCreateWithFlags(&bt->slow_in, hipEventDisableTiming));
  if (!defer_own_stream() || bt->slow_s) return GPX_OK;
  // GPX_SLOW_PRIORITY: the slow stream at the device's lowest (-1) or highest (1) stream priority
  // (streams of another priority take hardware queues of their own); 0 / unset: the default
  const int prio = knob_int(Knob::SlowPriority);
  if (prio != 0) {
    int least = 0, greatest = 0;
    HIPX(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPX(ctx, hipStreamCreateWithPriority(&bt->slow_s, hipStreamNonBlocking, prio > 0 ? greatest : least));
  } else {
    HIPX(ctx, hipStreamCreateWithFlags(&bt->slow_s, hipStreamNonBlocking));
  }
  HIPX(ctx, hipEventCreateWithFlags(&bt->slow_up, hipEventDisableTiming));
  HIPX(ctx, hipMalloc(&bt->d_slow_act, sizeof(int) * B));
  HIPX(ctx, hipMalloc(&bt->d_slow_theta, sizeof(double) * B * GPX_THETA_STRIDE));
  HIPX(ctx, hipMalloc(&bt->d_slow_bandp, sizeof(int) * B));
  HIPX(ctx, hipMalloc(&bt->d_slow_info, sizeof(int) * B));
  return GPX_OK;
}

// The slow part of a call: problems order[off .. off + n) of the uploaded active list (band16
// groups q/cnt, then the 64-row sweeps' p <= 1 problems (n1) and p = 2 ones), on slow_s, from
// copies of the active list / θ / widths so the next call's upload cannot change them under it
static int submit_slow(gpx_batch* bt, hipStream_t s, const int32_t* ids, int off, int n, int n_g16, const int* q,
                       const int* cnt, int n16, int n1, bool se1, int kband16, int max_terms, const double* theta) {
  gpx_ctx* ctx = bt->ctx;
  {
    const int e = slow_setup(bt);
    if (e != GPX_OK) return e;
  }
  std::unique_ptr<gpx_batch::SlowRec> rec;
  if (!bt->slow_pool.empty()) {
    rec = std::move(bt->slow_pool.back());
    bt->slow_pool.pop_back();
  } else {
    rec.reset(new gpx_batch::SlowRec());
    HIPX(ctx, hipEventCreateWithFlags(&rec->done, hipEventDisableTiming));
    const unsigned fl = slow_direct() ? hipHostMallocCoherent : hipHostMallocDefault;
    HIPX(ctx, hipHostMalloc(&rec->h_res, sizeof(double) * bt->B * kResStride, fl));
    HIPX(ctx, hipHostMalloc(&rec->h_info, sizeof(int) * bt->B, fl));
  }
  rec->ids.assign(ids, ids + n);
  // The wide launch's waves in reverse order, widest first (GPX_WIDE_REVERSE=0: ascending): its
  // workgroups are dispatched in index order as wave slots free up under the other processes'
  // sweeps, and a Q = 6..8 wave — 2-3x a Q = 4 / 5 wave's time — dispatched last used to end the
  // launch alone. Each wave's arithmetic is its own problem's, so the bits are unchanged; the
  // part's active copy and its result gather (rec->ids) take the same order.
  const bool wide_on = knob_on(Knob::DeferWide);
  int r0 = 0, r1 = 0;
  if (knob_on(Knob::WideReverse) && wide_on && se1 && defer_own_stream()) {
    const int wq = wide_launch_qmax(se1);
    int o = 0;
    r0 = r1 = -1;
    for (int g = 0; g < n_g16; ++g) {
      if (q[g] >= 4 && q[g] <= wq) {
        if (r0 < 0) r0 = o;
        r1 = o + cnt[g];
      }
      o += cnt[g];
    }
    if (r0 < 0) r0 = r1 = 0;
    std::reverse(rec->ids.begin() + r0, rec->ids.begin() + r1);
  }
  rec->theta.assign(theta, theta + (size_t)bt->B * GPX_THETA_STRIDE);
  rec->clear_events();
  // (the swept groups: the wide ones, Q > kBcrMaxQ, run as a reduction chain without band16 events)
  int g_sw = n_g16;
  while (wide_bcr_on(false) && g_sw > 0 && q[g_sw - 1] > kBcrMaxQ) --g_sw;
  rec->n_g16 = g_sw;
  rec->se1 = se1;
  for (int g = 0; g < n_g16; ++g) {
    rec->g16_q[g] = q[g];
    rec->g16_n[g] = cnt[g];
  }
  rec->p64.clear();
  const bool own = defer_own_stream();
  hipStream_t ss = own ? bt->slow_s : s;
  if (own) {
    HIPX(ctx, hipEventRecord(bt->slow_up, s));
    HIPX(ctx, hipStreamWaitEvent(ss, bt->slow_up, 0));
    // one launch of one-wave workgroups, not the runtime's three copies and a fill: its blit
    // kernels' multi-wave workgroups wait for free CU space behind the other processes' sweeps
    // (+2.8 % on the bench, profiles/r05_ab.md)
    launch_slow_inputs(bt->d_active + off, n, bt->d_slow_act, bt->d_theta, bt->d_slow_theta, bt->d_bandp,
                       bt->d_slow_bandp, bt->d_slow_info, bt->B, ss, r0, r1);
    HIPX(ctx, hipGetLastError());
    HIPX(ctx, hipEventRecord(bt->slow_in, ss));
    bt->slow_in_armed = true;
  }
  const bool fused64 = n > n16;
  if (ctx->profiling) {
    for (int g = 0; g < g_sw; ++g)
      for (int e = 0; e < 4; ++e) HIPX(ctx, hipEventCreate(&rec->fq16[g][e]));
    if (fused64) {
      for (int e = 0; e < 4; ++e) HIPX(ctx, hipEventCreate(&rec->fq[e]));
      // (the timed 64-row pair is the p <= 1 class's when there is one, else the p = 2 class's)
      const int t0 = n16, t1 = n1 > 0 ? n16 + n1 : n;
      for (int i = t0; i < t1; ++i) rec->p64.push_back(bt->h_bandp[ids[i]]);
    }
  }
  // (on the call's stream, after its download: the next call's upload follows this part in the
  // stream's order, so the part reads the call's own active list, θ and widths in place)
  Run r{bt, own ? bt->d_slow_act : bt->d_active + off, n, ss};
  r.bcr_wsp = &bt->bcr_ws_slow;
  r.bcr_capp = &bt->bcr_ws_slow_cap;
  if (own) {
    r.theta = bt->d_slow_theta;
    r.bandp = bt->d_slow_bandp;
    r.info = bt->d_slow_info;
  }
  // GPX_DEFER_LANES=1: the part's lanes (the wide band16 launch; the 64-row sweeps) on the
  // batch's lane streams, joined on ss, instead of one after another on ss
  r.one_stream = !knob_on(Knob::DeferLanes);
  // the part's band16 classes as one launch (band16_wide_kernel), or (GPX_DEFER_WIDE=0) one
  // forward and one backward launch per class, each at its own occupancy
  r.wide_from = wide_on ? 1 : 0;
  {
    const int e = band_fused_eval(r, n16, n_g16, q, cnt, se1, kband16, n1, max_terms,
                                  (ctx->profiling && fused64) ? rec->fq : nullptr, ctx->profiling ? rec->fq16 : nullptr);
    if (e != GPX_OK) return e;
  }
  const int slow_delay = knob_int(Knob::SlowDelayUs);
  if (slow_delay > 0) launch_spin_us(slow_delay, ss);
  if (slow_direct()) {
    // the gather writes the part's result rows straight into the record's coherent pinned
    // buffers: no copy-engine download on the slow stream, whose deferred parts follow each
    // other (their length is what deferred fits wait)
    launch_slow_gather(r.d_act, n, bt->results, kResStride, rec->h_res, own ? bt->d_slow_info : bt->d_info,
                       rec->h_info, ss);
  } else {
    launch_slow_gather(r.d_act, n, bt->results, kResStride, bt->d_slow_res, own ? bt->d_slow_info : bt->d_info,
                       bt->d_slow_info_c, ss);
    HIPX(ctx, hipMemcpyAsync(rec->h_res, bt->d_slow_res, sizeof(double) * n * kResStride, hipMemcpyDeviceToHost, ss));
    HIPX(ctx, hipMemcpyAsync(rec->h_info, bt->d_slow_info_c, sizeof(int) * n, hipMemcpyDeviceToHost, ss));
  }
  HIPX(ctx, hipEventRecord(rec->done, ss));
  if (!own) {
    // same-stream mode reads the call's active list, θ, widths and info in place: the next
    // upload into them (from any stream) waits for the part to finish (upload_common)
    HIPX(ctx, hipEventRecord(bt->slow_in, ss));
    bt->slow_in_armed = true;
  }
  HIPX(ctx, hipGetLastError());
  if (bt->deferred.size() != (size_t)bt->B) bt->deferred.assign(bt->B, 0);
  for (int i = 0; i < n; ++i) {
    bt->deferred[ids[i]] = 1;
    bt->fac_valid[ids[i]] = 0;
  }
  bt->slow_out.push_back(std::move(rec));
  return GPX_OK;
}

// ---- delivery: what _complete and a finished slow part have in common ----
static const char* const kNotPdMessage = "K + noise*I is not positive definite for some problem";

// One finished row (its result row `res`, its `inf`) into the caller's arrays and the factor
// cache (θ from `theta`, the call's B × GPX_THETA_STRIDE rows). band: the row ran on a banded path,
// so its band check applies and the cached factor is the banded one. False when the check failed:
// nothing is written and the caller re-evaluates the row densely (redo_dense).
static bool deliver_row(gpx_batch* bt, int b, const double* res, int inf, bool band, double band_tol,
                        const double* theta, double* lml, double* grad, int32_t* info, int& status) {
  const int np = bt->specs[b].n_params + mean_ncoef(bt, b);  // (the mean's coefficients follow the noise)
  if (band && inf == 0 && !(res[kResBandCheck] <= band_tol)) return false;
  info[b] = inf;
  if (inf != 0) {
    status = GPX_NOT_PD;
    lml[b] = NAN;
    for (int p = 0; p <= np; ++p) grad[(size_t)b * GPX_THETA_STRIDE + p] = NAN;
    bt->fac_valid[b] = 0;
    return true;
  }
  lml[b] = res[0];
  for (int p = 0; p <= np; ++p) grad[(size_t)b * GPX_THETA_STRIDE + p] = res[1 + p];
  std::memcpy(&bt->fac_theta[(size_t)b * GPX_THETA_STRIDE], theta + (size_t)b * GPX_THETA_STRIDE,
              sizeof(double) * GPX_THETA_STRIDE);
  bt->fac_valid[b] = 1;
  bt->fac_band[b] = band;
  return true;
}

// Profiling: one band16 width group (n problems of width q) from its four events (forward start /
// end, backward start / end). in_wide: the group ran inside a deferred part's wide launch
// (band_fused_eval's Wide16 lane): every one of that launch's groups' events spans the one kernel,
// so the launch is counted once (wide_seen), apart from the per-class launches.
static void time_band16_group(gpx_batch* bt, hipEvent_t* ev, int q, int n, bool in_wide, bool& wide_seen) {
  float f0 = 0.f, f1 = 0.f;
  (void)hipEventElapsedTime(&f0, ev[0], ev[1]);
  (void)hipEventElapsedTime(&f1, ev[2], ev[3]);
  gpx_timing& t = bt->timing;
  if (in_wide) {
    if (!wide_seen) {
      t.band16_wide_ms_total += f0;
      t.band16_wide_launches += 1.0;
      wide_seen = true;
    }
    t.band16_wide_flops += n * (band16_flops(bt->Np, q, true) + band16_flops(bt->Np, q, false));
    t.band16_wide_evals += n;
    t.band16_wave_ms += (double)n * (double)f0;
  } else {
    t.band16_fwd_ms_total += f0;
    t.band16_bwd_ms_total += f1;
    t.band16_wave_ms += (double)n * ((double)f0 + (double)f1);
    t.band16_launches += 1.0;
    t.band16_fwd_flops += n * band16_flops(bt->Np, q, true);
    t.band16_bwd_flops += n * band16_flops(bt->Np, q, false);
  }
  t.band16_evals += n;
  t.band16_q_sum += (double)q * n;
}

// Profiling: the timed 64-row launch pair (the p <= 1 class's when there is one, else the p = 2
// class's: p2_only) from its four events; p64: the band widths of the pair's problems
static void time_fused64_pair(gpx_batch* bt, hipEvent_t* ev, const std::vector<int>& p64, bool p2_only) {
  float f0 = 0.f, f1 = 0.f;
  (void)hipEventElapsedTime(&f0, ev[0], ev[1]);
  (void)hipEventElapsedTime(&f1, ev[2], ev[3]);
  bt->timing.band_fwd_ms_total += f0;
  bt->timing.band_bwd_ms_total += f1;
  bt->timing.band_fused_launches += 1.0;
  if (p2_only) bt->timing.band_fused_p2_launches += 1.0;
  for (int pb : p64) {
    bt->timing.band_fwd_flops += band_fused_flops(bt->Np, pb, true);
    bt->timing.band_bwd_flops += band_fused_flops(bt->Np, pb, false);
  }
}

// The rows `ids` re-evaluated on the dense path at `theta` on s (band storage: on the fallback
// slots): rows whose band check failed, and band storage's rows that were routed dense
static int redo_dense(gpx_batch* bt, const std::vector<int32_t>& ids, const double* theta, double* lml,
                      double* grad, int32_t* info, hipStream_t s, int& status) {
  if (ids.empty()) return GPX_OK;
  int rc;
  if (bt->compact) {
    rc = shadow_lml_grad(bt, ids, theta, lml, grad, info, s);
  } else {
    bt->force_dense = 1;
    rc = gpx_batch_lml_grad(bt, (int)ids.size(), ids.data(), theta, lml, grad, info, s);
    bt->force_dense = 0;
  }
  if (rc != GPX_OK && rc != GPX_NOT_PD) return rc;
  if (rc == GPX_NOT_PD) status = GPX_NOT_PD;
  return GPX_OK;
}

// A finished slow part's results into the caller's arrays, as _complete reports its own rows
// (band-check failures re-evaluated densely here)
static int deliver_slow(gpx_batch* bt, gpx_batch::SlowRec& rec, double* lml, double* grad, int32_t* info) {
  gpx_ctx* ctx = bt->ctx;
  const double band_tol = knob_real(Knob::BandTol);
  int status = GPX_OK;
  std::vector<int32_t> redo;
  const int n = (int)rec.ids.size();
  for (int i = 0; i < n; ++i) {
    const int b = rec.ids[i];
    bt->deferred[b] = 0;
    // (a redone row's info is written by the dense re-evaluation, once that succeeds)
    if (!deliver_row(bt, b, rec.h_res + (size_t)i * kResStride, rec.h_info[i], true, band_tol, rec.theta.data(), lml,
                     grad, info, status))
      redo.push_back(b);
  }
  if (ctx->profiling) {
    bt->timing.band_evals += n;
    bt->timing.evals += n;
    bool wide_seen = false;
    for (int g = 0; g < rec.n_g16; ++g) {
      const int q = rec.g16_q[g];
      const bool in_wide = rec.se1 && q >= 4 && q <= wide_qmax(true) && (q <= 5 || b16_inline_k_wide() == 3);
      time_band16_group(bt, rec.fq16[g], q, rec.g16_n[g], in_wide, wide_seen);
      bt->timing.band_p_sum += rec.g16_n[g];
    }
    if (rec.fq[0]) {
      bool p2 = !rec.p64.empty();
      for (int pb : rec.p64) p2 = p2 && pb == 2;
      time_fused64_pair(bt, rec.fq, rec.p64, p2);
      for (int pb : rec.p64) bt->timing.band_p_sum += pb;
    }
    bt->timing.band_fallbacks += (double)redo.size();
  }
  const int rc = redo_dense(bt, redo, rec.theta.data(), lml, grad, info, bt->slow_s ? bt->slow_s : ctx->stream, status);
  return rc != GPX_OK ? rc : status;
}

// every slow part that has finished (block: all of them, waiting), oldest first
static int deliver_ready(gpx_batch* bt, double* lml, double* grad, int32_t* info, bool block) {
  gpx_ctx* ctx = bt->ctx;
  int status = GPX_OK;
  while (!bt->slow_out.empty()) {
    gpx_batch::SlowRec& rec = *bt->slow_out.front();
    if (block) {
      HIPX(ctx, hipEventSynchronize(rec.done));
    } else {
      const hipError_t e = hipEventQuery(rec.done);
      if (e == hipErrorNotReady) break;
      if (e != hipSuccess) return fail(ctx, GPX_HIP_ERROR, std::string("hipEventQuery: ") + hipGetErrorString(e));
    }
    std::unique_ptr<gpx_batch::SlowRec> done = std::move(bt->slow_out.front());
    bt->slow_out.erase(bt->slow_out.begin());
    const int rc = deliver_slow(bt, *done, lml, grad, info);
    done->clear_events();
    bt->slow_pool.push_back(std::move(done));
    if (rc != GPX_OK && rc != GPX_NOT_PD) return rc;
    if (rc == GPX_NOT_PD) status = GPX_NOT_PD;
  }
  if (status == GPX_NOT_PD) last_error_slot() = kNotPdMessage;
  return status;
}

// ---- submit ----
}  // extern "C"

namespace gpx {
// What a call's fused range runs now and what goes out as a deferred slow part: the slow classes
// (band16 wider than defer_q, then the 64-row sweeps) are the tail of the fused range; they go out
// as a slow part and the call completes without them. Not on the reduction route (bcr_q), and a
// call of slow problems only just runs.
DeferSplit split_deferred(int defer_q, int bcr_q, int head, int n_g16, const int* g16_q, const int* g16_n, int n16,
                          int n_fused1, int n_fused) {
  DeferSplit sp{0, n_g16, n16, n_fused1};
  if (defer_q < 0 || n_fused <= 0 || bcr_q != 0) return sp;
  int k = 0, nb16 = 0;
  while (k < n_g16 && g16_q[k] <= defer_q) nb16 += g16_n[k++];
  if (n_fused > nb16 && head + nb16 > 0) sp = DeferSplit{n_fused - nb16, k, nb16, 0};
  return sp;
}
}  // namespace gpx

namespace {
// the arguments of a slow part's submit_slow (kept for after the download in same-stream deferral)
struct SlowPart { int off = -1, n = 0, n_g16 = 0, g0 = 0, n16 = 0, n1 = 0; bool se1 = true; int max_terms = 1; };

// one submit call between its routing and its launches
struct SubmitCall {
  gpx_batch* bt;
  hipStream_t s;
  const double* theta;
  Route rt;
  int n_active = 0;  // the problems launched by this call (band storage: without the shadowed ones)
  // a call with few band16 problems takes them by block cyclic reduction (gpx_bcr.hip): the
  // one-wavefront sweeps' N/16-step chain would be the whole call's latency
  int bcr_q = 0;
  // (the width groups [0, g_bcr) of Q <= kBcrMaxQ, n16_bcr problems: the reduction; wider ones keep
  // their sweeps, so a problem's arithmetic depends on its own width and the call's size only;
  // the wide groups [g_wide, n_g16), Q > kBcrMaxQ, a suffix: the bs = 128 reduction)
  int g_bcr = 0, n16_bcr = 0, g_wide = 0;
  // band storage: a few fallback problems go out at once on the fallback stream (more than the
  // fallback slots hold run in chunks at _complete)
  bool shadow_async = false;
  DeferSplit split{};
  SlowPart later;  // same-stream deferral: the slow part that follows the call's download

  int head() const { return rt.n_dense + rt.n_band; }
  int kband16() const { return rt.b16_p2 ? 3 : 2; }
  int max_terms(int i0, int i1) const {
    int m = 1;
    for (int i = i0; i < i1; ++i) m = std::max(m, (int)bt->specs[rt.order[i]].n_terms);
    return m;
  }
  // the reference's kernel (one SquaredExponential term on one column) everywhere in the range: the
  // band16 backward sweep's straight-line contraction
  bool se1(int i0, int i1) const {
    bool y = true;
    for (int i = i0; i < i1; ++i) y = y && se1_spec(bt->specs[rt.order[i]]);
    return y;
  }
  // a failure after the fallback evaluation went out leaves nothing pending on the fallback
  // slots: drain its stream and drop its state, so later calls are not refused
  int drop_shadow(int rc) const {
    if (shadow_async && bt->shadow && bt->shadow->pending_eval) {
      (void)hipStreamSynchronize(bt->shadow->pending_eval->s);
      bt->shadow->pending_eval.reset();
    }
    return rc;
  }
};

std::unique_ptr<gpx_batch::PendingEval> new_pending(const SubmitCall& c, int n_active, bool total_on, bool ct_on,
                                                    bool bp_on) {
  std::unique_ptr<gpx_batch::PendingEval> pe(new gpx_batch::PendingEval());
  pe->s = c.s;
  pe->n_active = n_active;
  pe->theta.assign(c.theta, c.theta + (size_t)c.bt->B * GPX_THETA_STRIDE);
  pe->total.reset(new PhaseTimer(total_on, c.s));
  pe->ct.reset(new PhaseTimer(ct_on, c.s));
  pe->bp.reset(new PhaseTimer(bp_on, c.s));
  return pe;
}

// Route each problem (route_call: the dense recursion, the per-block banded launches, the band16
// sweeps by width, the 64-row fused sweeps, or the fallback slots of band storage)
void route_submit(SubmitCall& c, int n_active, const int32_t* active) {
  gpx_batch* bt = c.bt;
  Route& rt = c.rt;
  route_call(bt, n_active, active, c.theta, rt);
  // a call with few band16 problems takes them by block cyclic reduction (gpx_bcr.hip, Q <= 5):
  // there its p64 = 2 problems go back to the 64-row sweeps (a Q = 6..8 one-wave sweep is the
  // throughput choice, but its N/16-step chain is 2-3x the 64-row sweeps' latency)
  const int bcr_max = bcr_max_problems(bt->band_route);
  if (!wide_bcr_on(true) && rt.n16 > 0 && rt.n16 <= bcr_max && rt.n_g16 > 0 && rt.g16_q[rt.n_g16 - 1] > kBcrMaxQ)
    route_call(bt, n_active, active, c.theta, rt, kBcrMaxQ);
  c.bcr_q = (rt.n16 > 0 && rt.n16 <= bcr_max) ? 1 : 0;
  while (c.bcr_q > 0 && c.g_bcr < rt.n_g16 && rt.g16_q[c.g_bcr] <= kBcrMaxQ) c.n16_bcr += rt.g16_n[c.g_bcr++];
  c.g_wide = rt.n_g16;
  while (wide_bcr_on(c.bcr_q > 0) && c.g_wide > 0 && rt.g16_q[c.g_wide - 1] > kBcrMaxQ) --c.g_wide;
  c.n_active = rt.n_dense + rt.n_band + rt.n_fused;
  c.shadow_async = !rt.shadow_ids.empty() && (int)rt.shadow_ids.size() <= kShadowSlots;
}

// everything on the dense fallback (the rebinds landed before)
int submit_all_shadow(SubmitCall& c) {
  std::unique_ptr<gpx_batch::PendingEval> pe = new_pending(c, 0, false, false, false);
  pe->shadow_ids = std::move(c.rt.shadow_ids);
  pe->shadow_async = c.shadow_async;
  c.bt->pending_eval = std::move(pe);
  return GPX_OK;
}

// a small-problem call (Np = 64, every problem on the one fused kernel): its I/O straight through
// coherent pinned memory — no upload or download DMA, the kernel launch and the synchronise
// are the call's whole device round trip (the drop-in pattern's solo calls, VERDICT r05 item 6;
// GPX_SMALL_DIRECT=0: the DMA'd I/O block)
bool small_direct_call(const SubmitCall& c) {
  // (not for a batch with a mean function: its gradient kernel follows the fused launch, whose
  // polled flag would tell the host to read the results before that kernel has written its columns)
  // (nor with ARD or Coregion problems, n_ard counts both: they take the launch chain below)
  return knob_on(Knob::SmallDirect) && small64_on(c.bt) && c.rt.n_dense == c.n_active && !c.shadow_async &&
         c.rt.shadow_ids.empty() && c.bt->n_mean == 0 && c.rt.n_ard == 0;
}

int submit_small_direct(SubmitCall& c) {
  gpx_batch* bt = c.bt;
  gpx_ctx* ctx = bt->ctx;
  const int n_active = c.n_active;
  if (!bt->h_sio) HIPX(ctx, hipHostMalloc(&bt->h_sio, bt->io_bytes, hipHostMallocCoherent));
  {
    const int e = fence_io(bt, c.s);
    if (e != GPX_OK) return e;
  }
  std::memcpy(bt->h_sio, c.rt.order.data(), sizeof(int) * n_active);
  std::memset(bt->h_sio + bt->io_info_off, 0, sizeof(int) * bt->B);
  std::memcpy(bt->h_sio + bt->io_theta_off, c.theta, sizeof(double) * GPX_THETA_STRIDE * bt->B);
  std::unique_ptr<gpx_batch::PendingEval> pd = new_pending(c, n_active, ctx->profiling != 0, false, false);
  pd->n_dense = n_active;
  pd->direct = true;
  // completion by polling the workgroups' flags (GPX_SMALL_POLL, default on; not when profiling,
  // whose events complete reads): a launch + synchronise round trip costs ≈ 12 µs, a launch and
  // a polled flag ≈ 7 (tools/micro/launch_roundtrip.hip)
  if (knob_on(Knob::SmallPoll) && !ctx->profiling) {
    bt->direct_tag = bt->direct_tag >= (1 << 30) ? 1 : bt->direct_tag + 1;
    pd->poll_tag = bt->direct_tag;
  }
  pd->total->mark();
  small64_eval(Run{bt, reinterpret_cast<const int*>(bt->h_sio), n_active, c.s}, true, bt->h_sio, pd->poll_tag);
  pd->total->mark();
  HIPX(ctx, hipGetLastError());
  pd->order = std::move(c.rt.order);
  bt->pending_eval = std::move(pd);
  return GPX_OK;
}

// the dense problems: [0, n_dense) of the active list
int submit_dense(SubmitCall& c, gpx_batch::PendingEval& pe) {
  gpx_batch* bt = c.bt;
  gpx_ctx* ctx = bt->ctx;
  hipStream_t s = c.s;
  const int n_dense = c.rt.n_dense;
  if (n_dense == 0) return GPX_OK;
  // (the ARD and Coregion problems: the last n_ard, the Coregion ones the last n_cg of those)
  const int n_ard = c.rt.n_ard, n_iso = n_dense - n_ard, n_cg = c.rt.n_cg;
  if (small64_on(bt)) {
    // Np = 64: the whole evaluation of every dense problem in one launch
    if (n_iso > 0) small64_eval(Run{bt, bt->d_active, n_iso, s}, true);
    if (n_ard > 0) {
      // an ARD problem of these sizes: the launch chain (build, leaf, solves, contraction, reduce)
      // with the ARD build and epilogue — by its spec, whatever else the call holds
      Run ra{bt, bt->d_active + n_iso, n_ard, s};
      ra.n_ard = n_ard;
      ra.n_cg = n_cg;
      ra.ard_terms = c.max_terms(n_iso, n_dense - n_cg);
      factor(ra);
      alpha_solve(ra);
      contract(ra, 1);
      reduce(ra);
    }
    return GPX_OK;
  }
  // Split the dense problems into up to kGroups ranges, each running the whole pipeline on
  // its own stream: one group's latency-bound phases (64x64 leaves, small recursion levels)
  // overlap another group's large MFMA GEMMs.
  // Default: one pipeline whose recursion forks the top-level T products onto aux streams
  // (concurrency inside the DAG). GPX_GROUPS=g instead splits the problems into g pipelines.
  const int ng = pe.ng = std::min(knob_int(Knob::Groups), n_dense);
  if (ng > 1 && !bt->fork) {
    HIPX(ctx, hipEventCreateWithFlags(&bt->fork, hipEventDisableTiming));
    for (int g = 0; g < kGroups; ++g) {
      HIPX(ctx, hipStreamCreateWithFlags(&bt->workers[g], hipStreamNonBlocking));
      HIPX(ctx, hipEventCreateWithFlags(&bt->join[g], hipEventDisableTiming));
    }
  }
  int next_event = 0;
  Run runs[kGroups];
  int start = 0;
  for (int g = 0; g < ng; ++g) {
    const int cnt = n_dense / ng + (g < n_dense % ng ? 1 : 0);
    runs[g] = Run{bt, bt->d_active + start, cnt, ng == 1 ? s : bt->workers[g], ng == 1, &next_event};
    runs[g].n_ard = std::max(0, start + cnt - std::max(start, n_iso));
    runs[g].n_cg = std::max(0, start + cnt - std::max(start, n_dense - n_cg));
    start += cnt;
  }
  if (ng > 1) {
    HIPX(ctx, hipEventRecord(bt->fork, s));
    for (int g = 0; g < ng; ++g) HIPX(ctx, hipStreamWaitEvent(runs[g].s, bt->fork, 0));
  }
  std::vector<PhaseTimer>& pts = pe.pts;
  pts.reserve(ng);
  for (int g = 0; g < ng; ++g) pts.emplace_back(ctx->profiling != 0, runs[g].s);
  for (int g = 0; g < ng; ++g) {
    const Run& r = runs[g];
    pts[g].mark();
    factor(r);
    pts[g].mark();
    alpha_solve(r);
    pts[g].mark();
  }
  if (ng > 1) {
    for (int g = 0; g < ng; ++g) {
      HIPX(ctx, hipEventRecord(bt->join[g], runs[g].s));
      HIPX(ctx, hipStreamWaitEvent(s, bt->join[g], 0));
    }
  }
  // The contraction fills the chip by itself (Np²/2/128² tiles per problem): one launch over
  // every dense problem, alone on the stream.
  // the contraction kernel is timestamped at its actual start/end (hipExtLaunchKernel), so
  // its duration excludes any wait behind kernels of other streams (concurrent batches)
  if (ctx->profiling) {
    HIPX(ctx, hipEventCreate(&pe.kev[0]));
    HIPX(ctx, hipEventCreate(&pe.kev[1]));
  }
  // optional: run the contraction on a highest-priority stream so that, with several batches
  // evaluating concurrently, its workgroups are dispatched ahead of the other batches' kernels
  const bool prio = knob_on(Knob::ContractPriority);
  Run cr{bt, bt->d_active, n_dense, s};
  cr.n_ard = n_ard;
  cr.n_cg = n_cg;
  cr.ard_terms = c.max_terms(n_iso, n_dense - n_cg);
  if (prio) {
    if (!bt->hp) {
      int lo = 0, hi = 0;
      HIPX(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIPX(ctx, hipStreamCreateWithPriority(&bt->hp, hipStreamNonBlocking, hi));
    }
    HIPX(ctx, hipEventRecord(bt->ev[kEvents - 4], s));
    HIPX(ctx, hipStreamWaitEvent(bt->hp, bt->ev[kEvents - 4], 0));
    cr.s = bt->hp;
  }
  PhaseTimer& ct = *pe.ct;
  ct.mark();
  contract(cr, c.max_terms(0, n_iso), pe.kev[0], pe.kev[1]);
  ct.mark();
  reduce(cr);
  if (prio) {
    HIPX(ctx, hipEventRecord(bt->ev[kEvents - 3], bt->hp));
    HIPX(ctx, hipStreamWaitEvent(s, bt->ev[kEvents - 3], 0));
  }
  ct.mark();
  return GPX_OK;
}

// the per-block band class: [n_dense, n_dense + n_band) of the active list
void submit_band_blocks(const SubmitCall& c) {
  const Route& rt = c.rt;
  if (rt.n_band > 0)
    band_eval(Run{c.bt, c.bt->d_active + rt.n_dense, rt.n_band, c.s}, rt.pband, c.max_terms(rt.n_dense, c.head()));
}
}  // namespace

extern "C" {

static int submit_slow_part(const SubmitCall& c, const SlowPart& p) {
  const Route& rt = c.rt;
  return submit_slow(c.bt, c.s, rt.order.data() + p.off, p.off, p.n, p.n_g16, rt.g16_q + p.g0, rt.g16_n + p.g0, p.n16,
                     p.n1, p.se1, c.kband16(), p.max_terms, c.theta);
}

// the fused classes, [head, n_active) of the active list: the deferred split, the slow part (on
// its own stream now, or kept in c.later for after the call's download), then what runs now
static int submit_fused(SubmitCall& c, gpx_batch::PendingEval& pe) {
  gpx_batch* bt = c.bt;
  gpx_ctx* ctx = bt->ctx;
  const Route& rt = c.rt;
  const int head = c.head();
  const DeferSplit sp = c.split =
      split_deferred(bt->defer_q, c.bcr_q, head, rt.n_g16, rt.g16_q, rt.g16_n, rt.n16, rt.n_fused1, rt.n_fused);
  if (sp.n_slow > 0) {
    const int off = c.n_active - sp.n_slow;
    const SlowPart part{off, sp.n_slow, rt.n_g16 - sp.n_g16_run, sp.n_g16_run, rt.n16 - sp.n16_run, rt.n_fused1,
                        c.se1(off, off + (rt.n16 - sp.n16_run)), c.max_terms(off, c.n_active)};
    if (defer_own_stream()) {
      const int rcs = submit_slow_part(c, part);
      if (rcs != GPX_OK) return c.drop_shadow(rcs);
    } else {
      c.later = part;
    }
  }
  const int n_fused = rt.n_fused - sp.n_slow, n16 = sp.n16_run, n_g16 = sp.n_g16_run;
  if (n_fused == 0) return GPX_OK;
  const bool fused64 = n_fused > n16;  // the 64-row fused kernels run too
  if (ctx->profiling && fused64)
    for (int e = 0; e < 4; ++e) HIPX(ctx, hipEventCreate(&pe.fq[e]));
  pe.n_band16 = n16;
  // (timing: the swept groups g_bcr .. g_wide only; the reductions' chains have their own events)
  pe.n_g16 = std::min(n_g16, c.g_wide) - c.g_bcr;
  pe.n_bcr = c.n16_bcr;
  for (int g = 0; g < pe.n_g16; ++g) {
    pe.g16_q[g] = rt.g16_q[c.g_bcr + g];
    pe.g16_n[g] = rt.g16_n[c.g_bcr + g];
    if (ctx->profiling)
      for (int e = 0; e < 4; ++e) HIPX(ctx, hipEventCreate(&pe.fq16[g][e]));
  }
  Run rf{bt, bt->d_active + head, n_fused, c.s};
  rf.bcr_q = c.bcr_q;
  rf.bcr_wsp = &bt->bcr_ws;
  rf.bcr_capp = &bt->bcr_ws_cap;
  rf.ev16_g0 = c.g_bcr;
  const int ebf = band_fused_eval(rf, n16, n_g16, rt.g16_q, rt.g16_n, c.se1(head, head + n16), c.kband16(),
                                  sp.n_fused1_run, c.max_terms(head, head + n_fused),
                                  (ctx->profiling && fused64) ? pe.fq : nullptr, ctx->profiling ? pe.fq16 : nullptr);
  return ebf != GPX_OK ? c.drop_shadow(ebf) : GPX_OK;
}

int gpx_batch_lml_grad_submit(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                              void* stream) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if (bt->pending_eval) return fail(ctx, GPX_BAD_ARG, "an evaluation is already submitted on this batch");
  {  // every argument check before anything is routed or submitted (the fallback slots included)
    const int e = check_active_theta(bt, n_active, active, theta);
    if (e != GPX_OK) return e;
  }
  if (!bt->deferred.empty())
    for (int i = 0; i < n_active; ++i)
      if (bt->deferred[active[i]])
        return fail(ctx, GPX_BAD_ARG, "a problem of the call has a deferred evaluation in flight");
  HIPX(ctx, hipSetDevice(ctx->device));
  SubClock sc(bt);
  ++bt->sub_calls;
  if (submit_stats_on() && bt->sub_calls % 256 == 0) print_submit_stats(bt);  // (runs that never destroy it)

  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  trace_mark(bt, 38, s);
  {  // slots rebound since the last call land first: their band tables (from the gather's
     // X boxes) decide the routing below
    const int rc0 = flush_rebinds(bt, s);
    if (rc0 != GPX_OK) return rc0;
  }
  trace_mark(bt, 39, s);
  sc.lap(0);
  SubmitCall c{bt, s, theta};
  route_submit(c, n_active, active);
  const Route& rt = c.rt;
  if (c.shadow_async) {
    const int rcs = shadow_submit(bt, rt.shadow_ids, theta, s);
    if (rcs != GPX_OK) return c.drop_shadow(rcs);
  }
  if (c.n_active == 0) return submit_all_shadow(c);
  if (rt.n_band > 0) {
    const int e = ensure(ctx, bt->bres, bt->bres_cap, (size_t)bt->B * bt->Np);
    if (e != GPX_OK) return c.drop_shadow(e);
  }
  if (c.n16_bcr > 0 || c.g_wide < rt.n_g16) {  // (the workspace is sized by band_fused_eval for what it launches)
    if (ctx->profiling && !bt->bcr_ev[0])
      for (auto& e2 : bt->bcr_ev) HIPX(ctx, hipEventCreate(&e2));
  }
  sc.lap(1);
  if (small_direct_call(c)) {
    const int rc = submit_small_direct(c);
    if (rc == GPX_OK) sc.lap(4);
    return rc;
  }
  int rc = upload_common(bt, c.n_active, rt.order.data(), theta, s);
  if (rc != GPX_OK) return c.drop_shadow(rc);
  sc.lap(2);
  rc = match_aux_priority(bt, s);
  if (rc != GPX_OK) return c.drop_shadow(rc);
  bt->flops_acc = 0.0;
  std::unique_ptr<gpx_batch::PendingEval> pe =
      new_pending(c, c.n_active, ctx->profiling != 0, ctx->profiling != 0 && rt.n_dense > 0, ctx->profiling != 0);
  pe->total->mark();
  if (bt->n_mean > 0) {  // the residuals every route below reads as its targets (eval_y)
    rc = mean_residuals(bt, bt->d_active, c.n_active, s);
    if (rc != GPX_OK) return c.drop_shadow(rc);
  }
  rc = submit_dense(c, *pe);
  if (rc != GPX_OK) return rc;
  pe->bp->mark();
  submit_band_blocks(c);
  rc = submit_fused(c, *pe);
  if (rc != GPX_OK) return rc;
  // (every route's reduce has written its result rows, on s or joined to it; α is the route's)
  if (bt->n_mean > 0) mean_gradients(bt, bt->d_active, c.n_active, s);
  pe->bp->mark();
  pe->total->mark();
  HIPX(ctx, hipGetLastError());
  sc.lap(3);
  // one DMA into the pinned block: [info | theta (unchanged) | results]
  HIPX(ctx, hipMemcpyAsync(bt->h_io + bt->io_info_off, bt->d_io + bt->io_info_off,
                           bt->io_bytes - bt->io_info_off, hipMemcpyDeviceToHost, s));
  trace_mark(bt, 44, s);
  if (c.later.off >= 0) {
    // the call completes here; its slow part follows on the same stream
    if (!bt->bulk_ev) HIPX(ctx, hipEventCreateWithFlags(&bt->bulk_ev, hipEventDisableTiming));
    HIPX(ctx, hipEventRecord(bt->bulk_ev, s));
    pe->bulk_done = bt->bulk_ev;
    const int rcs = submit_slow_part(c, c.later);
    if (rcs != GPX_OK) return c.drop_shadow(rcs);
  }
  sc.lap(4);
  const int n_slow = c.split.n_slow;
  if (n_slow > 0) {  // the call's own problems: [dense | band | bulk band16]
    pe->deferred_ids.assign(c.rt.order.end() - n_slow, c.rt.order.end());
    c.rt.order.resize(c.rt.order.size() - n_slow);
    pe->n_active = c.n_active - n_slow;
  }
  pe->order = std::move(c.rt.order);
  pe->n_dense = rt.n_dense;
  pe->n_band = rt.n_band;
  pe->n_fused = rt.n_fused - n_slow;
  pe->n_fused1 = c.split.n_fused1_run;
  pe->shadow_ids = std::move(c.rt.shadow_ids);
  pe->shadow_async = c.shadow_async;
  bt->pending_eval = std::move(pe);
  return GPX_OK;
}

// ---- complete ----
// the submitted evaluation's results are in the pinned block
static int wait_pending(gpx_batch* bt, const gpx_batch::PendingEval& pe) {
  gpx_ctx* ctx = bt->ctx;
  hipStream_t s = pe.s;
  if (pe.poll_tag > 0) {
    // a small-problem call: wait for every workgroup's flag (each is written after its results, a
    // system-scope fence between); the stream is asked now and then, so a failed launch ends the
    // wait with its error instead of a spin
    const volatile int* flags = reinterpret_cast<const volatile int*>(bt->h_sio + bt->io_flag_off);
    for (int i = 0, spins = 0; i < pe.n_active;) {
      if (flags[i] == pe.poll_tag) {
        ++i;
        continue;
      }
      if (++spins % 4096 == 0) {
        const hipError_t q = hipStreamQuery(s);
        if (q != hipErrorNotReady && q != hipSuccess) HIPX(ctx, q);
        if (q == hipSuccess && flags[i] != pe.poll_tag) {  // (finished without its flag: not expected)
          HIPX(ctx, hipStreamSynchronize(s));
          break;
        }
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  } else if (pe.bulk_done) {  // (a slow part follows the call on its stream)
    HIPX(ctx, hipEventSynchronize(pe.bulk_done));
  } else {
    HIPX(ctx, hipStreamSynchronize(s));
  }
  if (pe.direct) {  // (the kernel wrote info and results into the coherent block)
    for (int i = 0; i < pe.n_active; ++i) {
      const int b = pe.order[i];
      bt->h_info[b] = reinterpret_cast<const int*>(bt->h_sio + bt->io_info_off)[b];
      std::memcpy(bt->h_results + (size_t)b * kResStride,
                  reinterpret_cast<const double*>(bt->h_sio + bt->io_res_off) + (size_t)b * kResStride,
                  sizeof(double) * kResStride);
    }
  }
  return GPX_OK;
}

// profiling: the completed call's phases into bt->timing
static void account_timing(gpx_batch* bt, gpx_batch::PendingEval& pe) {
  const int n_active = pe.n_active, n_dense = pe.n_dense, n_band = pe.n_band, n_fused = pe.n_fused;
  const int n_fused1 = pe.n_fused1, ng = pe.ng;
  const std::vector<int32_t>& order = pe.order;
  PhaseTimer& total = *pe.total;
  PhaseTimer& ct = *pe.ct;
  bt->timing.factor_ms = bt->timing.alpha_ms = 0.0;
  for (int g = 0; g < ng; ++g) {
    bt->timing.factor_ms += pe.pts[g].ms(0, 1) / ng;
    bt->timing.alpha_ms += pe.pts[g].ms(1, 2) / ng;
  }
  // (the small-problem kernel of Np = 64 batches has no separate contraction launch to time)
  bt->timing.grad_ms = (n_dense > 0 && ct.ev.size() >= 3) ? ct.ms(0, 2) : 0.0;
  if (n_dense > 0 && pe.kev[0]) {
    float kms = 0.f;
    (void)hipEventElapsedTime(&kms, pe.kev[0], pe.kev[1]);
    bt->timing.contract_ms_total += kms;
    bt->timing.contract_launches += 1.0;
    double f = 0.0;
    for (int i = 0; i < bt->Np; ++i) f += 2.0 * (i + 1) * (double)(bt->Np - i);
    bt->timing.contract_alg_flops += n_dense * f;
  }
  const int b16_0 = n_dense + n_band, b16_1 = b16_0 + pe.n_band16;  // the band16 class's range of the order
  if (n_band + n_fused > 0) {
    bt->timing.band_ms_total += pe.bp->ms(0, 1);
    bt->timing.band_calls += 1.0;
    bt->timing.band_evals += n_band + n_fused;
    for (int i = n_dense; i < n_active; ++i)
      bt->timing.band_p_sum += (i >= b16_0 && i < b16_1) ? 1 : bt->h_bandp[order[i]];
  }
  if (pe.n_bcr > 0 && bt->bcr_ev[0]) {
    float fb = 0.f;
    (void)hipEventElapsedTime(&fb, bt->bcr_ev[0], bt->bcr_ev[1]);
    bt->timing.bcr_ms_total += fb;
    bt->timing.bcr_calls += 1.0;
    bt->timing.bcr_evals += pe.n_bcr;
  }
  bool wide_seen = false;  // (a call's own groups never run in the wide launch: deferred parts only)
  for (int g = 0; g < pe.n_g16; ++g) time_band16_group(bt, pe.fq16[g], pe.g16_q[g], pe.g16_n[g], false, wide_seen);
  if (n_fused > pe.n_band16) {
    // the timed launch pair is the p <= 1 class's when there is one, else the p = 2 class's
    std::vector<int> p64;
    for (int i = b16_1; i < (n_fused1 > 0 ? b16_1 + n_fused1 : n_active); ++i) p64.push_back(bt->h_bandp[order[i]]);
    time_fused64_pair(bt, pe.fq, p64, n_fused1 == 0);
  }
  bt->timing.predict_ms = 0.0;
  bt->timing.total_ms = total.ms(0, 1);
  bt->timing.gemm_flops = bt->flops_acc;
  bt->timing.eval_ms_total += total.ms(0, 1);
  bt->timing.evals += n_active;
}

int gpx_batch_lml_grad_complete(gpx_batch* bt, double* lml, double* grad, int32_t* info) {
  if (!bt) return GPX_BAD_ARG;
  gpx_ctx* ctx = bt->ctx;
  if (!bt->pending_eval) return fail(ctx, GPX_BAD_ARG, "no evaluation submitted on this batch");
  std::unique_ptr<gpx_batch::PendingEval> pe = std::move(bt->pending_eval);
  if (!lml || !grad || !info) return fail(ctx, GPX_BAD_ARG, "null output");
  HIPX(ctx, hipSetDevice(ctx->device));
  SubClock sc(bt);
  {
    const int e = wait_pending(bt, *pe);
    if (e != GPX_OK) return e;
  }
  sc.lap(5);
  const bool timed = pe->total->on;
  if (timed) account_timing(bt, *pe);
  const double* theta = pe->theta.data();
  int status = GPX_OK;
  // banded evaluations whose check failed are redone on the dense path below; rows i < n_dense
  // are dense (no band check, the cached factor is the dense one)
  const double band_tol = knob_real(Knob::BandTol);
  std::vector<int32_t> redo;
  for (int i = 0; i < pe->n_active; ++i) {
    const int b = pe->order[i];
    if (!deliver_row(bt, b, bt->h_results + (size_t)b * kResStride, bt->h_info[b], i >= pe->n_dense, band_tol, theta,
                     lml, grad, info, status)) {
      info[b] = 0;  // (until the dense re-evaluation writes it)
      redo.push_back(b);
    }
  }
  for (int b : pe->deferred_ids) {  // (their results come with a later _complete / deferred_wait)
    info[b] = GPX_INFO_DEFERRED;
    lml[b] = NAN;
    for (int p = 0; p <= bt->specs[b].n_params; ++p) grad[(size_t)b * GPX_THETA_STRIDE + p] = NAN;
  }
  if (!bt->slow_out.empty()) {  // earlier calls' slow parts that have finished by now
    const int rcd = deliver_ready(bt, lml, grad, info, false);
    if (rcd != GPX_OK && rcd != GPX_NOT_PD) return rcd;
    if (rcd == GPX_NOT_PD) status = GPX_NOT_PD;
  }
  if (status == GPX_NOT_PD) last_error_slot() = kNotPdMessage;
  if (timed) bt->timing.band_fallbacks += (double)redo.size();
  // band storage: the problems routed dense run on the dense fallback slots too (collected here
  // when _submit sent them out, else evaluated with the redone rows)
  std::vector<int32_t> ids;
  if (pe->shadow_async) {
    const int rc1 = shadow_collect(bt, pe->shadow_ids, lml, grad, info);
    if (rc1 != GPX_OK && rc1 != GPX_NOT_PD) return rc1;
    if (rc1 == GPX_NOT_PD) status = GPX_NOT_PD;
  } else {
    ids = pe->shadow_ids;
  }
  ids.insert(ids.end(), redo.begin(), redo.end());
  const int rc2 = redo_dense(bt, ids, theta, lml, grad, info, pe->s, status);
  return rc2 != GPX_OK ? rc2 : status;
}


int gpx_batch_lml_grad_query(gpx_batch* bt) {
  if (!bt) return GPX_BAD_ARG;
  if (!bt->pending_eval) return 1;
  hipError_t e = bt->pending_eval->bulk_done ? hipEventQuery(bt->pending_eval->bulk_done)
                                              : hipStreamQuery(bt->pending_eval->s);
  if (e == hipSuccess && bt->pending_eval->shadow_async) e = hipStreamQuery(bt->shadow_s);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return fail(bt->ctx, GPX_HIP_ERROR, std::string("hipStreamQuery: ") + hipGetErrorString(e));
}
int gpx_batch_lml_grad(gpx_batch* bt, int n_active, const int32_t* active, const double* theta,
                       double* lml, double* grad, int32_t* info, void* stream) {
  if (!bt) return GPX_BAD_ARG;
  if (!lml || !grad || !info) return fail(bt->ctx, GPX_BAD_ARG, "null output");
  const int rc = gpx_batch_lml_grad_submit(bt, n_active, active, theta, stream);
  if (rc != GPX_OK) return rc;
  return gpx_batch_lml_grad_complete(bt, lml, grad, info);
}
int gpx_batch_deferred_wait(gpx_batch* bt, double* lml, double* grad, int32_t* info) {
  if (!bt) return GPX_BAD_ARG;
  if (!lml || !grad || !info) return fail(bt->ctx, GPX_BAD_ARG, "null output");
  // a delivered row whose band check failed is re-evaluated densely through this batch (or its
  // fallback slots), which an evaluation still submitted on it would refuse: refuse before any
  // slow part is taken off the queue, so nothing is lost
  if (bt->pending_eval)
    return fail(bt->ctx, GPX_BAD_ARG, "an evaluation is submitted on this batch: complete it before deferred_wait");
  HIPX(bt->ctx, hipSetDevice(bt->ctx->device));
  return deliver_ready(bt, lml, grad, info, true);
}

int gpx_batch_deferred_rows(const gpx_batch* bt, int32_t* rows, int cap) {
  if (!bt) return 0;
  int n = 0;
  for (const auto& r : bt->slow_out)
    for (int b : r->ids) {
      if (rows && n < cap) rows[n] = b;
      ++n;
    }
  return n;
}

}  // extern "C"
