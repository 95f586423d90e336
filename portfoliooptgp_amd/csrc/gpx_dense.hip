// gpx_dense.hip — the dense evaluation's host side: the batched GEMM launcher's wrapper, the
// recursive Cholesky-and-inverse, the solve, the gradient contraction and its reduction, and
// the one-launch small-problem evaluation (kernels: gpx_kernels.hip). See gpx_api.hip's head
// for the algorithm.
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

namespace gpx {

// MFMA flops the GEMM launcher will issue for these args (bench / roofline bookkeeping)
double gemm_issued_flops(const GemmArgs& a, int na) {
  const int bm = gemm_tile(a, na);
  const int ti = a.M / bm, tj = a.N / bm;
  double f = 0.0;
  for (int x = 0; x < ti; ++x)
    for (int y = 0; y < tj; ++y) {
      if (a.lower_only && y > x) continue;
      const int i0 = x * bm, j0 = y * bm;
      int kmin = 0, kmax = a.K;
      if (a.tri & TRI_KMAX_I) kmax = std::min(kmax, i0 + bm);
      if (a.tri & TRI_KMAX_J) kmax = std::min(kmax, j0 + bm);
      if (a.tri & TRI_KMIN_J) kmin = std::max(kmin, j0);
      if (a.tri & TRI_KMIN_I) kmin = std::max(kmin, i0);
      if (kmax > kmin) f += 2.0 * bm * bm * (kmax - kmin);
    }
  return f * na;
}

void gemm(const Run& r, GemmArgs a, int epi, bool ta, bool tb) {
  a.active = r.d_act;
  // store GEMMs (the recursion's panels, trailing updates and inverses) pick 128-tiles only when
  // the launch still has a workgroup per CU (64-tiles otherwise: 4x the workgroups for the
  // recursion's lower levels in calls of few problems). An entry's sum runs over the same k in
  // the same 4-wide MFMA chunks either way — a wider tile's k-range only adds products with the
  // triangular operand's exact zeros, each ±0 onto a sum that is +0 until its first nonzero —
  // so a problem's arithmetic still does not depend on its call (tests/test_gpu_parity.py).
  // The contraction's per-tile partials do depend on the tile: it keeps the shape-only rule.
  a.small_tiles = r.bt->small_tiles || epi == EPI_STORE;
  launch_gemm(a, epi, ta, tb, r.na, r.s);
  if (r.bt->ctx->profiling) r.bt->flops_acc += gemm_issued_flops(a, r.na);
}

GemmArgs gemm_args(const double* A, int lda, const double* B, int ldb, double* C, int ldc,
                   long long stride, int M, int N, int K, int tri, int lower, double alpha,
                   double beta) {
  GemmArgs g{};
  // longest-K tiles first, with the K-determining tile index as the slow one
  g.order = (tri & TRI_KMAX_J) ? ORDER_COL_DESC : (tri & TRI_KMIN_J) ? ORDER_COL_ASC
          : (tri & TRI_KMAX_I) ? ORDER_ROW_DESC : ORDER_ROW_ASC;
  g.A = A; g.sA = stride; g.lda = lda;
  g.Bm = B; g.sB = stride; g.ldb = ldb;
  g.C = C; g.sC = stride; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.tri = tri; g.lower_only = lower;
  g.alpha = alpha; g.beta = beta;
  return g;
}

// Recursive Cholesky-and-inverse on the diagonal block [off, off+n) of every problem of r.
void chol_inv(const Run& r, int off, int n, int depth) {
  gpx_batch* bt = r.bt;
  const int Np = bt->Np;
  const long long st = mat_stride(bt);
  // GPX_LEAF128=0 recurses down to 64-leaves instead (A/B measurements)
  static const bool leaf128 = knob_on(Knob::Leaf128);
  if (n == kLeaf || (leaf128 && n == 2 * kLeaf)) {
    LeafArgs la{};
    la.active = r.d_act; la.K = bt->K; la.W = bt->W; la.sMat = st; la.ld = Np; la.off = off;
    la.ldiag = bt->ldiag; la.sVec = Np; la.info = bt->d_info;
    // a 128-node is factored and inverted by one fused kernel (no 64x64 GEMM launches)
    if (n == kLeaf) launch_leaf(la, r.na, r.s);
    else launch_leaf128(la, r.na, r.s);
    return;
  }
  int n1 = ((n / 2 + kLeaf - 1) / kLeaf) * kLeaf;
  if (n1 >= n) n1 = n - kLeaf;
  const int n2 = n - n1;
  chol_inv(r, off, n1, depth + 1);
  const long long o11 = (long long)off * Np + off;
  const long long o21 = (long long)(off + n1) * Np + off;
  const long long o22 = (long long)(off + n1) * Np + off + n1;
  // L21 = A21 · W11ᵀ          (opB(k,j) = W11[j][k], nonzero for k <= j)
  gemm(r, gemm_args(bt->K + o21, Np, bt->W + o11, Np, bt->L + o21, Np, st, n2, n1, n1,
                    TRI_KMAX_J, 0, 1.0, 0.0), EPI_STORE, false, true);
  // T = L21 · W11 → the dead A21 region of K   (opB(k,j) = W11[k][j], nonzero for k >= j).
  // T depends only on L21 and W11, so at the top depths it runs on an auxiliary stream
  // concurrently with the (latency-bound) recursion on A22 below.
  const GemmArgs targs = gemm_args(bt->L + o21, Np, bt->W + o11, Np, bt->K + o21, Np, st, n2, n1,
                                   n1, TRI_KMIN_J, 0, 1.0, 0.0);
  const bool fork = r.dag && depth < kAux && r.next_event && *r.next_event + 2 <= kEvents;
  hipEvent_t eT = nullptr;
  if (fork) {
    hipEvent_t eL = bt->ev[(*r.next_event)++];
    eT = bt->ev[(*r.next_event)++];
    Run ra = r;
    ra.s = bt->aux[depth];
    (void)hipEventRecord(eL, r.s);
    (void)hipStreamWaitEvent(ra.s, eL, 0);
    gemm(ra, targs, EPI_STORE, false, false);
    (void)hipEventRecord(eT, ra.s);
  } else {
    gemm(r, targs, EPI_STORE, false, false);
  }
  // A22 -= L21 · L21ᵀ         (lower tiles only)
  gemm(r, gemm_args(bt->L + o21, Np, bt->L + o21, Np, bt->K + o22, Np, st, n2, n2, n1, 0, 1,
                    -1.0, 1.0), EPI_STORE, false, true);
  chol_inv(r, off + n1, n2, depth + 1);
  if (fork) (void)hipStreamWaitEvent(r.s, eT, 0);
  // W21 = −W22 · T             (opA(i,k) = W22[i][k], nonzero for k <= i)
  gemm(r, gemm_args(bt->W + o22, Np, bt->K + o21, Np, bt->W + o21, Np, st, n2, n1, n2,
                    TRI_KMAX_I, 0, -1.0, 0.0), EPI_STORE, false, false);
}

// K build + recursive factor for the problems of r.
void factor(const Run& r) {
  gpx_batch* bt = r.bt;
  BuildArgs ba{};
  ba.active = r.d_act; ba.specs = bt->d_specs; ba.theta = bt->d_theta; ba.nvalid = bt->d_n;
  ba.X = bt->X; ba.sX = (long long)bt->Nmax * bt->D; ba.X2 = bt->X; ba.sX2 = ba.sX; ba.D = bt->D;
  ba.m2 = 0; ba.out = bt->K; ba.sOut = mat_stride(bt); ba.ldo = bt->Np; ba.rows = ba.cols = bt->Np;
  ba.symmetric = 1;
  build_range(ba, r.na, r.n_ard, r.n_cg, r.s);
  chol_inv(r, 0, bt->Np);
}

// the isotropic problems of a range by build_kernel, its trailing ARD ones by build_ard_kernel, the
// Coregion ones behind those by build_coreg_kernel
void build_range(const BuildArgs& a, int na, int n_ard, int n_cg, hipStream_t s) {
  if (na > n_ard) launch_build(a, na - n_ard, s);
  if (n_ard > n_cg) {
    BuildArgs b = a;
    b.active = a.active + (na - n_ard);
    launch_build_ard(b, n_ard - n_cg, s);
  }
  if (n_cg > 0) {
    BuildArgs b = a;
    b.active = a.active + (na - n_cg);
    launch_build_coreg(b, n_cg, s);
  }
}

// z = W y, α = Wᵀ z
void alpha_solve(const Run& r) {
  gpx_batch* bt = r.bt;
  const long long st = mat_stride(bt);
  TrmvArgs t{};
  t.active = r.d_act; t.Wm = bt->W; t.sW = st; t.ld = bt->Np;
  t.x = eval_y(bt); t.sx = bt->Nmax; t.nvalid = bt->d_n; t.y = bt->z; t.sy = bt->Np;
  t.rows = t.cols = bt->Np; t.lower = 1;
  launch_trmv_n(t, r.na, r.s);
  TrmvArgs u{};
  u.active = r.d_act; u.Wm = bt->W; u.sW = st; u.ld = bt->Np;
  u.x = bt->z; u.sx = bt->Np; u.nvalid = nullptr; u.y = bt->alpha; u.sy = bt->Np;
  u.rows = u.cols = bt->Np; u.lower = 1;
  launch_trmv_t(u, r.na, r.s);
}

// fused K⁻¹ = WᵀW formation + gradient contraction over lower tiles, then the reduction
// (max_terms: over the range's isotropic problems; its ARD ones: r.ard_terms — so an isotropic
// problem's instance does not depend on the ARD specs that share its call)
void contract(const Run& r, int max_terms, hipEvent_t ev0, hipEvent_t ev1) {
  gpx_batch* bt = r.bt;
  GemmArgs g = gemm_args(bt->W, bt->Np, bt->W, bt->Np, nullptr, 0, mat_stride(bt), bt->Np, bt->Np,
                         bt->Np, TRI_KMIN_I, 1, 1.0, 0.0);
  g.vec = bt->alpha; g.sVec = bt->Np; g.X = bt->X; g.sX = (long long)bt->Nmax * bt->D; g.D = bt->D;
  g.specs = bt->d_specs; g.theta = bt->d_theta; g.nvalid = bt->d_n;
  g.partial = bt->partial; g.sPartial = bt->partial_stride;
  g.ev_start = ev0; g.ev_stop = ev1;
  const int n_iso = r.na - r.n_ard;
  if (n_iso > 0) {
    Run ri = r;
    ri.na = n_iso;
    gemm(ri, g, max_terms <= 1 ? EPI_CONTRACT1 : max_terms == 2 ? EPI_CONTRACT2 : EPI_CONTRACT, true, false);
    g.ev_start = g.ev_stop = nullptr;  // (a mixed call's contraction time: its isotropic launch)
  }
  if (r.n_ard > r.n_cg) {
    // the ARD problems (behind the isotropic ones): the θ-indexed epilogue, sized by their own specs
    Run ra = r;
    ra.d_act = r.d_act + n_iso;
    ra.na = r.n_ard - r.n_cg;
    gemm(ra, g, r.ard_terms <= 2 ? EPI_CONTRACT_ARD2 : EPI_CONTRACT_ARD, true, false);
    g.ev_start = g.ev_stop = nullptr;
  }
  if (r.n_cg > 0) {
    // the Coregion problems (the range's last n_cg): their own epilogue, one instance per tile size
    Run rc = r;
    rc.d_act = r.d_act + (r.na - r.n_cg);
    rc.na = r.n_cg;
    gemm(rc, g, EPI_CONTRACT_COREG, true, false);
  }
}

void reduce(const Run& r) {
  gpx_batch* bt = r.bt;
  GemmArgs g{};
  g.M = g.N = bt->Np; g.lower_only = 1; g.small_tiles = bt->small_tiles;  // as gemm() launches it
  const int bm = gemm_tile(g, r.na), tt = bt->Np / bm;
  ReduceArgs ra{};
  ra.active = r.d_act; ra.partial = bt->partial; ra.sPartial = bt->partial_stride;
  ra.ntiles = tt * (tt + 1) / 2; ra.z = bt->z; ra.sVec = bt->Np; ra.ldiag = bt->ldiag;
  ra.nvalid = bt->d_n; ra.specs = bt->d_specs; ra.results = bt->results; ra.Np = bt->Np;
  launch_reduce(ra, r.na, r.s);
}


// Np = 64 and Np = 128 batches: every dense evaluation is one fused launch (small64_kernel,
// small128_kernel; GPX_SMALL64=0 / GPX_SMALL128=0: the six-launch chain, for A/B). Which path runs
// depends on Np only, never on the call.
bool small64_on(const gpx_batch* bt) {
  static const bool on64 = knob_on(Knob::Small64), on128 = knob_on(Knob::Small128);
  return (on64 && bt->Np == kLeaf) || (on128 && bt->Np == 2 * kLeaf);
}

// the fused small-problem evaluation (grad: the gradient and logML too) for the problems of r;
// sio: the call's I/O block in coherent pinned memory (active list, θ, info, results read and
// written there by the kernel), else the device I/O block
void small64_eval(const Run& r, bool grad, char* sio, int tag) {
  gpx_batch* bt = r.bt;
  Small64Args a{};
  a.active = r.d_act; a.specs = bt->d_specs; a.theta = bt->d_theta; a.nvalid = bt->d_n;
  a.X = bt->X; a.sX = (long long)bt->Nmax * bt->D; a.D = bt->D; a.Y = eval_y(bt); a.sY = bt->Nmax;
  a.W = bt->W; a.sMat = mat_stride(bt); a.ld = bt->Np;
  a.z = bt->z; a.alpha = bt->alpha; a.ldiag = bt->ldiag; a.sVec = bt->Np;
  a.info = bt->d_info; a.results = bt->results; a.grad = grad ? 1 : 0;
  if (sio) {
    a.active = reinterpret_cast<const int*>(sio);
    a.info = reinterpret_cast<int*>(sio + bt->io_info_off);
    a.theta = reinterpret_cast<const double*>(sio + bt->io_theta_off);
    a.results = reinterpret_cast<double*>(sio + bt->io_res_off);
    if (tag > 0) {
      a.done = reinterpret_cast<int*>(sio + bt->io_flag_off);
      a.tag = tag;
    }
  }
  int max_terms = 1;
  for (int b = 0; b < bt->B; ++b) max_terms = std::max(max_terms, (int)bt->specs[b].n_terms);
  if (bt->Np == kLeaf)
    launch_small64(a, max_terms, r.na, r.s);
  else
    launch_small128(a, max_terms, r.na, r.s);
}

}  // namespace gpx
