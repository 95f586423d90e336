// gpx_route.hip — which path a problem takes at θ: the band tables, the band widths read from
// them, the per-call limits and the routing of one evaluation call. Pure host logic
// (tests/c/host_harness.cpp runs it under ASan/UBSan).
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

// ---------------------------------------------------------------------------------------
// Block-banded path (kernels in gpx_band.hip)
// ---------------------------------------------------------------------------------------
// Exactness: for the monotone stationary kernels (SE, Matern12/32/52, Exponential) every value
// and θ-derivative carries the factor exp(−a(s)), s = r/ℓ, with a(s) = s²/2, s, s/2, √3 s or
// √5 s. When a(s) ≥ 746 that factor is exactly 0 in fp64 (exp underflows below 2^-1075 at
// 745.13) and so is the whole entry (0 times a finite polynomial). band_rmin bounds r from
// below for every pair of points in blocks (k, k − d) (bounding boxes of the blocks' valid
// rows, per term's active dims); the margin 746 − 745.13 covers the rounding of r²/ℓ² on the
// device many times over. The device forms r² as GPflow does, (−2a·b) + (‖a‖² + ‖b‖²) with
// a = x/ℓ, which can fall short of the true (Δx/ℓ)² by cancellation, by at most a few
// eps·(‖a‖² + ‖b‖² + ‖a−b‖·max‖a‖): band_width shaves 64 eps·(M² + sM + 1) off s² (M = the
// largest ‖x/ℓ‖ of the problem's valid rows, kept in slot 0 of each term's table).
// A sum vanishes when all its terms do, a product when any does.
namespace {
bool band_kind(int kind) { return kind >= GPX_SE && kind <= GPX_EXPONENTIAL; }

double band_arg(int kind, double s) {
  switch (kind) {
    case GPX_SE: return 0.5 * s * s;
    case GPX_MATERN12: return s;
    case GPX_EXPONENTIAL: return 0.5 * s;
    case GPX_MATERN32: return 1.7320508075688772 * s;
    default: return 2.23606797749979 * s;  // GPX_MATERN52
  }
}
}  // namespace

// band_rmin of problem b at block size bs (64: band_rmin, 16: band_rmin16) from the per-block
// boxes lo/hi [nvb][D] of its valid rows (blocks of bs rows)
// The widest band offset (in blocks of bs rows) any routing decision distinguishes: the 64-row
// paths take p <= band_limit <= Np/256, the band16 path Q <= kBand16MaxQ; a table entry beyond
// it only has to say "still nonzero" correctly, which a lower bound does.
static int band_table_cap(const gpx_batch* bt, int bs) {
  if (bs != kLeaf) return kBand16MaxQ + 1;
  // (GPX_BAND_PMAX: band_limit's override, when it raises the limit)
  return std::max(bt->Np / kLeaf / 4, knob_int(Knob::BandPmax)) + 1;
}

static void band_tables_lohi(gpx_batch* bt, int b, int bs, const std::vector<double>& lo,
                             const std::vector<double>& hi) {
  const int nb = bt->Np / bs, D = bt->D, n = bt->n[b];
  std::vector<double>& tabv = bs == kLeaf ? bt->band_rmin : bt->band_rmin16;
  double* out = tabv.data() + (size_t)b * GPX_MAX_TERMS * nb;
  std::fill(out, out + (size_t)GPX_MAX_TERMS * nb, INFINITY);
  int* tail = (bs == kLeaf ? bt->band_tail : bt->band_tail16).data() + (size_t)b * GPX_MAX_TERMS;
  std::fill(tail, tail + GPX_MAX_TERMS, nb);
  const gpx_kernel_spec& sp = bt->specs[b];
  const int nvb = (n + bs - 1) / bs;  // blocks holding valid rows
  const int cap = band_table_cap(bt, bs);
  for (int t = 0; t < sp.n_terms; ++t) {
    const int d0 = sp.terms[t].dim_start, dn = sp.terms[t].dim_count;
    double* rt = out + (size_t)t * nb;
    // one active dimension with the blocks' boxes in increasing order (day offsets): the gap
    // between blocks k and k − dd is lo[k] − hi[k − dd], nondecreasing in dd for every k, so
    // rmin is nondecreasing and rmin[cap] bounds every later entry from below
    bool sorted = dn == 1;
    for (int k = 1; sorted && k < nvb; ++k) sorted = hi[(size_t)(k - 1) * D + d0] <= lo[(size_t)k * D + d0];
    const int ddmax = sorted ? std::min(nvb - 1, cap) : nvb - 1;
    double m2 = 0.0;  // max ‖x‖² over the valid rows (active dims), bounded by the boxes
    for (int k = 0; k < nvb; ++k) {
      double s2 = 0.0;
      for (int d = d0; d < d0 + dn; ++d) {
        const double mx = std::max(std::fabs(lo[(size_t)k * D + d]), std::fabs(hi[(size_t)k * D + d]));
        s2 += mx * mx;
      }
      m2 = std::max(m2, s2);
    }
    rt[0] = std::sqrt(m2) * (1.0 + 1e-12);
    for (int dd = 1; dd <= ddmax; ++dd) {
      double m = INFINITY;
      for (int k = dd; k < nvb; ++k) {
        double g2 = 0.0;
        for (int d = d0; d < d0 + dn; ++d) {
          const double g = std::max(0.0, std::max(lo[(size_t)k * D + d] - hi[(size_t)(k - dd) * D + d],
                                                  lo[(size_t)(k - dd) * D + d] - hi[(size_t)k * D + d]));
          g2 += g * g;
        }
        m = std::min(m, g2);
      }
      // the box gap is exact in real arithmetic; shave a relative 1e-12 off for the rounding
      // of the sums above
      rt[dd] = std::sqrt(m) * (1.0 - 1e-12);
    }
    if (ddmax < nvb - 1) {
      for (int dd = ddmax + 1; dd < nvb; ++dd) rt[dd] = rt[ddmax];
      tail[t] = ddmax;
    }
  }
}

// both tables from the 16-row boxes box[nvb16][D][2] of problem b (the 64-row boxes are their
// unions); band_rmin16 is kept only where the 16-row path can run (Np <= kBand16MaxNp)
void band_tables_boxes(gpx_batch* bt, int b, const double* box) {
  const int D = bt->D, n = bt->n[b];
  const int nv16 = (n + kBox - 1) / kBox, nv64 = (n + kLeaf - 1) / kLeaf;
  std::vector<double> lo((size_t)nv64 * D, INFINITY), hi((size_t)nv64 * D, -INFINITY);
  for (int k = 0; k < nv16; ++k)
    for (int d = 0; d < D; ++d) {
      const size_t e = (size_t)k * D + d, f = (size_t)(k / (kLeaf / kBox)) * D + d;
      lo[f] = std::min(lo[f], box[2 * e]);
      hi[f] = std::max(hi[f], box[2 * e + 1]);
    }
  band_tables_lohi(bt, b, kLeaf, lo, hi);
  if (!bt->band_rmin16.empty()) {
    std::vector<double> lo16((size_t)nv16 * D), hi16((size_t)nv16 * D);
    for (size_t e = 0; e < (size_t)nv16 * D; ++e) {
      lo16[e] = box[2 * e];
      hi16[e] = box[2 * e + 1];
    }
    band_tables_lohi(bt, b, kBox, lo16, hi16);
  }
}

void band_tables(gpx_batch* bt, int b, const double* hostX) {
  const int D = bt->D, n = bt->n[b];
  const int nvb = (n + kBox - 1) / kBox;
  std::vector<double> box((size_t)nvb * D * 2);
  for (int k = 0; k < nvb; ++k)
    for (int d = 0; d < D; ++d) {
      double a = INFINITY, z = -INFINITY;
      for (int r = k * kBox; r < std::min(n, (k + 1) * kBox); ++r) {
        a = std::min(a, hostX[(size_t)r * D + d]);
        z = std::max(z, hostX[(size_t)r * D + d]);
      }
      box[2 * ((size_t)k * D + d)] = a;
      box[2 * ((size_t)k * D + d) + 1] = z;
    }
  band_tables_boxes(bt, b, box.data());
}

static int band_width_bs(const gpx_batch* bt, int b, const double* th, int bs) {
  const gpx_kernel_spec& sp = bt->specs[b];
  for (int t = 0; t < sp.n_terms; ++t)
    if (!band_kind(sp.terms[t].kind)) return -1;
  const int nb = bt->Np / bs;
  const double* tab = (bs == kLeaf ? bt->band_rmin : bt->band_rmin16).data() + (size_t)b * GPX_MAX_TERMS * nb;
  const int* tail = (bs == kLeaf ? bt->band_tail : bt->band_tail16).data() + (size_t)b * GPX_MAX_TERMS;
  const bool prod = sp.n_terms > 1 && sp.combine == GPX_PRODUCT;
  auto nz_at = [&](int d) {
    bool nz = prod;
    for (int t = 0; t < sp.n_terms; ++t) {
      const double ell = th[sp.terms[t].param_offset];
      const double r = tab[(size_t)t * nb + d];
      bool term_nz = false;
      if (r != INFINITY) {
        const double sv = r / ell, M = tab[(size_t)t * nb] / ell;
        const double s2 = sv * sv - 64.0 * DBL_EPSILON * (M * M + sv * M + 1.0);
        term_nz = !(band_arg(sp.terms[t].kind, s2 > 0.0 ? std::sqrt(s2) : 0.0) >= 746.0);
      }
      nz = prod ? (nz && term_nz) : (nz || term_nz);
    }
    return nz;
  };
  // beyond the largest tail offset every term's entry repeats, so the scan from the top gives the
  // same answer as testing that offset once
  int top = nb - 1, tmax = 0;
  for (int t = 0; t < sp.n_terms; ++t) tmax = std::max(tmax, tail[t]);
  if (tmax >= 1 && tmax < nb - 1) {
    if (nz_at(tmax)) return nb - 1;
    top = tmax - 1;
  }
  for (int d = top; d >= 1; --d)
    if (nz_at(d)) return d;
  return 0;
}

int band_width(const gpx_batch* bt, int b, const double* th) { return band_width_bs(bt, b, th, kLeaf); }

// the band width in 16-row blocks (band16 kernels), or -1 when the tables are not kept
int band_width16(const gpx_batch* bt, int b, const double* th) {
  if (bt->band_rmin16.empty()) return -1;
  return band_width_bs(bt, b, th, kBox);
}

// the 16-row path (gpx_band16.hip) takes p64 <= 1 problems whose band is at most this many
// 16-blocks (GPX_BAND16=0 disables it)
int band16_limit(const gpx_batch* bt) {
  if (!knob_on(Knob::Band16)) return -1;
  if (bt->band_rmin16.empty() || bt->D > kBand16MaxD) return -1;
  return kBand16MaxQ;
}

// shapes the banded path handles: ≥ 8 blocks (smaller problems are a few leaves densely) and
// z in LDS for the solve. Band tables are kept for every such batch, whatever GPX_BAND says.
bool band_shape(const gpx_batch* bt) { return bt->Np / kLeaf >= 8 && bt->Np <= 8192; }

int band_limit(const gpx_batch* bt) {
  // read per call (cheap), so a process can compare the paths on the same problems
  const bool on = knob_on(Knob::Band);
  const int pmax_env = knob_int(Knob::BandPmax);
  if (!on || bt->force_dense || !band_shape(bt)) return -1;
  return pmax_env >= 0 ? pmax_env : bt->Np / kLeaf / 4;
}

// Routing of one evaluation call: the block-banded path when K and every ∂K/∂θ vanish exactly
// beyond a band of p <= band_limit 64-blocks at this θ (gpx_band.hip), the dense recursion
// otherwise. p <= 2 problems whose band is at most band16_limit 16-blocks take the band16
// sweeps (grouped by width Q), other p <= 2 problems the 64-row fused sweeps; band storage runs
// everything else on its dense fallback slots. Pure host logic over the band tables (writes
// h_bandp; tests/c/host_harness.cpp runs it under ASan/UBSan).
RouteLimits route_limits(const gpx_batch* bt) {
  RouteLimits L;
  L.plim = band_limit(bt);
  if (bt->compact) L.plim = std::min(L.plim, kBandStoreP);
  L.fused_on = knob_on(Knob::BandFused);  // 0: p <= 2 problems take the per-block launches too
  L.q16lim = L.fused_on ? band16_limit(bt) : -1;
  // the widest SE1 band16 class (GPX_BAND16_QMAX, default kBand16MaxQ): only with both sweeps
  // computing K's tiles inline
  L.q16wide = b16_inline_k() == 3 ? knob_int(Knob::Band16Qmax) : kBand16MaxQAny;
  return L;
}

// one problem's path at θ (route_call and gpx_batch_band_class)
RouteKind route_one(const gpx_batch* bt, int b, const double* thb, const RouteLimits& L, int& w) {
  const int p = L.plim >= 0 ? band_width(bt, b, thb) : -1;
  w = p;
  if (p >= 0 && p <= L.plim) {
    // p <= 2 problems whose band is at most kBand16MaxQ 16-blocks: the band16 sweeps
    int q16 = (p <= 2 && L.q16lim > 0) ? band_width16(bt, b, thb) : -1;
    // Q = 6..8 (a one-wave sweep whose window fills the register file): SE1 problems whose K
    // tiles both sweeps compute inline (their LDS holds no K tiles), up to GPX_BAND16_QMAX
    if (q16 > kBand16MaxQAny && !(q16 <= L.q16wide && se1_spec(bt->specs[b]))) q16 = -1;
    if (q16 >= 0 && q16 <= L.q16lim) {
      w = std::max(q16, 1);
      return kRouteBand16;
    }
    // (the p = 2 sweep holds four 64x64 LDS blocks plus three 64·D X-row slots: <= 160 KiB)
    if (L.fused_on && (p <= 1 || (p == 2 && bt->D <= 12))) return kRouteFused;
    return bt->compact ? kRouteShadow : kRouteBand;  // band storage runs the fused sweeps only
  }
  return bt->compact ? kRouteShadow : kRouteDense;   // (band storage: dense on the fallback slots)
}

void route_call(gpx_batch* bt, int n_active, const int32_t* active, const double* theta, Route& rt,
                int q16wide_cap) {
  std::vector<int32_t>& order = rt.order;
  order.clear();
  order.reserve(n_active);
  rt.shadow_ids.clear();
  std::vector<int32_t> band_ids, fused_ids;
  int pband = 0;
  RouteLimits L = route_limits(bt);
  L.q16wide = std::min(L.q16wide, q16wide_cap);
  std::vector<int32_t> b16_ids[kBand16MaxQ + 1];  // band16 class by width Q (16-blocks)
  bool b16_p2 = false;                             // ... holding p = 2 problems (K band of 3 diagonals)
  for (int i = 0; i < n_active; ++i) {
    const int b = active[i];
    const double* thb = theta + (size_t)b * GPX_THETA_STRIDE;
    int w = -1;
    switch (route_one(bt, b, thb, L, w)) {
      case kRouteBand16:
        bt->h_bandp[b] = w;
        b16_ids[w].push_back(b);
        b16_p2 = b16_p2 || band_width(bt, b, thb) == 2;
        break;
      case kRouteFused:
        bt->h_bandp[b] = w;
        fused_ids.push_back(b);
        break;
      case kRouteBand:
        bt->h_bandp[b] = w;
        band_ids.push_back(b);
        pband = std::max(pband, w);
        break;
      case kRouteShadow:
        if (w >= 0 && w <= L.plim) bt->h_bandp[b] = w;
        rt.shadow_ids.push_back(b);
        break;
      default:
        order.push_back(b);
    }
  }
  rt.n16 = 0;
  for (int q = 1; q <= kBand16MaxQ; ++q) rt.n16 += (int)b16_ids[q].size();
  // the dense class: isotropic specs first, then the ARD ones, then the Coregion ones (each with
  // its own build and contraction; n_ard counts the ARD and the Coregion ones)
  const auto first_ard = std::stable_partition(order.begin(), order.end(),
                                               [&](int32_t b) { return dense_class(bt->specs[b]) == 0; });
  rt.n_ard = (int)(order.end() - first_ard);
  const auto first_cg = std::stable_partition(first_ard, order.end(),
                                              [&](int32_t b) { return dense_class(bt->specs[b]) != 2; });
  rt.n_cg = (int)(order.end() - first_cg);
  rt.n_dense = (int)order.size();
  rt.n_band = (int)band_ids.size();
  rt.n_fused = (int)fused_ids.size() + rt.n16;
  rt.pband = pband;
  rt.b16_p2 = b16_p2;
  order.insert(order.end(), band_ids.begin(), band_ids.end());
  // fused problems: the band16 class first (by width), then p <= 1 (its own two-blocks-per-CU
  // kernels), then p = 2
  rt.n_g16 = 0;
  for (int q = 1; q <= kBand16MaxQ; ++q)
    if (!b16_ids[q].empty()) {
      order.insert(order.end(), b16_ids[q].begin(), b16_ids[q].end());
      rt.g16_q[rt.n_g16] = q;
      rt.g16_n[rt.n_g16++] = (int)b16_ids[q].size();
    }
  rt.n_fused1 = 0;
  for (int b : fused_ids)
    if (bt->h_bandp[b] <= 1) order.push_back(b), ++rt.n_fused1;
  for (int b : fused_ids)
    if (bt->h_bandp[b] > 1) order.push_back(b);
}
// the reference's kernel: one SquaredExponential term on one input column (the band16 sweeps'
// straight-line contraction, and the only family of the Q > kBand16MaxQAny classes)
bool se1_spec(const gpx_kernel_spec& sp) {
  return sp.n_terms == 1 && sp.terms[0].kind == GPX_SE && sp.terms[0].dim_count == 1;
}

// a spec with an ARD term (GPX_TERM_ARD): never banded (band_kind refuses the flagged kind), always
// the dense route's ARD kernels
bool ard_spec(const gpx_kernel_spec& sp) {
  for (int t = 0; t < sp.n_terms && t < GPX_MAX_TERMS; ++t)
    if (sp.terms[t].kind & GPX_TERM_ARD) return true;
  return false;
}

// a spec with a Coregion term (GPX_COREGION): never banded (no band kind), always the dense route's
// Coregion kernels, whatever its partner terms are
bool coreg_spec(const gpx_kernel_spec& sp) {
  for (int t = 0; t < sp.n_terms && t < GPX_MAX_TERMS; ++t)
    if (sp.terms[t].kind == GPX_COREGION) return true;
  return false;
}

int dense_class(const gpx_kernel_spec& sp) { return coreg_spec(sp) ? 2 : ard_spec(sp) ? 1 : 0; }

unsigned signed_slot_mask(const gpx_kernel_spec& sp) {
  unsigned m = 0;
  const int P = sp.reserved & 0xff, R = (sp.reserved >> 8) & 0xff;
  for (int t = 0; t < sp.n_terms && t < GPX_MAX_TERMS; ++t) {
    if (sp.terms[t].kind != GPX_COREGION) continue;
    for (int e = 0; e < P * R; ++e) {
      const int p = sp.terms[t].param_offset + e;
      if (p >= 0 && p < GPX_THETA_STRIDE) m |= 1u << p;
    }
  }
  return m;
}

// (a Coregion term's count depends on the spec's P and R: spec_error counts it itself)
int term_param_count(const gpx_term& tm) {
  const int kind = tm.kind & GPX_TERM_KIND_MASK;
  const int np = (kind == GPX_RQ || kind == GPX_PERIODIC_SE) ? 3 : (kind == GPX_LINEAR ? 1 : 2);
  return (tm.kind & GPX_TERM_ARD) ? np - 1 + tm.dim_count : np;
}

const char* spec_error(const gpx_kernel_spec& sp, int D) {
  if (sp.n_terms < 1 || sp.n_terms > GPX_MAX_TERMS || sp.n_params < 1 || sp.n_params >= GPX_THETA_STRIDE)
    return "bad kernel spec";
  int staged = 0;
  bool ard = false, raw = false, coreg = false;
  for (int t = 0; t < sp.n_terms; ++t) {
    const gpx_term& tm = sp.terms[t];
    const int kind = tm.kind & GPX_TERM_KIND_MASK;
    if ((tm.kind & ~(GPX_TERM_ARD | GPX_TERM_KIND_MASK)) != 0 || kind < GPX_SE || kind > GPX_COREGION ||
        tm.dim_start < 0 || tm.dim_count < 1 || tm.dim_start + tm.dim_count > D || tm.param_offset < 0)
      return "bad kernel term";
    if (kind == GPX_COREGION) {
      // P | R << 8 in reserved; θ slots [W row-major (P·R), κ (P)]
      const int P = sp.reserved & 0xff, R = (sp.reserved >> 8) & 0xff;
      if (tm.kind & GPX_TERM_ARD) return "GPX_TERM_ARD is valid with the SE, Matern, Exponential and RationalQuadratic kinds only";
      if (tm.dim_count != 1) return "a Coregion term acts on exactly one input column (dim_count == 1)";
      if (coreg) return "a spec may hold one Coregion term";
      if (P < 1 || R < 1 || (sp.reserved & ~0xffff) != 0)
        return "a Coregion spec needs P >= 1 and R >= 1 in reserved (P | R << 8)";
      if (sp.n_terms > 1 && sp.combine != GPX_PRODUCT)
        return "a Coregion term is valid alone or in a GPX_PRODUCT spec, not in a GPX_SUM";
      if (tm.param_offset + P * R + P > sp.n_params) return "bad kernel term";
      coreg = true;
      continue;
    }
    if (tm.kind & GPX_TERM_ARD) {
      if (kind > GPX_RQ) return "GPX_TERM_ARD is valid with the SE, Matern, Exponential and RationalQuadratic kinds only";
      if (tm.dim_count < 2) return "GPX_TERM_ARD needs dim_count >= 2 (one active dim: the plain term)";
      ard = true;
    }
    if (tm.param_offset + term_param_count(tm) > sp.n_params) return "bad kernel term";
    if (kind <= GPX_RQ) staged += tm.dim_count;
    else raw = true;
  }
  // (the ARD kernels stage every stationary term's scaled rows, and the raw rows for Linear /
  // Periodic terms, in GPX_MAX_DIM doubles per row)
  if (ard && sp.n_params + 1 > GPX_THETA_STRIDE - 1)
    return "an ARD spec may use GPX_THETA_STRIDE - 1 columns of the theta row (kernel parameters + noise)";
  if (ard && staged + (raw ? D : 0) > GPX_MAX_DIM)
    return "an ARD spec's stationary terms cover more than GPX_MAX_DIM input columns in total";
  if (!coreg && sp.reserved != 0) return "reserved must be 0 in a spec without a Coregion term";
  if (coreg && sp.n_params + 1 > GPX_THETA_STRIDE - 1)
    return "a Coregion spec may use GPX_THETA_STRIDE - 1 columns of the theta row (kernel parameters + noise)";
  // (the Coregion kernels stage the partner terms' rows as the ARD kernels do, and the rows' output
  // indices in one more column)
  if (coreg && staged + (raw ? D : 0) + 1 > GPX_MAX_DIM)
    return "a Coregion spec's partner terms cover more than GPX_MAX_DIM - 1 input columns in total";
  return nullptr;
}

}  // namespace gpx

extern "C" {

int gpx_spec_signed_mask(const gpx_kernel_spec* spec, int D, uint32_t* mask_out) {
  if (!spec || !mask_out || D < 1 || D > GPX_MAX_DIM || spec_error(*spec, D)) return GPX_BAD_ARG;
  *mask_out = signed_slot_mask(*spec);
  return GPX_OK;
}

int gpx_batch_band_width(gpx_batch* bt, int n_rows, const int32_t* rows, const double* theta, int32_t* p_out) {
  if (!bt) return GPX_BAD_ARG;
  if (n_rows < 0 || (n_rows > 0 && (!rows || !theta || !p_out))) return fail(bt->ctx, GPX_BAD_ARG, "bad band-width query");
  const int plim = band_limit(bt);
  for (int i = 0; i < n_rows; ++i) {
    const int b = rows[i];
    if (b < 0 || b >= bt->B) return fail(bt->ctx, GPX_BAD_ARG, "row out of range");
    bool pending = false;
    for (const auto& e : bt->pend) pending = pending || e.b == b;
    if (pending) {  // its band tables arrive with the next call's gather
      p_out[i] = -2;
      continue;
    }
    // (a spec with an ARD or a Coregion term: band_width's −1, dense)
    const int p = plim >= 0 ? band_width(bt, b, theta + (size_t)b * GPX_THETA_STRIDE) : -1;
    p_out[i] = (p >= 0 && p <= plim) ? p : -1;
  }
  return GPX_OK;
}

int gpx_batch_band_class(gpx_batch* bt, int n_rows, const int32_t* rows, const double* theta, int32_t* cls_out) {
  if (!bt) return GPX_BAD_ARG;
  if (n_rows < 0 || (n_rows > 0 && (!rows || !theta || !cls_out)))
    return fail(bt->ctx, GPX_BAD_ARG, "bad band-class query");
  const RouteLimits L = route_limits(bt);
  for (int i = 0; i < n_rows; ++i) {
    const int b = rows[i];
    if (b < 0 || b >= bt->B) return fail(bt->ctx, GPX_BAD_ARG, "row out of range");
    bool pending = false;
    for (const auto& e : bt->pend) pending = pending || e.b == b;
    if (pending) {
      cls_out[i] = -2;
      continue;
    }
    int w = -1;
    const RouteKind k = route_one(bt, b, theta + (size_t)b * GPX_THETA_STRIDE, L, w);
    cls_out[i] = k == kRouteBand16 ? w : (k == kRouteFused || k == kRouteBand) ? (L.q16lim > 0 ? 32 : 16) + w : -1;
  }
  return GPX_OK;
}

}  // extern "C"
