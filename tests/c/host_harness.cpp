// Host-logic harness for the C ABI's pure host parts (SURVEY §5 sanitizers),
// built with AddressSanitizer + UndefinedBehaviorSanitizer on the HOST code only (hipcc
// --offload-host-only: no device code object at all, so nothing here can run on a GPU) and run
// by tests/test_host_harness.py on the CPU.
//
// What it checks, on seeded random batches:
//   * band_tables / band_tables_boxes (the per-block lower bounds on point distances the
//     banded routing rests on) — the two agree bit for bit;
//   * band_width / band_width16 are SAFE: every kernel entry beyond the reported band is an
//     exact fp64 zero by the device's own formula (GPflow's r², the term's exp argument), and
//     tight for sorted 1-D inputs (at most one block wider than the true band);
//   * route_call (gpx_route.hip: gpx_batch_lml_grad_submit's routing) puts every active problem
//     exactly once in [dense | per-block band | band16 by width | fused p <= 1 | fused p = 2] or on
//     the band-storage fallback, with class sizes, widths and h_bandp consistent, under the
//     GPX_BAND / GPX_BAND16 / GPX_BAND_FUSED switches;
//   * the knob table (gpx_knobs.h): every row's default when unset, the clamps and masks, the
//     derived rules, per-call knobs following the environment and Once knobs keeping their value;
//   * plan_lanes and split_deferred (gpx_eval.hip): recorded tables of what the code did before
//     they were separated out, and the plan's invariants on seeded random width groups.
// Exit status 0 and a final "OK" line when every check holds.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../portfoliooptgp_amd/csrc/gpx_host.h"

using namespace gpx;

static int g_fail = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (g_fail < 20) {                        \
        std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        std::fprintf(stderr, __VA_ARGS__);      \
        std::fprintf(stderr, "\n");             \
      }                                         \
      ++g_fail;                                 \
    }                                           \
  } while (0)

static double exp_arg(int kind, double s) {  // the term's exp argument a(s), s = r/ℓ
  switch (kind) {
    case GPX_SE: return 0.5 * s * s;
    case GPX_MATERN12: return s;
    case GPX_EXPONENTIAL: return 0.5 * s;
    case GPX_MATERN32: return std::sqrt(3.0) * s;
    default: return std::sqrt(5.0) * s;
  }
}

// is K_ij (and every ∂K/∂θ) nonzero by the device's formula: r² as GPflow's square_distance
// forms it on x/ℓ, r = sqrt(max(r², 1e-36)); a sum is nonzero when any term is, a product
// when all are
static bool entry_nz(const gpx_kernel_spec& sp, const double* th, const double* xi, const double* xj) {
  const bool prod = sp.n_terms > 1 && sp.combine == GPX_PRODUCT;
  bool nz = prod;
  for (int t = 0; t < sp.n_terms; ++t) {
    const gpx_term& tm = sp.terms[t];
    const double ell = th[tm.param_offset];
    double dot = 0.0, sa = 0.0, sb = 0.0;
    for (int d = tm.dim_start; d < tm.dim_start + tm.dim_count; ++d) {
      const double a = xi[d] / ell, b = xj[d] / ell;
      dot += a * b;
      sa += a * a;
      sb += b * b;
    }
    double r2 = -2.0 * dot + (sa + sb);
    r2 = r2 > 1e-36 ? r2 : 1e-36;
    const bool tnz = std::exp(-exp_arg(tm.kind, std::sqrt(r2))) != 0.0;
    nz = prod ? (nz && tnz) : (nz || tnz);
  }
  return nz;
}

struct Problem {
  gpx_kernel_spec sp{};
  std::vector<double> x;  // [n][D]
  int n = 0;
  bool sorted1d = false;
};

static gpx_kernel_spec make_spec(std::mt19937_64& rng, int D) {
  gpx_kernel_spec sp{};
  std::uniform_int_distribution<int> nt(1, 3), kind(GPX_SE, GPX_PERIODIC_SE), comb(0, 1);
  sp.n_terms = nt(rng);
  sp.combine = comb(rng);
  int off = 0;
  for (int t = 0; t < sp.n_terms; ++t) {
    int k = kind(rng);
    if (k == GPX_RQ && (rng() & 1)) k = GPX_SE;
    std::uniform_int_distribution<int> ds(0, D - 1);
    const int d0 = ds(rng);
    std::uniform_int_distribution<int> dc(1, D - d0);
    sp.terms[t] = gpx_term{k, d0, dc(rng), off};
    off += (k == GPX_RQ || k == GPX_PERIODIC_SE) ? 3 : 2;
  }
  sp.n_params = off;
  return sp;
}

// ---- the knob table (gpx_knobs.h) ----
// `host_harness knobs` prints every knob's value and the derived rules as this process sees them;
// the checks below run it as a child under chosen environments (the Once knobs are read once).
static int print_knobs() {
  for (int k = 0; k < (int)Knob::kCount; ++k) std::printf("%s %.17g\n", kKnobs[k].name, knob_value((Knob)k));
  std::printf("b16_inline_k_wide %d\nwide_qmax_se1 %d\nwide_qmax_any %d\nwide_bcr_on_sweeps %d\nwide_bcr_on_bcr %d\n"
              "wide_launch_qmax_se1 %d\nbcr_max_sweeps %d\nbcr_max_bcr %d\nbcr_max_auto %d\n",
              b16_inline_k_wide(), wide_qmax(true), wide_qmax(false), (int)wide_bcr_on(false), (int)wide_bcr_on(true),
              wide_launch_qmax(true), bcr_max_problems(GPX_BAND_ROUTE_SWEEPS), bcr_max_problems(GPX_BAND_ROUTE_BCR),
              bcr_max_problems(GPX_BAND_ROUTE_AUTO));
  return 0;
}

static std::map<std::string, double> child_knobs(const char* self, const std::string& env) {
  std::map<std::string, double> out;
  const std::string cmd = env + " '" + self + "' knobs";
  FILE* f = popen(cmd.c_str(), "r");
  CHECK(f != nullptr, "popen %s", cmd.c_str());
  if (!f) return out;
  char name[64];
  double v;
  while (std::fscanf(f, "%63s %lf", name, &v) == 2) out[name] = v;
  CHECK(pclose(f) == 0, "child failed: %s", cmd.c_str());
  return out;
}

static void check_knobs(const char* self) {
  for (int k = 0; k < (int)Knob::kCount; ++k) unsetenv(kKnobs[k].name);
  // unset: every row's default (and the rules derived from the defaults)
  std::map<std::string, double> d = child_knobs(self, "");
  for (int k = 0; k < (int)Knob::kCount; ++k) {
    CHECK(d.count(kKnobs[k].name) && d[kKnobs[k].name] == kKnobs[k].def, "%s unset: %g, table default %g",
          kKnobs[k].name, d[kKnobs[k].name], kKnobs[k].def);
    CHECK(knob_parse(kKnobs[k], nullptr) == kKnobs[k].def, "%s: knob_parse(unset)", kKnobs[k].name);
  }
  CHECK(d["GPX_B16_INLINE_K"] == 3 && d["b16_inline_k_wide"] == 3 && d["wide_qmax_se1"] == 8 && d["wide_qmax_any"] == 5,
        "inline-K / wide_qmax defaults");
  CHECK(d["GPX_WIDE_BCR"] == 1 && d["wide_bcr_on_sweeps"] == 0 && d["wide_bcr_on_bcr"] == 1 &&
        d["wide_launch_qmax_se1"] == 8, "wide_bcr defaults");
  CHECK(d["bcr_max_sweeps"] == 0 && d["bcr_max_bcr"] == (1 << 30) && d["bcr_max_auto"] == 32, "bcr_max_problems by route");
  CHECK(d["GPX_BAND_LANE_STREAMS"] == 1 + kAux && d["GPX_BAND16_QMAX"] == kBand16MaxQ && d["GPX_BAND_TOL"] == 1e-6 &&
        d["GPX_GROUPS"] == 1 && d["GPX_BAND_PMAX"] == -1, "documented defaults");
  // the clamps and masks, low side and high side
  std::map<std::string, double> lo = child_knobs(self, "GPX_WIDE_QMAX=3 GPX_WIDE_BCR=7 GPX_B16_INLINE_K=7 "
                                                       "GPX_BAND_LANE_STREAMS=0 GPX_LEAF128=0 GPX_BCR_MAX=5");
  CHECK(lo["GPX_WIDE_QMAX"] == 5 && lo["GPX_WIDE_BCR"] == 2 && lo["GPX_B16_INLINE_K"] == 3 &&
        lo["GPX_BAND_LANE_STREAMS"] == 1 && lo["GPX_LEAF128"] == 0, "clamps: WIDE_QMAX 3->%g WIDE_BCR 7->%g INLINE_K 7->%g "
        "LANE_STREAMS 0->%g", lo["GPX_WIDE_QMAX"], lo["GPX_WIDE_BCR"], lo["GPX_B16_INLINE_K"], lo["GPX_BAND_LANE_STREAMS"]);
  CHECK(lo["wide_bcr_on_sweeps"] == 1 && lo["wide_launch_qmax_se1"] == kBcrMaxQ && lo["wide_qmax_se1"] == 5,
        "GPX_WIDE_BCR=2: the wide launch stops at kBcrMaxQ");
  CHECK(lo["bcr_max_sweeps"] == 5 && lo["bcr_max_bcr"] == 5, "GPX_BCR_MAX overrides the batch's route");
  std::map<std::string, double> hi = child_knobs(self, "GPX_WIDE_QMAX=99 GPX_WIDE_BCR=-1 GPX_B16_INLINE_K=1 "
                                                       "GPX_B16_INLINE_K_WIDE=6 GPX_DEFER_STREAM=0 GPX_SLOW_DIRECT=2");
  CHECK(hi["GPX_WIDE_QMAX"] == 8 && hi["GPX_WIDE_BCR"] == 0 && hi["wide_bcr_on_bcr"] == 0, "clamps: WIDE_QMAX 99->%g "
        "WIDE_BCR -1->%g", hi["GPX_WIDE_QMAX"], hi["GPX_WIDE_BCR"]);
  CHECK(hi["GPX_B16_INLINE_K"] == 1 && hi["b16_inline_k_wide"] == 2 && hi["wide_qmax_se1"] == 5,
        "GPX_B16_INLINE_K_WIDE is its own mask; wide_qmax is 5 without wide inline K");
  CHECK(hi["GPX_DEFER_STREAM"] == 0 && hi["GPX_SLOW_DIRECT"] == 1, "flags");
  std::map<std::string, double> in1 = child_knobs(self, "GPX_B16_INLINE_K=1");
  CHECK(in1["b16_inline_k_wide"] == 1, "b16_inline_k_wide defaults to b16_inline_k");
  // every per-call knob reflects a change between two reads in this process
  static const struct { Knob k; const char* a; double va; const char* b; double vb; } percall[] = {
      {Knob::BcrMax, "7", 7, "0", 0},       {Knob::Band, "0", 0, "1", 1},         {Knob::BandPmax, "3", 3, "9", 9},
      {Knob::Band16, "0", 0, "2", 1},       {Knob::BandFused, "0", 0, "1", 1},    {Knob::Band16Qmax, "5", 5, "11", 8},
      {Knob::BandTol, "1e-30", 1e-30, "0.5", 0.5}, {Knob::Groups, "2", 2, "9", kGroups}};
  int n_percall = 0;
  for (int k = 0; k < (int)Knob::kCount; ++k) n_percall += kKnobs[k].read == KnobRead::PerCall;
  CHECK(n_percall == (int)(sizeof(percall) / sizeof(percall[0])), "a per-call knob without a check here");
  for (const auto& p : percall) {
    const KnobDef& kd = kKnobs[(int)p.k];
    CHECK(kd.read == KnobRead::PerCall, "%s is not per call", kd.name);
    setenv(kd.name, p.a, 1);
    CHECK(knob_value(p.k) == p.va, "%s=%s reads %g", kd.name, p.a, knob_value(p.k));
    setenv(kd.name, p.b, 1);
    CHECK(knob_value(p.k) == p.vb, "%s=%s reads %g", kd.name, p.b, knob_value(p.k));
    unsetenv(kd.name);
    CHECK(knob_value(p.k) == kd.def, "%s unset reads %g", kd.name, knob_value(p.k));
  }
  // a Once knob keeps its first value
  CHECK(wide_bcr_mode() == 1, "GPX_WIDE_BCR unset");
  setenv("GPX_WIDE_BCR", "2", 1);
  CHECK(wide_bcr_mode() == 1, "GPX_WIDE_BCR changed inside the process");
  unsetenv("GPX_WIDE_BCR");
}

// ---- plan_lanes and split_deferred (gpx_eval.hip) ----
struct PlanCase {
  int wide_bcr_mode, lane_order, n_g16, q[kBand16MaxQ], n[kBand16MaxQ], n1, n2, se1, bcr_q, wide_from, nl;
  long long need;
  Lane lanes[kMaxLanes];
};
// Recorded from band_fused_eval as it stood before it was split into plan and dispatch (a scratch
// copy of its lane block with a print), under GPX_WIDE_BCR = 0, 1, 2 and GPX_LANE_ORDER = 0, 1,
// Nmax = 2000: a Q = 3-only call; Q = 3, 4, 5 with wide_from = 1; a Q = 4..8 deferred part, SE1 and
// not; a reduction-route call with Q = 2, 5, 7; each with no tail, a p <= 1 tail and a p = 2 tail.
static const PlanCase kPlanCases[] = {
    {0, 0, 1, {3}, {10}, 0, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {0, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}}},
    {0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 1, 0, 1, 1, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}}},
    {0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 0, 0, 1, 5, 0LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}}},
    {0, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 0, 1, 1, 0, 3, 3649060LL, {{LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::Band16, 2, 3, 1, 5, 0LL}}},
    {0, 0, 1, {3}, {10}, 5, 0, 1, 0, 0, 2, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}, {LaneKind::Fused1, 0, 0, 5, 10, 0LL}}},
    {0, 0, 3, {3, 4, 5}, {12, 7, 3}, 5, 0, 1, 0, 1, 3, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused1, 0, 0, 5, 22, 0LL}}},
    {0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}}},
    {0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 0, 0, 1, 6, 0LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}}},
    {0, 0, 3, {2, 5, 7}, {3, 2, 1}, 5, 0, 1, 1, 0, 4, 3649060LL, {{LaneKind::Fused1, 0, 0, 5, 6, 0LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::Band16, 2, 3, 1, 5, 0LL}}},
    {0, 0, 1, {3}, {10}, 0, 11, 1, 0, 0, 2, 0LL, {{LaneKind::Fused2, 0, 0, 11, 10, 0LL}, {LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {0, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 11, 1, 0, 1, 3, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 22, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}}},
    {0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 1, 0, 1, 2, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 24, 0LL}}},
    {0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 0, 0, 1, 6, 0LL, {{LaneKind::Fused2, 0, 0, 11, 24, 0LL}, {LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}}},
    {0, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 11, 1, 1, 0, 4, 3649060LL, {{LaneKind::Fused2, 0, 0, 11, 6, 0LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::Band16, 2, 3, 1, 5, 0LL}}},
    {0, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 9, 1, 0, 1, 4, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused2, 0, 0, 9, 26, 0LL}, {LaneKind::Fused1, 0, 0, 4, 22, 0LL}}},
    {0, 0, 0, {}, {}, 3, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Fused1, 0, 0, 3, 0, 0LL}}},
    {1, 0, 1, {3}, {10}, 0, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {1, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}}},
    {1, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 1, 0, 1, 1, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}}},
    {1, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 0, 0, 1, 5, 0LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}}},
    {1, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 0, 1, 1, 0, 3, 5494581LL, {{LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}}},
    {1, 0, 1, {3}, {10}, 5, 0, 1, 0, 0, 2, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}, {LaneKind::Fused1, 0, 0, 5, 10, 0LL}}},
    {1, 0, 3, {3, 4, 5}, {12, 7, 3}, 5, 0, 1, 0, 1, 3, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused1, 0, 0, 5, 22, 0LL}}},
    {1, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}}},
    {1, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 0, 0, 1, 6, 0LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}}},
    {1, 0, 3, {2, 5, 7}, {3, 2, 1}, 5, 0, 1, 1, 0, 4, 5494581LL, {{LaneKind::Fused1, 0, 0, 5, 6, 0LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}}},
    {1, 0, 1, {3}, {10}, 0, 11, 1, 0, 0, 2, 0LL, {{LaneKind::Fused2, 0, 0, 11, 10, 0LL}, {LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {1, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 11, 1, 0, 1, 3, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 22, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}}},
    {1, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 1, 0, 1, 2, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 24, 0LL}}},
    {1, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 0, 0, 1, 6, 0LL, {{LaneKind::Fused2, 0, 0, 11, 24, 0LL}, {LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}}},
    {1, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 11, 1, 1, 0, 4, 5494581LL, {{LaneKind::Fused2, 0, 0, 11, 6, 0LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}}},
    {1, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 9, 1, 0, 1, 4, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused2, 0, 0, 9, 26, 0LL}, {LaneKind::Fused1, 0, 0, 4, 22, 0LL}}},
    {1, 0, 0, {}, {}, 3, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Fused1, 0, 0, 3, 0, 0LL}}},
    {2, 0, 1, {3}, {10}, 0, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {2, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}}},
    {2, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 1, 0, 1, 2, 16609689LL, {{LaneKind::Wide16, 0, 2, 15, 0, 0LL}, {LaneKind::BcrWide, 2, 5, 9, 15, 0LL}}},
    {2, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 0, 0, 1, 3, 16609689LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::BcrWide, 2, 5, 9, 15, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}}},
    {2, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 0, 1, 1, 0, 3, 5494581LL, {{LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}}},
    {2, 0, 1, {3}, {10}, 5, 0, 1, 0, 0, 2, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}, {LaneKind::Fused1, 0, 0, 5, 10, 0LL}}},
    {2, 0, 3, {3, 4, 5}, {12, 7, 3}, 5, 0, 1, 0, 1, 3, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused1, 0, 0, 5, 22, 0LL}}},
    {2, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 1, 0, 1, 3, 16609689LL, {{LaneKind::Wide16, 0, 2, 15, 0, 0LL}, {LaneKind::BcrWide, 2, 5, 9, 15, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}}},
    {2, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 0, 0, 1, 4, 16609689LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::BcrWide, 2, 5, 9, 15, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}}},
    {2, 0, 3, {2, 5, 7}, {3, 2, 1}, 5, 0, 1, 1, 0, 4, 5494581LL, {{LaneKind::Fused1, 0, 0, 5, 6, 0LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}}},
    {2, 0, 1, {3}, {10}, 0, 11, 1, 0, 0, 2, 0LL, {{LaneKind::Fused2, 0, 0, 11, 10, 0LL}, {LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {2, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 11, 1, 0, 1, 3, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 22, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}}},
    {2, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 1, 0, 1, 3, 16609689LL, {{LaneKind::Wide16, 0, 2, 15, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 24, 0LL}, {LaneKind::BcrWide, 2, 5, 9, 15, 0LL}}},
    {2, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 0, 0, 1, 4, 16609689LL, {{LaneKind::Fused2, 0, 0, 11, 24, 0LL}, {LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::BcrWide, 2, 5, 9, 15, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}}},
    {2, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 11, 1, 1, 0, 4, 5494581LL, {{LaneKind::Fused2, 0, 0, 11, 6, 0LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}}},
    {2, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 9, 1, 0, 1, 4, 0LL, {{LaneKind::Band16, 0, 1, 12, 0, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused2, 0, 0, 9, 26, 0LL}, {LaneKind::Fused1, 0, 0, 4, 22, 0LL}}},
    {2, 0, 0, {}, {}, 3, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Fused1, 0, 0, 3, 0, 0LL}}},
    {1, 1, 1, {3}, {10}, 0, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {1, 1, 3, {3, 4, 5}, {12, 7, 3}, 0, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Band16, 0, 1, 12, 0, 0LL}}},
    {1, 1, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 1, 0, 1, 1, 0LL, {{LaneKind::Wide16, 0, 5, 24, 0, 0LL}}},
    {1, 1, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 0, 0, 1, 5, 0LL, {{LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}, {LaneKind::Band16, 0, 1, 9, 0, 0LL}}},
    {1, 1, 3, {2, 5, 7}, {3, 2, 1}, 0, 0, 1, 1, 0, 3, 5494581LL, {{LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}, {LaneKind::Bcr, 0, 1, 3, 0, 0LL}}},
    {1, 1, 1, {3}, {10}, 5, 0, 1, 0, 0, 2, 0LL, {{LaneKind::Fused1, 0, 0, 5, 10, 0LL}, {LaneKind::Band16, 0, 1, 10, 0, 0LL}}},
    {1, 1, 3, {3, 4, 5}, {12, 7, 3}, 5, 0, 1, 0, 1, 3, 0LL, {{LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused1, 0, 0, 5, 22, 0LL}, {LaneKind::Band16, 0, 1, 12, 0, 0LL}}},
    {1, 1, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 1, 0, 1, 2, 0LL, {{LaneKind::Fused1, 0, 0, 5, 24, 0LL}, {LaneKind::Wide16, 0, 5, 24, 0, 0LL}}},
    {1, 1, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 5, 0, 0, 0, 1, 6, 0LL, {{LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Fused1, 0, 0, 5, 24, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}, {LaneKind::Band16, 0, 1, 9, 0, 0LL}}},
    {1, 1, 3, {2, 5, 7}, {3, 2, 1}, 5, 0, 1, 1, 0, 4, 5494581LL, {{LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}, {LaneKind::Fused1, 0, 0, 5, 6, 0LL}}},
    {1, 1, 1, {3}, {10}, 0, 11, 1, 0, 0, 2, 0LL, {{LaneKind::Band16, 0, 1, 10, 0, 0LL}, {LaneKind::Fused2, 0, 0, 11, 10, 0LL}}},
    {1, 1, 3, {3, 4, 5}, {12, 7, 3}, 0, 11, 1, 0, 1, 3, 0LL, {{LaneKind::Fused2, 0, 0, 11, 22, 0LL}, {LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Band16, 0, 1, 12, 0, 0LL}}},
    {1, 1, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 1, 0, 1, 2, 0LL, {{LaneKind::Fused2, 0, 0, 11, 24, 0LL}, {LaneKind::Wide16, 0, 5, 24, 0, 0LL}}},
    {1, 1, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 11, 0, 0, 1, 6, 0LL, {{LaneKind::Band16, 0, 1, 9, 0, 0LL}, {LaneKind::Band16, 1, 2, 6, 9, 0LL}, {LaneKind::Band16, 2, 3, 4, 15, 0LL}, {LaneKind::Band16, 3, 4, 3, 19, 0LL}, {LaneKind::Band16, 4, 5, 2, 22, 0LL}, {LaneKind::Fused2, 0, 0, 11, 24, 0LL}}},
    {1, 1, 3, {2, 5, 7}, {3, 2, 1}, 0, 11, 1, 1, 0, 4, 5494581LL, {{LaneKind::Bcr, 0, 1, 3, 0, 0LL}, {LaneKind::Bcr, 1, 2, 2, 3, 1388208LL}, {LaneKind::BcrWide, 2, 3, 1, 5, 3649060LL}, {LaneKind::Fused2, 0, 0, 11, 6, 0LL}}},
    {1, 1, 3, {3, 4, 5}, {12, 7, 3}, 4, 9, 1, 0, 1, 4, 0LL, {{LaneKind::Wide16, 1, 3, 10, 12, 0LL}, {LaneKind::Fused2, 0, 0, 9, 26, 0LL}, {LaneKind::Fused1, 0, 0, 4, 22, 0LL}, {LaneKind::Band16, 0, 1, 12, 0, 0LL}}},
    {1, 1, 0, {}, {}, 3, 0, 1, 0, 0, 1, 0LL, {{LaneKind::Fused1, 0, 0, 3, 0, 0LL}}},
};
static const int kPlanNmax = 2000;

static LaneLimits limits_of(int mode, int lane_order, bool se1, int bcr_q) {
  return LaneLimits{se1 ? 8 : 5, mode == 2 || (mode == 1 && bcr_q > 0), lane_order};
}

static long long lane_slot(const Lane& l, const int* q, int Nmax) {
  return bcr_ws_doubles(l.kind == LaneKind::BcrWide ? kBcrWideQ : q[l.g], Nmax);
}

static void check_plan_properties(const LanePlan& P, int n_g16, const int* q, const int* n, int n16, int n1, int na,
                                  bool se1, int bcr_q, int wide_from, const LaneLimits& lim, int Nmax, const char* what) {
  CHECK(P.nl >= 0 && P.nl <= kMaxLanes, "%s: %d lanes", what, P.nl);
  std::vector<int> goff(n_g16 + 1, 0);
  for (int g = 0; g < n_g16; ++g) goff[g + 1] = goff[g] + n[g];
  // the lanes' ranges tile [0, na) exactly once
  std::vector<Lane> by_off(P.lanes, P.lanes + P.nl);
  std::sort(by_off.begin(), by_off.end(), [](const Lane& a, const Lane& b) { return a.off < b.off; });
  int pos = 0;
  for (const Lane& l : by_off) {
    CHECK(l.off == pos && l.n > 0, "%s: lane at %d (+%d), expected at %d", what, l.off, l.n, pos);
    pos = l.off + l.n;
  }
  CHECK(pos == na, "%s: lanes cover %d of %d", what, pos, na);
  long long need = 0;
  std::vector<std::pair<long long, long long>> ws;
  for (int i = 0; i < P.nl; ++i) {
    const Lane& l = P.lanes[i];
    const bool b16 = l.kind != LaneKind::Fused1 && l.kind != LaneKind::Fused2;
    if (b16) {  // its groups are adjacent and are exactly its problems
      CHECK(l.g >= 0 && l.g < l.g_end && l.g_end <= n_g16 && l.off == goff[l.g] && l.n == goff[l.g_end] - goff[l.g],
            "%s: lane groups [%d, %d) vs range %d (+%d)", what, l.g, l.g_end, l.off, l.n);
      if (!(l.g >= 0 && l.g < l.g_end && l.g_end <= n_g16)) continue;
      CHECK(l.g_end == l.g + 1 || l.kind == LaneKind::Wide16 || l.kind == LaneKind::BcrWide, "%s: merged lane kind", what);
    } else {
      CHECK(l.off == (l.kind == LaneKind::Fused1 ? n16 : n16 + n1) && l.n == (l.kind == LaneKind::Fused1 ? n1 : na - n16 - n1),
            "%s: 64-row lane range", what);
      continue;
    }
    for (int g = l.g; g < l.g_end; ++g) {
      if (l.kind == LaneKind::Wide16)
        CHECK(se1 && wide_from > 0 && q[g] >= 4 && q[g] <= lim.wide_qmax, "%s: wide lane holds Q = %d", what, q[g]);
      if (l.kind == LaneKind::Bcr) CHECK(bcr_q > 0 && q[g] <= kBcrMaxQ, "%s: reduction lane holds Q = %d", what, q[g]);
      if (l.kind == LaneKind::BcrWide) CHECK(lim.wide_bcr && q[g] > kBcrMaxQ, "%s: block-128 lane holds Q = %d", what, q[g]);
    }
    if (l.kind == LaneKind::Bcr || l.kind == LaneKind::BcrWide) {
      ws.push_back({l.wso, l.wso + (long long)l.n * lane_slot(l, q, Nmax)});
      need = std::max(need, ws.back().second);
    }
  }
  std::sort(ws.begin(), ws.end());
  for (size_t i = 0; i < ws.size(); ++i)
    CHECK(ws[i].first >= 0 && (i == 0 || ws[i].first >= ws[i - 1].second), "%s: reduction workspaces overlap", what);
  CHECK(P.ws_need >= need && (need > 0 || P.ws_need == 0), "%s: workspace need %lld, lanes use %lld", what, P.ws_need, need);
  // largest first; GPX_LANE_ORDER=1: the bulk lane last
  const int last = (lim.lane_order == 1 && P.nl > 1) ? P.nl - 1 : P.nl;
  for (int i = 1; i < last; ++i) CHECK(P.lanes[i].n <= P.lanes[i - 1].n, "%s: lanes not in size order", what);
  if (last < P.nl)
    for (int i = 0; i < last; ++i) CHECK(P.lanes[i].n <= P.lanes[last].n, "%s: the bulk lane is not last", what);
}

static void check_plan_lanes(std::mt19937_64& rng) {
  char what[96];
  int ci = 0;
  for (const PlanCase& c : kPlanCases) {
    std::snprintf(what, sizeof(what), "plan case %d", ci++);
    int n16 = 0;
    for (int g = 0; g < c.n_g16; ++g) n16 += c.n[g];
    const int na = n16 + c.n1 + c.n2;
    const LaneLimits lim = limits_of(c.wide_bcr_mode, c.lane_order, c.se1 != 0, c.bcr_q);
    const LanePlan P = plan_lanes(c.n_g16, c.q, c.n, n16, c.n1, na, c.se1 != 0, c.bcr_q, c.wide_from, lim, kPlanNmax);
    CHECK(P.nl == c.nl && P.ws_need == c.need, "%s: %d lanes need %lld, recorded %d need %lld", what, P.nl, P.ws_need,
          c.nl, c.need);
    for (int i = 0; i < std::min(P.nl, c.nl); ++i) {
      const Lane &a = P.lanes[i], &b = c.lanes[i];
      CHECK(a.kind == b.kind && a.g == b.g && a.g_end == b.g_end && a.n == b.n && a.off == b.off && a.wso == b.wso,
            "%s lane %d: {%d, %d, %d, %d, %d, %lld} recorded {%d, %d, %d, %d, %d, %lld}", what, i, (int)a.kind, a.g,
            a.g_end, a.n, a.off, a.wso, (int)b.kind, b.g, b.g_end, b.n, b.off, b.wso);
    }
    check_plan_properties(P, c.n_g16, c.q, c.n, n16, c.n1, na, c.se1 != 0, c.bcr_q, c.wide_from, lim, kPlanNmax, what);
  }
  CHECK(wide_qmax(true) == 8 && wide_qmax(false) == 5, "wide_qmax under the default environment");
  for (int round = 0; round < 200; ++round) {
    int q[kBand16MaxQ], n[kBand16MaxQ], n_g16 = 0, n16 = 0;
    const int want = (int)(rng() % (kBand16MaxQ + 1));
    for (int w = 1; w <= kBand16MaxQ; ++w)  // widths strictly increasing in 1..8
      if ((int)(rng() % (kBand16MaxQ - w + 1)) < want - n_g16) {
        q[n_g16] = w;
        n[n_g16] = 1 + (int)(rng() % 40);
        n16 += n[n_g16++];
      }
    const int n1 = (int)(rng() % 21), n2 = (int)(rng() % 21), na = n16 + n1 + n2;
    const int Nmax = 449 + (int)(rng() % 4000);
    for (int v = 0; v < 48; ++v) {
      const bool se1 = v & 1;
      const int bcr_q = (v >> 1) & 1, wide_from = (v >> 2) & 1, lane_order = (v >> 3) & 1, mode = v / 16;
      const LaneLimits lim = limits_of(mode, lane_order, se1, bcr_q);
      const LanePlan P = plan_lanes(n_g16, q, n, n16, n1, na, se1, bcr_q, wide_from, lim, Nmax);
      std::snprintf(what, sizeof(what), "random plan %d variant %d", round, v);
      check_plan_properties(P, n_g16, q, n, n16, n1, na, se1, bcr_q, wide_from, lim, Nmax, what);
    }
  }
}

struct SplitCase {
  int defer_q, bcr_q, head, n_g16, q[kBand16MaxQ], n[kBand16MaxQ], n_fused1, n2, n_slow, n_g16_run, n16_run, n_fused1_run;
};
// Recorded the same way from gpx_batch_lml_grad_submit's deferred split: deferral off; Q = 3 runs
// and the rest is slow; a call of slow problems only (just runs) and the same beside dense
// problems; the reduction route (no deferral); only 64-row problems slow; nothing slow; defer_q = 0.
static const SplitCase kSplitCases[] = {
    {-1, 0, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 2, 0, 3, 22, 4},
    {3, 0, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 2, 16, 1, 12, 0},
    {3, 0, 0, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 0, 5, 24, 0},
    {3, 0, 5, 5, {4, 5, 6, 7, 8}, {9, 6, 4, 3, 2}, 0, 0, 24, 0, 0, 0},
    {3, 1, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 2, 0, 3, 22, 4},
    {5, 0, 0, 3, {3, 4, 5}, {12, 7, 3}, 4, 2, 6, 3, 22, 0},
    {5, 0, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 5, 5, 3, 22, 0},
    {5, 0, 0, 3, {3, 4, 5}, {12, 7, 3}, 0, 0, 0, 3, 22, 0},
    {3, 0, 0, 1, {3}, {10}, 0, 0, 0, 1, 10, 0},
    {0, 0, 0, 1, {3}, {10}, 3, 0, 0, 1, 10, 3},
    {0, 0, 2, 1, {3}, {10}, 3, 0, 13, 0, 0, 0},
    {4, 0, 0, 3, {2, 5, 7}, {3, 2, 1}, 0, 1, 4, 1, 3, 0},
    {3, 0, 0, 0, {}, {}, 6, 2, 0, 0, 0, 6},
    {3, 0, 1, 0, {}, {}, 6, 2, 8, 0, 0, 0},
};

static void check_split_deferred() {
  int ci = 0;
  for (const SplitCase& c : kSplitCases) {
    int n16 = 0;
    for (int g = 0; g < c.n_g16; ++g) n16 += c.n[g];
    const DeferSplit s = split_deferred(c.defer_q, c.bcr_q, c.head, c.n_g16, c.q, c.n, n16, c.n_fused1, n16 + c.n_fused1 + c.n2);
    CHECK(s.n_slow == c.n_slow && s.n_g16_run == c.n_g16_run && s.n16_run == c.n16_run && s.n_fused1_run == c.n_fused1_run,
          "split case %d: {%d, %d, %d, %d} recorded {%d, %d, %d, %d}", ci, s.n_slow, s.n_g16_run, s.n16_run,
          s.n_fused1_run, c.n_slow, c.n_g16_run, c.n16_run, c.n_fused1_run);
    ++ci;
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "knobs") return print_knobs();
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 40;
  std::mt19937_64 rng(20261017);
  check_knobs(argv[0]);
  {
    std::mt19937_64 prng(20261019);
    check_plan_lanes(prng);
  }
  check_split_deferred();
  long long checked_pairs = 0, routed = 0, band16_routed = 0, tight_checked = 0;
  for (int round = 0; round < rounds; ++round) {
    const int D = 1 + (int)(rng() % 3);
    const int Nmax = (round % 4 == 0) ? 4096 : 512 + 64 * (int)(rng() % 24);
    const int B = 6;
    gpx_batch bt;
    bt.B = B;
    bt.Nmax = Nmax;
    bt.D = D;
    bt.Np = (Nmax + 63) / 64 * 64;
    bt.compact = (round % 3 == 1);
    bt.n.assign(B, 0);
    bt.specs.assign(B, gpx_kernel_spec{});
    bt.band_rmin.assign((size_t)B * GPX_MAX_TERMS * (bt.Np / kLeaf), INFINITY);
    bt.band_tail.assign((size_t)B * GPX_MAX_TERMS, bt.Np / kLeaf);
    bt.band_rmin16.assign((size_t)B * GPX_MAX_TERMS * (bt.Np / kBox), INFINITY);
    bt.band_tail16.assign((size_t)B * GPX_MAX_TERMS, bt.Np / kBox);
    std::vector<int> bandp(B, -7);
    bt.h_bandp = bandp.data();
    std::vector<Problem> pr(B);
    std::vector<double> theta((size_t)B * GPX_THETA_STRIDE, 1.0);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    for (int b = 0; b < B; ++b) {
      Problem& p = pr[b];
      p.n = (b == 0) ? Nmax : std::max(1, (int)(Nmax * (0.3 + 0.7 * U(rng))));
      // inputs: unit-spaced day offsets (the reference's), jittered sorted, scaled, or random
      // (problems 0, 1: the reference's kernel on day offsets, C2's regime)
      const int mode = b < 2 ? (int)(rng() % 2) : (int)(rng() % 4);
      if (mode == 3) p.n = std::min(p.n, 1024);  // (unsorted inputs: every pair is brute-forced)
      p.sorted1d = D == 1 && mode <= 2;
      p.x.assign((size_t)p.n * D, 0.0);
      const double scale = mode == 2 ? 0.05 + 3.0 * U(rng) : 1.0;
      for (int i = 0; i < p.n; ++i)
        for (int d = 0; d < D; ++d) {
          double v;
          if (mode == 0) v = (double)i;
          else if (mode == 1) v = i + 0.4 * U(rng);
          else if (mode == 2) v = i * scale;
          else v = 4096.0 * U(rng);
          p.x[(size_t)i * D + d] = (D > 1 && d > 0 && mode != 3) ? v + d : v;
        }
      p.sp = (b < 2) ? gpx_kernel_spec{1, 0, 2, 0, {gpx_term{GPX_SE, 0, 1, 0}}} : make_spec(rng, D);
      bt.n[b] = p.n;
      bt.specs[b] = p.sp;
      // θ: lengthscales from 0.3 to 60 (bands from one block to dense)
      double* th = theta.data() + (size_t)b * GPX_THETA_STRIDE;
      for (int q = 0; q < p.sp.n_params; ++q) th[q] = 0.5 + U(rng);
      for (int t = 0; t < p.sp.n_terms; ++t) th[p.sp.terms[t].param_offset] = 0.3 * std::pow(200.0, U(rng));
      if (b < 2) th[0] = 0.8 + 1.4 * U(rng);  // ℓ ∈ [0.8, 2.2]: band16 widths Q = 2..6
      th[p.sp.n_params] = 1e-5;
      band_tables(&bt, b, p.x.data());
      // the box path (gpx_batch_rebind_device's gather hands back 16-row boxes) gives the same tables
      {
        const int nv16 = (p.n + kBox - 1) / kBox;
        std::vector<double> box((size_t)nv16 * D * 2);
        for (int k = 0; k < nv16; ++k)
          for (int d = 0; d < D; ++d) {
            double a = INFINITY, z = -INFINITY;
            for (int r = k * kBox; r < std::min(p.n, (k + 1) * kBox); ++r) {
              a = std::min(a, p.x[(size_t)r * D + d]);
              z = std::max(z, p.x[(size_t)r * D + d]);
            }
            box[2 * ((size_t)k * D + d)] = a;
            box[2 * ((size_t)k * D + d) + 1] = z;
          }
        const size_t t64 = (size_t)GPX_MAX_TERMS * (bt.Np / kLeaf), t16 = (size_t)GPX_MAX_TERMS * (bt.Np / kBox);
        std::vector<double> r64(bt.band_rmin.begin() + b * t64, bt.band_rmin.begin() + (b + 1) * t64);
        std::vector<double> r16(bt.band_rmin16.begin() + b * t16, bt.band_rmin16.begin() + (b + 1) * t16);
        band_tables_boxes(&bt, b, box.data());
        bool same = true;
        for (size_t e = 0; e < t64; ++e) same = same && r64[e] == bt.band_rmin[b * t64 + e];
        for (size_t e = 0; e < t16; ++e) same = same && r16[e] == bt.band_rmin16[b * t16 + e];
        CHECK(same, "round %d problem %d: band_tables_boxes differs from band_tables", round, b);
      }
    }
    // widths: safe and (sorted 1-D) tight
    for (int b = 0; b < B; ++b) {
      const Problem& p = pr[b];
      const double* th = theta.data() + (size_t)b * GPX_THETA_STRIDE;
      const int w64 = band_width(&bt, b, th), w16 = band_width16(&bt, b, th);
      bool bandable = true;
      for (int t = 0; t < p.sp.n_terms; ++t) bandable = bandable && p.sp.terms[t].kind <= GPX_EXPONENTIAL;
      CHECK((w64 < 0) == !bandable, "round %d problem %d: band_width %d for a %s kernel", round, b, w64,
            bandable ? "band" : "non-band");
      if (!bandable) continue;
      // true widths from every pair (i > j) within reach: beyond the reported band every entry
      // must be an exact zero
      int t64 = 0, t16 = 0;
      const int reach = std::min(p.n, 64 * (w64 + 3));
      for (int i = 0; i < p.n; ++i) {
        const int j0 = p.sorted1d ? std::max(0, i - reach) : 0;
        for (int j = j0; j < i; ++j) {
          if ((i >> 6) - (j >> 6) <= t64 && (i >> 4) - (j >> 4) <= t16) continue;
          ++checked_pairs;
          if (entry_nz(p.sp, th, &p.x[(size_t)i * D], &p.x[(size_t)j * D])) {
            t64 = std::max(t64, (i >> 6) - (j >> 6));
            t16 = std::max(t16, (i >> 4) - (j >> 4));
          }
        }
      }
      CHECK(w64 >= t64, "round %d problem %d: band_width %d < true %d (nonzero entries beyond the band)", round, b,
            w64, t64);
      CHECK(w16 >= t16, "round %d problem %d: band_width16 %d < true %d", round, b, w16, t16);
      // tight for sorted 1-D inputs while the true band is inside the tables' exact range (beyond
      // the widest band any path routes the tables repeat a lower bound: "dense", by design)
      if (p.sorted1d && p.sp.n_terms == 1) {
        const int cap64 = bt.Np / kLeaf / 4 + 1, cap16 = kBand16MaxQ + 1;
        if (t64 + 1 < cap64)
          CHECK(w64 <= t64 + 1, "round %d problem %d: band_width %d loose (true %d)", round, b, w64, t64);
        if (t16 + 1 < cap16)
          CHECK(w16 <= t16 + 1, "round %d problem %d: band_width16 %d loose (true %d)", round, b, w16, t16);
        tight_checked += (t16 + 1 < cap16);
      }
    }
    // routing under the switches
    static const char* envs[][2] = {{"GPX_BAND", nullptr}, {"GPX_BAND16", "0"}, {"GPX_BAND_FUSED", "0"},
                                    {"GPX_BAND", "0"}};
    for (int v = 0; v < 4; ++v) {
      unsetenv("GPX_BAND");
      unsetenv("GPX_BAND16");
      unsetenv("GPX_BAND_FUSED");
      if (envs[v][1]) setenv(envs[v][0], envs[v][1], 1);
      std::vector<int32_t> active;
      for (int b = 0; b < B; ++b)
        if (v == 0 || (rng() & 3)) active.push_back(b);
      std::fill(bandp.begin(), bandp.end(), -7);
      Route rt;
      route_call(&bt, (int)active.size(), active.data(), theta.data(), rt);
      std::vector<int> seen(B, 0);
      for (int b : rt.order) seen[b]++;
      for (int b : rt.shadow_ids) seen[b]++;
      for (int b = 0; b < B; ++b) {
        const bool act = std::find(active.begin(), active.end(), b) != active.end();
        CHECK(seen[b] == (act ? 1 : 0), "round %d env %d: problem %d routed %d times", round, v, b, seen[b]);
      }
      CHECK((int)rt.order.size() == rt.n_dense + rt.n_band + rt.n_fused, "order size %zu vs classes", rt.order.size());
      CHECK(!bt.compact || (rt.n_dense == 0 && rt.n_band == 0), "band storage routed problems to dense/per-block");
      int s16 = 0;
      for (int g = 0; g < rt.n_g16; ++g) {
        s16 += rt.g16_n[g];
        CHECK(rt.g16_q[g] >= 1 && rt.g16_q[g] <= kBand16MaxQ && (g == 0 || rt.g16_q[g] > rt.g16_q[g - 1]),
              "band16 group widths not increasing in 1..%d", kBand16MaxQ);
      }
      CHECK(s16 == rt.n16, "band16 group sizes %d vs n16 %d", s16, rt.n16);
      CHECK(rt.n_fused1 <= rt.n_fused - rt.n16, "fused p<=1 count");
      // segment checks
      int pos = rt.n_dense + rt.n_band;
      for (int g = 0; g < rt.n_g16; ++g)
        for (int i = 0; i < rt.g16_n[g]; ++i, ++pos) {
          const int b = rt.order[pos];
          const double* th = theta.data() + (size_t)b * GPX_THETA_STRIDE;
          const int w16 = band_width16(&bt, b, th);
          CHECK(bandp[b] == rt.g16_q[g] && std::max(w16, 1) == rt.g16_q[g] && band_width(&bt, b, th) <= 2,
                "band16 problem %d: h_bandp %d, group Q %d, width16 %d", b, bandp[b], rt.g16_q[g], w16);
          ++band16_routed;
        }
      for (int i = 0; i < rt.n_fused - rt.n16; ++i, ++pos) {
        const int b = rt.order[pos];
        const int p = band_width(&bt, b, theta.data() + (size_t)b * GPX_THETA_STRIDE);
        CHECK(bandp[b] == p && p <= 2 && ((i < rt.n_fused1) == (p <= 1)), "fused problem %d: p %d bandp %d", b, p,
              bandp[b]);
      }
      // gpx_batch_band_class (the drivers' class query) agrees with the routing
      {
        std::vector<int32_t> cls(active.size());
        CHECK(gpx_batch_band_class(&bt, (int)active.size(), active.data(), theta.data(), cls.data()) == GPX_OK,
              "gpx_batch_band_class failed");
        const int q16lim = route_limits(&bt).q16lim;
        for (size_t i = 0; i < active.size(); ++i) {
          const int b = active[i];
          const auto at = std::find(rt.order.begin(), rt.order.end(), b) - rt.order.begin();
          const double* th = theta.data() + (size_t)b * GPX_THETA_STRIDE;
          int want;
          if (at >= (long)rt.order.size() || at < rt.n_dense) {
            want = -1;  // dense, or band storage's fallback slots
          } else if (at < rt.n_dense + rt.n_band || at >= rt.n_dense + rt.n_band + rt.n16) {
            want = (q16lim > 0 ? 32 : 16) + band_width(&bt, b, th);
          } else {
            want = bandp[b];
          }
          CHECK(cls[i] == want, "round %d env %d problem %d: band_class %d, routed as %d", round, v, b, cls[i], want);
        }
      }
      if (v == 1) CHECK(rt.n16 == 0, "GPX_BAND16=0 still routed %d problems to band16", rt.n16);
      if (v == 3) CHECK(rt.n16 + rt.n_band + rt.n_fused == 0 || bt.compact == 0 ? rt.n_band + rt.n_fused == 0 : true,
                        "GPX_BAND=0 still routed banded problems");
      routed += (long long)active.size();
    }
    unsetenv("GPX_BAND");
    unsetenv("GPX_BAND16");
    unsetenv("GPX_BAND_FUSED");
    bt.h_bandp = nullptr;
  }
  std::printf("pairs checked %lld, tight band16 widths %lld, problems routed %lld (band16 %lld), failures %d\n",
              checked_pairs, tight_checked, routed, band16_routed, g_fail);
  if (g_fail) return 1;
  std::printf("OK\n");
  return 0;
}
