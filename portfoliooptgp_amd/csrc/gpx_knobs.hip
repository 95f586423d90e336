// gpx_knobs.hip — the knob table of gpx_knobs.h, its accessors and the rules derived from the
// knobs. Host code only. The one file of csrc/ that reads GPX_ variables from the environment.
#include <algorithm>
#include <cstdlib>
#include "gpx_host.h"

namespace gpx {

static_assert(kGroups == 4 && 1 + kAux == 4 && kBand16MaxQ == 8,
              "the limits of GPX_GROUPS, GPX_BAND_LANE_STREAMS and GPX_BAND16_QMAX in gpx_knobs.h");

const KnobDef kKnobs[(int)Knob::kCount] = {
#define GPX_KNOB_ROW(id, name, type, read, def, lo, hi, meaning) \
  {name, KnobType::type, KnobRead::read, (double)(def), lo, hi, meaning},
    GPX_KNOB_TABLE(GPX_KNOB_ROW)
#undef GPX_KNOB_ROW
};

double knob_parse(const KnobDef& d, const char* text) {
  if (!text) return d.def;
  switch (d.type) {
    case KnobType::Flag: return atoi(text) != 0 ? 1.0 : 0.0;
    case KnobType::Mask: return (double)(atoi(text) & d.hi);
    case KnobType::Real: return atof(text);
    default: return (double)std::max(d.lo, std::min(d.hi, atoi(text)));
  }
}

namespace {
struct OnceValues {
  double v[(int)Knob::kCount];
  OnceValues() {
    for (int k = 0; k < (int)Knob::kCount; ++k)
      v[k] = kKnobs[k].read == KnobRead::Once ? knob_parse(kKnobs[k], getenv(kKnobs[k].name)) : 0.0;
  }
};
}  // namespace

double knob_value(Knob k) {
  const KnobDef& d = kKnobs[(int)k];
  if (d.read == KnobRead::PerCall) return knob_parse(d, getenv(d.name));
  static const OnceValues once;
  return once.v[(int)k];
}

// which SE1 band16 sweeps compute their K tiles from X (bit 0: forward, bit 1: backward): a sweep
// that does not reads K's band. Same bits every way. Default: both (round 4: +4-7 % on the C2
// bench, K's band never in HBM)
int b16_inline_k() { return knob_int(Knob::B16InlineK); }

// the same for the wide launch of a deferred part (default: as above)
int b16_inline_k_wide() {
  const int kin = knob_int(Knob::B16InlineKWide);
  return kin == kKnobUnset ? b16_inline_k() : kin;
}

// the widest band16 class a deferred part's wide launch takes: 5, or 8 (GPX_WIDE_QMAX, default
// 8) for SE1 parts whose sweeps compute K inline
int wide_qmax(bool se1) { return (se1 && b16_inline_k_wide() == 3) ? knob_int(Knob::WideQmax) : 5; }

// band16 widths Q > kBcrMaxQ (6..8) by the block-cyclic-reduction chain of block size 128
// (gpx_bcr.hip bcrw_*; GPX_WIDE_BCR): 1 (default) in calls on the reduction route (the batch's
// band route "bcr": latency — before round 6 these widths went to the 64-row sweeps there),
// 2 in every call, 0 never. Measured in the C2 bench's layout (8 host processes, thousands of
// problems in flight) mode 2 loses 35 % with deferral and 12 % without (profiles/r06_ab.md: the
// chain's 8-wave, 150 KB-LDS workgroups wait for an empty CU behind the other processes' sweeps),
// so the sweeps route keeps its one-wavefront Q = 6..8 sweeps. Either way a problem's path is a
// function of its own width and the batch's route, never of the call.
int wide_bcr_mode() { return knob_int(Knob::WideBcr); }
bool wide_bcr_on(bool bcr_route) { return wide_bcr_mode() == 2 || (wide_bcr_mode() == 1 && bcr_route); }

// the widest class a deferred part's wide launch (band16_wide_kernel) takes (deferred parts
// exist on the sweeps route only)
int wide_launch_qmax(bool se1) { return wide_bcr_on(false) ? std::min(wide_qmax(se1), kBcrMaxQ) : wide_qmax(se1); }

// the most band16 problems a call may hold for them to take the block-cyclic-reduction path
// (gpx_bcr.hip) instead of the one-wavefront sweeps: the batch's route (gpx_batch_set_band_route:
// sweeps 0, BCR every call, AUTO 32), unless GPX_BCR_MAX is set, which overrides it for the
// whole process (read per call: a process can compare the paths)
int bcr_max_problems(int band_route) {
  const int e = knob_int(Knob::BcrMax);
  if (e != kKnobUnset) return e;
  switch (band_route) {
    case GPX_BAND_ROUTE_BCR: return 1 << 30;
    case GPX_BAND_ROUTE_AUTO: return 32;
    default: return 0;
  }
}

}  // namespace gpx
