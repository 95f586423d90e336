// gpx_knobs.h — every environment variable the library reads, in ONE table (definitions and the
// rules derived from them: gpx_knobs.hip). No other file of csrc/ calls getenv for a GPX_ name.
//
// A row: enum name, variable, type, when it is read, default, lower / upper limit, meaning.
//   Flag  unset: the default; set: atoi(text) != 0
//   Int   unset: the default; set: atoi(text) clamped to [lo, hi]
//   Mask  unset: the default; set: atoi(text) & hi
//   Real  unset: the default; set: atof(text)
//   Once     read at the process's first knob access and kept (tests use a child process)
//   PerCall  read from the environment at every access (tests flip these inside one process)
// A default of kKnobUnset means "derived when unset": see the rule named in the row's meaning.
#pragma once
#include <climits>

namespace gpx {

constexpr int kKnobUnset = INT_MIN;
constexpr int kKnobNoLo = INT_MIN, kKnobNoHi = INT_MAX;

#define GPX_KNOB_TABLE(X)                                                                                      \
  /* dense recursion and the small-problem kernels */                                                          \
  X(Leaf128, "GPX_LEAF128", Flag, Once, 1, 0, 1, "0: the recursion goes down to 64-leaves (no fused 128-node kernel)") \
  X(Small64, "GPX_SMALL64", Flag, Once, 1, 0, 1, "0: Np = 64 batches run the six-launch chain, not small64_kernel")     \
  X(Small128, "GPX_SMALL128", Flag, Once, 1, 0, 1, "0: the same for Np = 128 (small128_kernel)")                       \
  X(SmallDirect, "GPX_SMALL_DIRECT", Flag, Once, 1, 0, 1, "0: a small-problem call's I/O through the DMA'd block, not coherent pinned memory") \
  X(SmallPoll, "GPX_SMALL_POLL", Flag, Once, 1, 0, 1, "0: such a call completes by a stream synchronise, not by polled flags")  \
  X(Groups, "GPX_GROUPS", Int, PerCall, 1, 1, 4, "dense problems split into this many concurrent pipelines (at most kGroups)") \
  X(ContractPriority, "GPX_CONTRACT_PRIORITY", Flag, Once, 0, 0, 1, "1: the dense contraction on a highest-priority stream") \
  /* routing */                                                                                                \
  X(Band, "GPX_BAND", Flag, PerCall, 1, 0, 1, "0: every problem takes the dense path")                         \
  X(BandPmax, "GPX_BAND_PMAX", Int, PerCall, -1, kKnobNoLo, kKnobNoHi, "widest band (64-blocks) the banded path takes; < 0: Np/256") \
  X(Band16, "GPX_BAND16", Flag, PerCall, 1, 0, 1, "0: no 16-row band sweeps (the 64-row sweeps take those problems)") \
  X(BandFused, "GPX_BAND_FUSED", Flag, PerCall, 1, 0, 1, "0: p <= 2 problems take the per-block launches too")  \
  X(Band16Qmax, "GPX_BAND16_QMAX", Int, PerCall, 8, kKnobNoLo, 8, "widest SE1 band16 class (16-blocks, at most kBand16MaxQ)") \
  X(BandTol, "GPX_BAND_TOL", Real, PerCall, 1e-6, 0, 0, "band-check tolerance; failing problems are redone densely") \
  X(BcrMax, "GPX_BCR_MAX", Int, PerCall, kKnobUnset, kKnobUnset + 1, kKnobNoHi,"most band16 problems of a call on the reduction path; unset: bcr_max_problems (the batch's route)") \
  /* band16 sweeps and the reduction chains */                                                                 \
  X(B16InlineK, "GPX_B16_INLINE_K", Mask, Once, 3, 0, 3, "SE1 sweeps computing K tiles from X: bit 0 forward, bit 1 backward") \
  X(B16InlineKWide, "GPX_B16_INLINE_K_WIDE", Mask, Once, kKnobUnset, 0, 3, "the same for a deferred part's wide launch; unset: b16_inline_k") \
  X(B16Fused, "GPX_B16_FUSED", Flag, Once, 0, 0, 1, "1: an SE1 class's two sweeps as one fused launch")          \
  X(WideQmax, "GPX_WIDE_QMAX", Int, Once, 8, 5, 8, "widest class of the wide launch for SE1 parts with K inline (wide_qmax)") \
  X(WideBcr, "GPX_WIDE_BCR", Int, Once, 1, 0, 2, "widths 6..8 by the block-128 reduction: 0 never, 1 on the reduction route, 2 always (wide_bcr_on)") \
  X(BcrGraph, "GPX_BCR_GRAPH", Flag, Once, 1, 0, 1, "0: the reduction chains launched directly, not replayed as HIP graphs") \
  /* lanes */                                                                                                  \
  X(LaneOrder, "GPX_LANE_ORDER", Int, Once, 0, kKnobNoLo, kKnobNoHi, "1: the small lanes are enqueued ahead of the bulk lane") \
  X(BandLanes, "GPX_BAND_LANES", Flag, Once, 1, 0, 1, "0: every width class one after another on the call's stream") \
  X(BandLaneStreams, "GPX_BAND_LANE_STREAMS", Int, Once, 4, 1, kKnobNoHi, "streams the lanes are spread over (default 1 + kAux)") \
  /* deferred slow parts */                                                                                    \
  X(DeferStream, "GPX_DEFER_STREAM", Flag, Once, 1, 0, 1, "0: a deferred part follows the call on the call's own stream") \
  X(DeferWide, "GPX_DEFER_WIDE", Flag, Once, 1, 0, 1, "0: a deferred part's band16 classes as per-class launches, not one wide launch") \
  X(DeferLanes, "GPX_DEFER_LANES", Flag, Once, 0, 0, 1, "1: a deferred part's lanes on the batch's lane streams")  \
  X(WideReverse, "GPX_WIDE_REVERSE", Flag, Once, 1, 0, 1, "0: the wide launch's waves in ascending width order")    \
  X(SlowDirect, "GPX_SLOW_DIRECT", Flag, Once, 0, 0, 1, "1: a deferred part's results gathered into coherent pinned memory") \
  X(SlowPriority, "GPX_SLOW_PRIORITY", Int, Once, 0, kKnobNoLo, kKnobNoHi, "slow stream priority: < 0 lowest, > 0 highest, 0 default") \
  X(SlowDelayUs, "GPX_SLOW_DELAY_US", Int, Once, 0, kKnobNoLo, kKnobNoHi, "> 0: a spin kernel of this many µs after each deferred part (experiments)") \
  /* host profiling */                                                                                         \
  X(SubmitStats, "GPX_SUBMIT_STATS", Flag, Once, 0, 0, 1, "1: wall-clock phase accumulators of submit / complete / predict")

enum class Knob : int {
#define GPX_KNOB_ENUM(id, name, type, read, def, lo, hi, meaning) id,
  GPX_KNOB_TABLE(GPX_KNOB_ENUM)
#undef GPX_KNOB_ENUM
  kCount
};

enum class KnobType { Flag, Int, Mask, Real };
enum class KnobRead { Once, PerCall };
struct KnobDef {
  const char* name;
  KnobType type;
  KnobRead read;
  double def;  // (an Int / Mask / Flag default is a whole number)
  int lo, hi;
  const char* meaning;
};
extern const KnobDef kKnobs[(int)Knob::kCount];

// the value `text` (nullptr: unset) gives the knob: default, clamp or mask applied. Pure.
double knob_parse(const KnobDef& d, const char* text);
// the knob's value now (PerCall: one getenv; Once: the process's cached value)
double knob_value(Knob k);
inline bool knob_on(Knob k) { return knob_value(k) != 0.0; }
inline int knob_int(Knob k) { return (int)knob_value(k); }
inline double knob_real(Knob k) { return knob_value(k); }

// ---- rules derived from the knobs ----
int b16_inline_k();                  // GPX_B16_INLINE_K (bit 0 forward, bit 1 backward)
int b16_inline_k_wide();             // ... for the wide launch (GPX_B16_INLINE_K_WIDE; unset: as above)
int wide_qmax(bool se1);             // widest class of the wide launch: 5, or GPX_WIDE_QMAX for SE1 with wide inline K
int wide_bcr_mode();                 // GPX_WIDE_BCR
bool wide_bcr_on(bool bcr_route);    // band16 widths Q > kBcrMaxQ by the block-128 reduction in this call
int wide_launch_qmax(bool se1);      // widest class a deferred part's wide launch takes
int bcr_max_problems(int band_route);  // GPX_BCR_MAX, else by the batch's route (GPX_BAND_ROUTE_*)

}  // namespace gpx
