// gpx_reduce.h — wave and block reductions shared by the SVGP / SGPR element kernels
// (gpx_svgp_kernels.hip) and the SVGP per-point route (gpx_svgp_lik_kernels.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "gpx_internal.h"

namespace gpx {

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline int theta_slot(const DevSpec* gs, int p) {
  // θ index p -> (term, q) slot t*3+q of the per-term derivative sums, or -1
  for (int t = 0; t < gs->n_terms; ++t) {
    const int o = gs->terms[t].param_offset, kind = gs->terms[t].kind;
    const int np = (kind == GPX_RQ || kind == GPX_PERIODIC_SE) ? 3 : (kind == GPX_LINEAR ? 1 : 2);
    if (p >= o && p < o + np) return t * 3 + (p - o);
  }
  return -1;
}

// Block reduction of the per-lane sums[4][3] into out[16] (θ layout).
template <int NT>
__device__ void reduce_theta(double (&sums)[NT][3], const DevSpec* gs, double* sred, double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < GPX_MAX_TERMS; ++t)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v = t < NT ? wsum(sums[t < NT ? t : 0][q]) : 0.0;
      if (lane == 0) sred[wave * 16 + t * 3 + q] = v;
    }
  __syncthreads();
  if (threadIdx.x < GPX_THETA_STRIDE) {
    const int slot = theta_slot(gs, threadIdx.x);
    out[threadIdx.x] = slot >= 0 ? sred[slot] + sred[16 + slot] + sred[32 + slot] + sred[48 + slot] : 0.0;
  }
}

}  // namespace gpx
