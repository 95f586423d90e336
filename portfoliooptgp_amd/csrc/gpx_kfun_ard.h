// gpx_kfun_ard.h — device functions of the ARD (one lengthscale per active dimension) stationary
// terms, GPX_TERM_ARD in gpx_term.kind (include/gpx.h). Only the dense route's ARD kernels include
// this: the K build and k** of gpx_ard.hip and the ARD contraction epilogue of the fused K⁻¹ = WᵀW
// GEMM (gpx_kernels.hip). The isotropic functions of gpx_kfun.h are not touched.
//
// θ layout of an ARD term over dn active dims: [ℓ_0 … ℓ_{dn−1}, σ²] (RQ: [α, ℓ_0 … ℓ_{dn−1}, σ²]).
// Arithmetic as GPflow's Stationary with a vector lengthscale: a_d = x_d / ℓ_d (a division), then
// r² = −2·Σ a_d b_d + (Σ a_d² + Σ b_d²) on the scaled rows (sqdist_scaled: contraction off, sums
// in d order) — the rows are staged scaled in LDS once per tile, so at ℓ_d = ℓ the values are the
// isotropic term's bit for bit (the value formulas are eval_term's own, called on the scaled rows).
// Derivatives: ∂K/∂ℓ_d = σ²·g'(r²)·(−2)·(a_d − b_d)²/ℓ_d = c·(a_d − b_d)²/ℓ_d with one coefficient c
// per entry (SE: σ² g; RQ: σ² g/b; K_r kinds: −σ² g'(r)/r, zero where the 1e-36 clamp is active).
#pragma once
#include <hip/hip_runtime.h>
#include "gpx_kfun.h"

namespace gpx {

typedef double ard_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_sum_ard(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int ard_kind(const gpx_term& t) { return t.kind & GPX_TERM_KIND_MASK; }
__device__ __forceinline__ bool ard_on(const gpx_term& t) { return (t.kind & GPX_TERM_ARD) != 0; }
// the stationary kinds (inputs staged over their ℓ); Linear and Periodic read X itself
__device__ __forceinline__ bool ard_prescaled(const gpx_term& t) { return term_prescaled(ard_kind(t)); }
// θ slots of a term: its first ℓ, the number of ℓ entries, its σ², and its parameter count
__device__ __forceinline__ int ard_ell_slot(const gpx_term& t) {
  return t.param_offset + (ard_kind(t) == GPX_RQ ? 1 : 0);
}
__device__ __forceinline__ int ard_nell(const gpx_term& t) { return ard_on(t) ? t.dim_count : 1; }
__device__ __forceinline__ int ard_nparams(const gpx_term& t) {
  return ard_on(t) ? term_nparams(ard_kind(t)) - 1 + t.dim_count : term_nparams(t.kind);
}

// the term as eval_term reads it on pre-scaled rows: its kind without the flag and a θ triple in
// the isotropic order (the ℓ entry is not read on scaled rows)
struct ArdIso {
  gpx_term t;
  double th[3];
};
__device__ __forceinline__ ArdIso ard_iso(const gpx_term& t, const double* __restrict__ th /* the row */) {
  ArdIso r;
  r.t = t;
  r.t.kind = ard_kind(t);
  r.t.param_offset = 0;
  const int e = ard_ell_slot(t), v = e + ard_nell(t);
  if (r.t.kind == GPX_RQ) { r.th[0] = th[t.param_offset]; r.th[1] = th[e]; r.th[2] = th[v]; }
  else { r.th[0] = th[e]; r.th[1] = th[v]; r.th[2] = 0.0; }
  return r;
}

// K(xi, xj) of a spec with ARD terms. xi / xj: the raw rows (read by Linear / Periodic terms only);
// sxs + soff[t]: term t's scaled rows, [rows][dim_count], i / j the row indices into them.
__device__ __forceinline__ double ard_eval_k(const DevSpec& s, const double* __restrict__ th,
                                             const double* __restrict__ xi, const double* __restrict__ xj,
                                             const double* __restrict__ sxs, const int* __restrict__ soff,
                                             int i, int j) {
  const bool prod = (s.combine == GPX_PRODUCT && s.n_terms > 1);
  double acc = prod ? 1.0 : 0.0;
#pragma unroll
  for (int t = 0; t < GPX_MAX_TERMS; ++t) {
    if (t >= s.n_terms) break;
    const gpx_term& tm = s.terms[t];
    double v;
    if (ard_prescaled(tm)) {
      const ArdIso q = ard_iso(tm, th);
      const int dn = tm.dim_count;
      v = eval_term<false>(q.t, q.th, xi, xj, nullptr, sxs + soff[t] + i * dn, sxs + soff[t] + j * dn);
    } else {
      v = eval_term<false>(tm, th + tm.param_offset, xi, xj, nullptr);
    }
    if (prod) acc *= v; else acc += v;
  }
  return acc;
}

// value and derivatives of one ARD term at r² (on its scaled rows), in eval_term's dk order with
// the ℓ entry holding the coefficient c of ∂K/∂ℓ_d = c·(a_d − b_d)²/ℓ_d
__device__ __forceinline__ double ard_term_grad(int kind, double r2, const double (&th)[3], double (&dk)[3]) {
  dk[2] = 0.0;
  if (kind == GPX_SE) {
    const double var = th[1], g = exp(-0.5 * r2);
    dk[0] = var * g;
    dk[1] = g;
    return var * g;
  }
  if (kind == GPX_RQ) {
    const double a = th[0], var = th[2];
    const double b = 1.0 + 0.5 * r2 / a;
    const double lb = log(b);
    const double g = exp(-a * lb);
    dk[0] = var * g * (-lb + 0.5 * r2 / (a * b));
    dk[1] = var * (g / b);
    dk[2] = g;
    return var * g;
  }
  const double var = th[1];
  const bool clamped = !(r2 > 1e-36);
  const double r = sqrt(clamped ? 1e-36 : r2);
  double g, dgdr;
  if (kind == GPX_MATERN12) {
    g = exp(-r); dgdr = -g;
  } else if (kind == GPX_EXPONENTIAL) {
    g = exp(-0.5 * r); dgdr = -0.5 * g;
  } else if (kind == GPX_MATERN32) {
    const double sq3 = 1.7320508075688772, e = exp(-sq3 * r);
    g = (1.0 + sq3 * r) * e; dgdr = -3.0 * r * e;
  } else {
    const double sq5 = 2.23606797749979, e = exp(-sq5 * r);
    g = (1.0 + sq5 * r + (5.0 / 3.0) * r * r) * e;
    dgdr = -(5.0 / 3.0) * r * (1.0 + sq5 * r) * e;
  }
  dk[0] = clamped ? 0.0 : -var * dgdr / r;
  dk[1] = g;
  return var * g;
}

// what θ slot p of a spec holds, packed: bits 0-1 the term, 2-3 the entry q of that term's dk[],
// bit 4: an ARD ℓ_d (the entry is the coefficient: times (a_d − b_d)²), bits 5-9 the term's
// dim_count, bits 10.. the offset of a_d in the scaled rows (soff[t] + d). −1: no kernel parameter.
template <int NT>
__device__ __forceinline__ int ard_slot_meta(const DevSpec& s, const int (&soff)[NT], int p) {
  int m = -1;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= s.n_terms) break;
    const gpx_term& tm = s.terms[t];
    const int o = tm.param_offset, np = ard_nparams(tm);
    if (p < o || p >= o + np) continue;
    if (!ard_on(tm)) {
      m = t | ((p - o) << 2);
    } else {
      const int e = ard_ell_slot(tm), dn = tm.dim_count;
      const int rq = ard_kind(tm) == GPX_RQ ? 1 : 0;
      if (p < e) m = t;                                        // RQ's α
      else if (p < e + dn) m = t | (rq << 2) | 16 | (dn << 5) | ((soff[t] + (p - e)) << 10);
      else m = t | ((rq + 1) << 2);                            // σ²
    }
  }
  return m;
}

// The ARD gradient contraction over one lower tile of K⁻¹ = WᵀW (acc = K⁻¹_ij of this wave's
// quadrant), the epilogue of gemm_kernel<BM, true, false, EPI_CONTRACT_ARD*>:
//   g_θ += w_ij (α_i α_j − K⁻¹_ij) ∂K_ij/∂θ,  w = 2 below the diagonal, 1 on it,
// accumulated per lane straight into θ-indexed sums (statically indexed: the slot loop is unrolled
// and each slot's meaning is a wave-uniform word), the ARD slots without their 1/ℓ_d, which is
// applied once to the tile's total. Writes out[0..15] per tile as the isotropic epilogue does.
// smem: 4·16·WT + 2·BM·GPX_MAX_DIM + 2·BM + GPX_THETA_STRIDE + 64 doubles.
template <int BM, int NT, int MT>
__device__ __forceinline__ void ard_contract_tile(const double* __restrict__ X, const double* __restrict__ al,
                                                  const double* __restrict__ theta, const DevSpec* gs,
                                                  int D, int n, int i0, int j0, ard_d4 (&acc)[MT][MT],
                                                  double* __restrict__ smem, double* __restrict__ out) {
  constexpr int BN = BM, WT = BM / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const DevSpec spec = *gs;
  // the scaled rows of the stationary terms, then (for Linear / Periodic terms) the raw rows
  int soff[NT];
  int P = 0;
  bool raw = false;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    soff[t] = 0;
    if (t >= spec.n_terms) continue;
    if (ard_prescaled(spec.terms[t])) {
      soff[t] = (BM + BN) * P;
      P += spec.terms[t].dim_count;
    } else {
      raw = true;
    }
  }
  const int Dr = raw ? D : 0;
  double* sacc = smem;                      // [4 waves][16][WT]
  double* sxp = sacc + 4 * 16 * WT;         // term t's x/ℓ at soff[t]: [BM + BN][its dims]
  double* sxr = sxp + (BM + BN) * P;        // [BM + BN][Dr] raw rows
  double* sai = sacc + 4 * 16 * WT + 2 * BM * GPX_MAX_DIM;  // [BM]
  double* saj = sai + BM;                   // [BN]
  double* sth = saj + BN;                   // [16]
  double* sred = sth + GPX_THETA_STRIDE;    // [4 waves][16]
  __syncthreads();
  if (P + Dr > GPX_MAX_DIM || spec.n_terms > NT) {  // (refused at create / rebind: never launched)
    if (tid < GPX_THETA_STRIDE) out[tid] = 0.0;
    return;
  }
  if (tid < BM) { sai[tid] = al[i0 + tid]; saj[tid] = al[j0 + tid]; }
  if (tid < GPX_THETA_STRIDE) sth[tid] = theta[tid];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= spec.n_terms || !ard_prescaled(spec.terms[t])) continue;
    const gpx_term& tm = spec.terms[t];
    const int dn = tm.dim_count, e0 = ard_ell_slot(tm);
    const bool vec = ard_on(tm);
    for (int e = tid; e < BM * dn; e += 256) {
      const int r = e / dn, dd = e - r * dn;
      const double ell = theta[e0 + (vec ? dd : 0)];
      const int d = tm.dim_start + dd;
      sxp[soff[t] + e] = ((i0 + r < n) ? X[(long long)(i0 + r) * D + d] : 0.0) / ell;
      sxp[soff[t] + BM * dn + e] = ((j0 + r < n) ? X[(long long)(j0 + r) * D + d] : 0.0) / ell;
    }
  }
  for (int e = tid; e < BM * Dr; e += 256) {
    const int r = e / Dr;
    sxr[e] = (i0 + r < n) ? X[(long long)(i0 + r) * D + (e - r * Dr)] : 0.0;
    sxr[BM * Dr + e] = (j0 + r < n) ? X[(long long)(j0 + r) * D + (e - r * Dr)] : 0.0;
  }
  int meta[GPX_THETA_STRIDE];
#pragma unroll
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) meta[p] = ard_slot_meta<NT>(spec, soff, p);
  double sums[GPX_THETA_STRIDE];
#pragma unroll
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) sums[p] = 0.0;
  double snoise = 0.0;
  const bool prod = (NT > 1 && spec.combine == GPX_PRODUCT && spec.n_terms > 1);
  constexpr int RG = 64 / WT;
  double* wacc = sacc + wave * (16 * WT);
  const int cl = lane % WT, rg = lane / WT;
  const int jl = wc * WT + cl;            // this lane's column within the tile
  const int j = j0 + jl;
#pragma unroll
  for (int h = 0; h < MT; ++h) {
#pragma unroll
    for (int nn = 0; nn < MT; ++nn)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        wacc[((lane >> 4) + 4 * r) * WT + nn * 16 + (lane & 15)] = acc[h][nn][r];
    __syncthreads();
    if (j < n) {
      const double aj = saj[jl];
#pragma unroll 1
      for (int rr = rg; rr < 16; rr += RG) {
        const int il = wr * WT + h * 16 + rr;
        const int i = i0 + il;
        if (i >= j && i < n) {
          const double w = (i == j) ? 1.0 : 2.0;
          const double v = w * fma(sai[il], aj, -wacc[rr * WT + cl]);
          double dk[NT][3], vals[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            dk[t][0] = dk[t][1] = dk[t][2] = 0.0;
            vals[t] = 1.0;
            if (t >= spec.n_terms) continue;
            const gpx_term& tm = spec.terms[t];
            const int dn = tm.dim_count;
            if (!ard_prescaled(tm)) {
              vals[t] = eval_term<true>(tm, sth + tm.param_offset, sxr + il * Dr, sxr + (BM + jl) * Dr, dk[t]);
            } else if (!ard_on(tm)) {
              vals[t] = eval_term<true>(tm, sth + tm.param_offset, nullptr, nullptr, dk[t],
                                        sxp + soff[t] + il * dn, sxp + soff[t] + (BM + jl) * dn);
            } else {
              const ArdIso q = ard_iso(tm, sth);
              const double r2 = sqdist_scaled(sxp + soff[t] + il * dn, sxp + soff[t] + (BM + jl) * dn, dn);
              vals[t] = ard_term_grad(q.t.kind, r2, q.th, dk[t]);
            }
          }
          if (prod) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              double others = 1.0;
#pragma unroll
              for (int u = 0; u < NT; ++u) if (u != t) others *= vals[u];
              dk[t][0] *= others; dk[t][1] *= others; dk[t][2] *= others;
            }
          }
#pragma unroll
          for (int p = 0; p < GPX_THETA_STRIDE; ++p) {
            const int m = meta[p];
            if (m < 0) continue;
            double f = 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
              for (int q = 0; q < 3; ++q)
                if ((m & 15) == (t | (q << 2))) f = dk[t][q];
            if (m & 16) {
              const int dn = (m >> 5) & 31, o = m >> 10;
              const double df = sxp[o + il * dn] - sxp[o + (BM + jl) * dn];
              f *= df * df;
            }
            sums[p] = fma(v, f, sums[p]);
          }
          if (i == j) snoise += v;
        }
      }
    }
    __syncthreads();
  }
  // block reduction: wave sums (σn²'s in its own θ slot), then the four waves in turn
  snoise = wave_sum_ard(snoise);
#pragma unroll
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) {
    const double sv = wave_sum_ard(sums[p]);
    if (lane == 0) sred[wave * 16 + p] = (p == spec.n_params) ? snoise : sv;
  }
  __syncthreads();
  if (tid < GPX_THETA_STRIDE) {
    double s = 0.0;
    if (tid <= spec.n_params) s = sred[tid] + sred[16 + tid] + sred[32 + tid] + sred[48 + tid];
    // an ARD ℓ_d's slot: the 1/ℓ_d left out of every entry
    for (int t = 0; t < gs->n_terms; ++t) {
      const gpx_term& tm = gs->terms[t];
      const int e = ard_ell_slot(tm);
      if (ard_on(tm) && tid >= e && tid < e + tm.dim_count) s = s / sth[tid];
    }
    out[tid] = s;
  }
}

// K_diag(x) with ARD terms: eval_kdiag's, the σ² of an ARD term read at its own slot
__device__ __forceinline__ double ard_eval_kdiag(const DevSpec& s, const double* __restrict__ th,
                                                 const double* __restrict__ x) {
  const bool prod = (s.combine == GPX_PRODUCT && s.n_terms > 1);
  double acc = prod ? 1.0 : 0.0;
  for (int t = 0; t < s.n_terms; ++t) {
    const gpx_term& tm = s.terms[t];
    double v;
    if (tm.kind == GPX_LINEAR) {
#pragma clang fp contract(off)
      const double var = th[tm.param_offset];
      v = (x[tm.dim_start] * x[tm.dim_start]) * var;
      for (int d = 1; d < tm.dim_count; ++d) v = v + (x[tm.dim_start + d] * x[tm.dim_start + d]) * var;
    } else if (tm.kind == GPX_PERIODIC_SE) {
      v = th[tm.param_offset + 1];
    } else {
      v = th[ard_ell_slot(tm) + ard_nell(tm)];
    }
    if (prod) acc *= v; else acc += v;
  }
  return acc;
}

}  // namespace gpx
