// gpx_kfun_coreg.h — device functions of specs with a Coregion term (GPX_COREGION, include/gpx.h):
// gpflow.kernels.Coregion, K(x, x') = B[a, b] with a / b the integer output index read from one
// input column and B = W Wᵀ + diag(κ). Only the dense route's Coregion kernels include this: the K
// build and k** of gpx_coregion.hip and the EPI_CONTRACT_COREG epilogue of the fused K⁻¹ = WᵀW
// GEMM (gpx_kernels.hip). The isotropic and ARD functions (gpx_kfun.h, gpx_kfun_ard.h) are called,
// not changed: a partner term's value has the bits it has in an ARD or isotropic spec.
//
// θ layout of the term: [W row-major (P·R), κ (P)] at param_offset; P | R << 8 in the spec's
// `reserved`. W is signed (any finite value), κ > 0. A spec holds at most one Coregion term, alone
// or as one factor of a product.
// Derivatives per entry, a = a_i, b = b_j:  ∂K/∂W_pr = [a=p]·W_br + [b=p]·W_ar,  ∂K/∂κ_p = [a=p][b=p],
// each times the partner terms' values.
#pragma once
#include <hip/hip_runtime.h>
#include "gpx_kfun_ard.h"

namespace gpx {

constexpr int kCoregMaxP = 7;  // (P·(R + 1) + 1 <= GPX_THETA_STRIDE − 1 with R >= 1)
// meaning words of the Coregion θ slots (the partners' slots keep ard_slot_meta's words, < 1 << 23)
constexpr int kCoregSlotW = 1 << 28, kCoregSlotK = 1 << 29;

__device__ __forceinline__ bool cg_is(const gpx_term& t) { return t.kind == GPX_COREGION; }
__device__ __forceinline__ int cg_P(const DevSpec& s) { return s.reserved & 0xff; }
__device__ __forceinline__ int cg_R(const DevSpec& s) { return (s.reserved >> 8) & 0xff; }
// a partner term whose rows are staged over its ℓ (the stationary kinds)
__device__ __forceinline__ bool cg_prescaled(const gpx_term& t) { return !cg_is(t) && ard_prescaled(t); }
// a partner term that reads the raw rows (Linear, Periodic)
__device__ __forceinline__ bool cg_raw(const gpx_term& t) { return !cg_is(t) && !ard_prescaled(t); }

// the output index of a row: the index column's value as an int, clamped to [0, P − 1] (a value
// that is no valid index — the Python surface refuses those — never reads outside B; NaN reads 0)
__device__ __forceinline__ int cg_index(double x, int P) {
  return x >= 1.0 ? (x < (double)P ? (int)x : P - 1) : 0;
}

// B[p][q] = Σ_r W_pr W_qr (+ κ_p on the diagonal), th at the term's first slot; sums in r order
__device__ __forceinline__ double cg_b(const double* __restrict__ th, int P, int R, int p, int q) {
  double s = 0.0;
  for (int r = 0; r < R; ++r) s = fma(th[p * R + r], th[q * R + r], s);
  if (p == q) s += th[P * R + p];
  return s;
}

// K(xi, xj) of a spec with a Coregion term: ard_eval_k's partner terms times sB[a][b]
// (sB: [kCoregMaxP][kCoregMaxP]); a / b the clamped output indices of the two rows
__device__ __forceinline__ double cg_eval_k(const DevSpec& s, const double* __restrict__ th,
                                            const double* __restrict__ xi, const double* __restrict__ xj,
                                            const double* __restrict__ sxs, const int* __restrict__ soff,
                                            int i, int j, const double* __restrict__ sB, int a, int b) {
  const bool prod = (s.combine == GPX_PRODUCT && s.n_terms > 1);
  double acc = prod ? 1.0 : 0.0;
#pragma unroll
  for (int t = 0; t < GPX_MAX_TERMS; ++t) {
    if (t >= s.n_terms) break;
    const gpx_term& tm = s.terms[t];
    double v;
    if (cg_is(tm)) {
      v = sB[a * kCoregMaxP + b];
    } else if (ard_prescaled(tm)) {
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

// K_diag(x): the partners' K_diag (ard_eval_kdiag's values) times B[a][a]
__device__ __forceinline__ double cg_eval_kdiag(const DevSpec& s, const double* __restrict__ th,
                                                const double* __restrict__ x) {
  const bool prod = (s.combine == GPX_PRODUCT && s.n_terms > 1);
  const int P = cg_P(s), R = cg_R(s);
  double acc = prod ? 1.0 : 0.0;
  for (int t = 0; t < s.n_terms; ++t) {
    const gpx_term& tm = s.terms[t];
    double v;
    if (cg_is(tm)) {
      const int a = cg_index(x[tm.dim_start], P);
      v = cg_b(th + tm.param_offset, P, R, a, a);
    } else if (tm.kind == GPX_LINEAR) {
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

// what θ slot p holds: a partner's slot as ard_slot_meta packs it; a W slot kCoregSlotW | p' | r << 4
// (W_p'r), a κ slot kCoregSlotK | p'. −1: no kernel parameter.
__device__ __forceinline__ int cg_slot_meta(const DevSpec& s, const int (&soff)[GPX_MAX_TERMS], int p) {
  int m = -1;
  const int P = cg_P(s), R = cg_R(s);
#pragma unroll
  for (int t = 0; t < GPX_MAX_TERMS; ++t) {
    if (t >= s.n_terms) break;
    const gpx_term& tm = s.terms[t];
    const int o = tm.param_offset;
    if (cg_is(tm)) {
      if (p >= o && p < o + P * R) {
        const int pp = (p - o) / R;
        m = kCoregSlotW | pp | ((p - o - pp * R) << 4);
      } else if (p >= o + P * R && p < o + P * R + P) {
        m = kCoregSlotK | (p - o - P * R);
      }
      continue;
    }
    const int np = ard_nparams(tm);
    if (p < o || p >= o + np) continue;
    if (!ard_on(tm)) {
      m = t | ((p - o) << 2);
    } else {
      const int e = ard_ell_slot(tm), dn = tm.dim_count;
      const int rq = ard_kind(tm) == GPX_RQ ? 1 : 0;
      if (p < e) m = t;
      else if (p < e + dn) m = t | (rq << 2) | 16 | (dn << 5) | ((soff[t] + (p - e)) << 10);
      else m = t | ((rq + 1) << 2);
    }
  }
  return m;
}

// The gradient contraction of a Coregion spec over one lower tile of K⁻¹ = WᵀW, the epilogue of
// gemm_kernel<BM, true, false, EPI_CONTRACT_COREG>: ard_contract_tile's structure (per-lane
// θ-indexed sums, a wave-uniform meaning word per slot, wave then block reduction, no atomics)
// with the Coregion term's B[a][b] among the values and its W / κ slots among the sums: per entry
// and slot two selects and one multiply-add on v·Π(partner values).
// smem: 4·16·WT + 2·BM·GPX_MAX_DIM + 2·BM + GPX_THETA_STRIDE + 64 doubles (gemm_kernel's kEpiLds);
// the rows' output indices take one column of the staging area (staged + raw + 1 <= GPX_MAX_DIM,
// refused at create / rebind otherwise), B the block-reduction area until the sums are final.
template <int BM, int MT>
__device__ __forceinline__ void cg_contract_tile(const double* __restrict__ X, const double* __restrict__ al,
                                                 const double* __restrict__ theta, const DevSpec* gs,
                                                 int D, int n, int i0, int j0, ard_d4 (&acc)[MT][MT],
                                                 double* __restrict__ smem, double* __restrict__ out) {
  constexpr int BN = BM, WT = BM / 2, NT = GPX_MAX_TERMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const DevSpec spec = *gs;
  const int P = cg_P(spec), R = cg_R(spec);
  int soff[NT];
  int S = 0, tc = -1, icol = 0, woff = 0;
  bool raw = false;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    soff[t] = 0;
    if (t >= spec.n_terms) continue;
    if (cg_is(spec.terms[t])) {
      tc = t;
      icol = spec.terms[t].dim_start;
      woff = spec.terms[t].param_offset;
    } else if (ard_prescaled(spec.terms[t])) {
      soff[t] = (BM + BN) * S;
      S += spec.terms[t].dim_count;
    } else {
      raw = true;
    }
  }
  const int Dr = raw ? D : 0;
  double* sacc = smem;                      // [4 waves][16][WT]
  double* sxp = sacc + 4 * 16 * WT;         // term t's x/ℓ at soff[t]: [BM + BN][its dims]
  double* sxr = sxp + (BM + BN) * S;        // [BM + BN][Dr] raw rows
  int* sidx = reinterpret_cast<int*>(sxr + (BM + BN) * Dr);  // [BM + BN] output indices
  double* sai = sacc + 4 * 16 * WT + 2 * BM * GPX_MAX_DIM;   // [BM]
  double* saj = sai + BM;                   // [BN]
  double* sth = saj + BN;                   // [16]
  double* sred = sth + GPX_THETA_STRIDE;    // [4 waves][16]; B [P][kCoregMaxP] until the reduction
  __syncthreads();
  if (S + Dr + 1 > GPX_MAX_DIM || tc < 0 || P < 1 || P > kCoregMaxP || R < 1 ||
      woff + P * R + P > spec.n_params) {  // (refused at create / rebind: never launched)
    if (tid < GPX_THETA_STRIDE) out[tid] = 0.0;
    return;
  }
  if (tid < BM) { sai[tid] = al[i0 + tid]; saj[tid] = al[j0 + tid]; }
  if (tid < GPX_THETA_STRIDE) sth[tid] = theta[tid];
  if (tid < P * kCoregMaxP) {
    const int p = tid / kCoregMaxP, q = tid - p * kCoregMaxP;
    sred[tid] = q < P ? cg_b(theta + woff, P, R, p, q) : 0.0;
  }
  for (int r = tid; r < BM; r += 256) {
    sidx[r] = (i0 + r < n) ? cg_index(X[(long long)(i0 + r) * D + icol], P) : 0;
    sidx[BM + r] = (j0 + r < n) ? cg_index(X[(long long)(j0 + r) * D + icol], P) : 0;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= spec.n_terms || !cg_prescaled(spec.terms[t])) continue;
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
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) meta[p] = cg_slot_meta(spec, soff, p);
  double sums[GPX_THETA_STRIDE];
#pragma unroll
  for (int p = 0; p < GPX_THETA_STRIDE; ++p) sums[p] = 0.0;
  double snoise = 0.0;
  const bool prod = (spec.combine == GPX_PRODUCT && spec.n_terms > 1);
  const double* sW = sth + woff;
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
      const int jb = sidx[BM + jl];
#pragma unroll 1
      for (int rr = rg; rr < 16; rr += RG) {
        const int il = wr * WT + h * 16 + rr;
        const int i = i0 + il;
        if (i >= j && i < n) {
          const double w = (i == j) ? 1.0 : 2.0;
          const double v = w * fma(sai[il], aj, -wacc[rr * WT + cl]);
          const int ia = sidx[il];
          double dk[NT][3], vals[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            dk[t][0] = dk[t][1] = dk[t][2] = 0.0;
            vals[t] = 1.0;
            if (t >= spec.n_terms) continue;
            const gpx_term& tm = spec.terms[t];
            const int dn = tm.dim_count;
            if (cg_is(tm)) {
              vals[t] = sred[ia * kCoregMaxP + jb];
            } else if (!ard_prescaled(tm)) {
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
          double vc = v;  // v · Π(partner values): the Coregion slots' common factor
          if (prod) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              double others = 1.0;
#pragma unroll
              for (int u = 0; u < NT; ++u) if (u != t) others *= vals[u];
              dk[t][0] *= others; dk[t][1] *= others; dk[t][2] *= others;
              if (t == tc) vc = v * others;
            }
          }
#pragma unroll
          for (int p = 0; p < GPX_THETA_STRIDE; ++p) {
            const int m = meta[p];
            if (m < 0) continue;
            if (m & (kCoregSlotW | kCoregSlotK)) {
              const int pp = m & 15;
              double f;
              if (m & kCoregSlotK) {
                f = (ia == pp && jb == pp) ? 1.0 : 0.0;
              } else {
                const int r = (m >> 4) & 15;
                f = (ia == pp ? sW[jb * R + r] : 0.0) + (jb == pp ? sW[ia * R + r] : 0.0);
              }
              sums[p] = fma(vc, f, sums[p]);
              continue;
            }
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
      if (!cg_is(tm) && ard_on(tm) && tid >= e && tid < e + tm.dim_count) s = s / sth[tid];
    }
    out[tid] = s;
  }
}

}  // namespace gpx
