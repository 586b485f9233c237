// sim_tile.h — the tiled exact-f32 similarity block shared by the fused softmax statistics (simce_tiled.hip) and
// the retrieval epilogues (retrieval.hip): one 64-key x 64-query block of S^T = Y X^T on v_mfma_f32_32x32x2_f32, keys
// on the MFMA rows and queries on the lanes.  Every caller sees the same k-ordered arithmetic per logit.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int keyrow32(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x4 ld4(const float* row, int k, int P) {
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
  if (k + 3 < P) t = *reinterpret_cast<const f32x4*>(row + k);
  else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (k + e < P) t[e] = row[k + e];
  }
  return t;
}

// S^T tile [64 keys][64 queries] += Y_tile X_tile^T over the whole contraction P: BKT-deep K-steps, operands global ->
// registers -> LDS (issue early / write late, two LDS buffers), wave (wm, wn) accumulates keys [32 wm, +32) x queries
// [32 wn, +32).  yrows / xrows: this thread's staging rows (thread -> row = idx / (BKT / 4), float4 idx % (BKT / 4)).
// Ends with a barrier: every wave has finished reading the buffers.
template <int BKT>
__device__ __forceinline__ void s_tile(f32x16& acc, const float* const (&yrows)[BKT / 16], const float* const (&xrows)[BKT / 16],
                                       float* smem, int P, int tid, int wm, int wn, int li, int h) {
  constexpr int LD = BKT + 4, TL = 64 * LD, NF = BKT / 16, NJJ = BKT / 8, QPR = BKT / 4;
  f32x4 ya[NF], xa[NF];
  int srow[NF], skq[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int idx = tid + i * 256;
    srow[i] = idx / QPR; skq[i] = (idx % QPR) * 4;
    ya[i] = ld4(yrows[i], skq[i], P); xa[i] = ld4(xrows[i], skq[i], P);
  }
  __syncthreads();                                                        // whoever read these buffers last is done
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    *reinterpret_cast<f32x4*>(smem + srow[i] * LD + skq[i]) = ya[i];
    *reinterpret_cast<f32x4*>(smem + TL + srow[i] * LD + skq[i]) = xa[i];
  }
  __syncthreads();
  const int nk = (P + BKT - 1) / BKT;
  for (int s = 0; s < nk; ++s) {
    const float* yt = smem + (s & 1) * 2 * TL;
    const float* xt = yt + TL;
    if (s + 1 < nk) {
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        ya[i] = ld4(yrows[i], (s + 1) * BKT + skq[i], P); xa[i] = ld4(xrows[i], (s + 1) * BKT + skq[i], P);
      }
    }
    f32x4 af[NJJ], bf[NJJ];
#pragma unroll
    for (int jj = 0; jj < NJJ; ++jj) {
      af[jj] = *reinterpret_cast<const f32x4*>(yt + (wm * 32 + li) * LD + 8 * jj + 4 * h);
      bf[jj] = *reinterpret_cast<const f32x4*>(xt + (wn * 32 + li) * LD + 8 * jj + 4 * h);
    }
#pragma unroll
    for (int jj = 0; jj < NJJ; ++jj)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[jj][e], bf[jj][e], acc, 0, 0, 0);
    if (s + 1 < nk) {
      float* nb = smem + ((s + 1) & 1) * 2 * TL;
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        *reinterpret_cast<f32x4*>(nb + srow[i] * LD + skq[i]) = ya[i];
        *reinterpret_cast<f32x4*>(nb + TL + srow[i] * LD + skq[i]) = xa[i];
      }
    }
    __syncthreads();
  }
}

}  // namespace
