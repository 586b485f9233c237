// key_sum_tile.h — the weighted key sum behind cloud_tile.h's tile walk: out[q, :] = sum_key W[key, q] y_key without the
// weights leaving the workgroup.  key_sum_zero / key_sum_tile / key_sum_store: out^T += Y^T W^T of a tile whose weights
// lie in LDS, and the transposed slab store.  Device functions only, no kernel: the cloud kernels (sinkhorn.hip's apply
// pass, kernel_sums.hip, kmeans.hip, label_dist_sums.hip) take it through cloud_keysum.h, which adds the finalize kernel;
// the InfoNCE gradient kernels (simce_tiled.hip, simce_hard.hip: W = dL/dS, out = dX) include this file alone and have
// finalize kernels of their own.
#pragma once
#include "cloud_tile.h"

namespace {

// out[q, :] += sum_key W[key, q] y_key over a tile whose weights the kernel has written to LDS in the accumulator
// layout, gl[key][query]: out^T[p, q] += Y^T[p, key] W^T[key, q] as a second MFMA product whose M dimension is p.  Wave w
// owns p in [w P/4, (w+1) P/4) for all 64 queries; the key tile comes back in four 16-key blocks staged in LDS.
constexpr int KEYSUM_PMAX = 512;                  // contraction / output width limit
constexpr int YH_LD = KEYSUM_PMAX + 4;            // floats per staged key row
constexpr int KSB = 16;                           // keys per staged block of the second product
constexpr int BKG = 16;                           // K-step of the S tile (LDS budget: 2 workgroups per CU)
constexpr int KLOOP_LDS_FLOATS = 2 * 2 * 64 * (BKG + 4);                  // the K-loop buffers of s_tile<BKG>
constexpr int KEYSUM_LDS_FLOATS = TK * TQ + KSB * YH_LD;                  // weight tile gl + staged key block yh

__device__ __forceinline__ void key_sum_zero(f32x16 (&dx)[4][2]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) dx[a][b][r] = 0.f;
}

// the tile at j0: gl written by every wave (the first barrier here completes it); yh [KSB][YH_LD] is scratch.
// CACHE: the two-segment key list of KeyWalk<BKT, true>, keys [Ny, Nk) are rows of Yc.
template <bool CACHE = false>
__device__ __forceinline__ void key_sum_tile(f32x16 (&dx)[4][2], const float* Y, int Ny, int P, int j0, const float* gl,
                                             float* yh, int tid, int wid, int li, int h, const float* Yc = nullptr,
                                             int Nk = 0) {
  const int npt = (P + 127) / 128;                                        // 32-row p tiles per wave: P/4 / 32
  const int pw = npt * 32;                                                // p rows per wave
  for (int kb = 0; kb < TK / KSB; ++kb) {
    __syncthreads();                                                      // gl complete (kb = 0) / yh free again
    {
      // stage Y[16 keys][P]: thread -> (key = tid / 16, 16-B chunks c = tid % 16 + 16 i), loads first, then stores
      int j = j0 + kb * KSB + (tid >> 4);
      const float* yr;
      if constexpr (CACHE) {
        j = j < Nk ? j : Nk - 1;                                          // clamped: its weights are zero
        yr = (j < Ny) ? Y + (long)j * P : Yc + (long)(j - Ny) * P;
      } else {
        j = j < Ny ? j : Ny - 1;                                          // clamped: its weights are zero
        yr = Y + (long)j * P;
      }
      float* dst = yh + (tid >> 4) * YH_LD;
#pragma unroll
      for (int g = 0; g < 2; ++g) {                                       // two groups of four: 16 staging registers
        f32x4 tmp[KEYSUM_PMAX / 128];
#pragma unroll
        for (int i = 0; i < KEYSUM_PMAX / 128; ++i) {
          const int c = (tid & 15) + 16 * (g * (KEYSUM_PMAX / 128) + i);
          tmp[i] = (c * 4 < P) ? ld4(yr, c * 4, P) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < KEYSUM_PMAX / 128; ++i) {
          const int c = (tid & 15) + 16 * (g * (KEYSUM_PMAX / 128) + i);
          if (c * 4 < P) *reinterpret_cast<f32x4*>(dst + c * 4) = tmp[i];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < KSB / 2; ++u) {                                   // MFMA u contracts keys 2u (h = 0) and 2u + 1
      const int kl = 2 * u + h;
      const float b0 = gl[(kb * KSB + kl) * TQ + li], b1 = gl[(kb * KSB + kl) * TQ + 32 + li];
#pragma unroll
      for (int a = 0; a < 4; ++a)
        if (a < npt) {
          const int prow = wid * pw + a * 32 + li;
          const float av = prow < P ? yh[kl * YH_LD + prow] : 0.f;
          dx[a][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, dx[a][0], 0, 0, 0);
          dx[a][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, dx[a][1], 0, 0, 0);
        }
    }
  }
}

// out^T accumulators -> rows [q][p] of this split's slab in slab [ksplit][Mx][P], through LDS (one 32 x 32 block per
// wave at a time; yh holds the four).  After a barrier that follows the last key_sum_tile.
__device__ __forceinline__ void key_sum_store(const f32x16 (&dx)[4][2], float* yh, float* slab, int Mx, int P, int q0, int ks,
                                              int wid, int li, int h) {
  const int npt = (P + 127) / 128, pw = npt * 32;
  float* tb = yh + wid * (32 * 33);
#pragma unroll
  for (int a = 0; a < 4; ++a) {                             // (fully unrolled: the accumulators are register arrays)
    if (a < npt) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) tb[li * 33 + keyrow32(r, h)] = dx[a][b][r];    // [query][p]
        // wave-private region: the wave's own writes are visible to its reads in program order
#pragma unroll
        for (int it = 0; it < 16; ++it) {
          const int ql = it * 2 + h;                                      // 2 query rows per pass, 32 consecutive p each
          const int q = q0 + b * 32 + ql, pp = wid * pw + a * 32 + li;
          if (q < Mx && pp < P) slab[((long)ks * Mx + q) * P + pp] = tb[ql * 33 + li];
        }
      }
    }
  }
}

}  // namespace
