// plane_tile.h — what the bf16-plane kernels (retrieval.hip's sim_cand_kernel, sinkhorn.hip's sinkhorn_lse_x3_kernel)
// share, the counterpart of cloud_tile.h's KeyWalk on v_mfma_f32_32x32x16_bf16:
//   * PlaneWalk: one workgroup's walk over the 64-key tiles of its key split for a block of 128 queries - coordinates,
//     staging pointers, the double-buffered K-loop over the planes clipk_split_bf16 writes.
// Each kernel keeps its __shared__ array, what it does with the products, its lane-half merge and its partial format.
#pragma once
#include "common.h"

namespace {

constexpr int PLQ = 128, PLK = 64;                // queries per workgroup, keys per tile
constexpr int PLBK = 32, PLLD = PLBK + 8;         // K-step in bf16 elements (two MFMA k-steps), LDS row pitch (80 B)

// Workgroup (blockIdx.x, blockIdx.y) = (query block, key split), 256 threads.  Wave w owns queries [32 w, +32) against
// all 64 keys of a tile: two 32 x 32 accumulators sharing one query fragment; lane li of half h holds query qg and key
// j0 + 32 kb + keyrow32(r, h) in acc[kb][r].  NPL planes per operand: 1 (bf16: hi) or 2 (bf16x3: hi and lo, three MFMAs
// per fragment pair into the same accumulator - hi.hi, hi.lo, lo.hi).  The planes have a row pitch PP that is a
// multiple of PLBK with zero pads: the K-loop has no tail and every staging load is 16 bytes.
template <int NPL>
struct PlaneWalk {
  static constexpr int KT = PLK * PLLD, QT = PLQ * PLLD, BUF = NPL * (KT + QT);   // one buffer: key planes | query planes
  static constexpr int LDS_ELEMS = 2 * BUF;       // the kernel's __shared__ unsigned short array (16-byte aligned)

  const unsigned short* yh; const unsigned short* yl; int Ny, PP;
  unsigned short* sm;
  int w, li, h;
  int sr, sc;                                     // staging: row sr (+64 for queries), 16-byte chunk sc
  int q0, ks, qg;
  int t_beg, t_end;                               // this split's tiles
  const unsigned short* xs[2][NPL];               // this thread's query staging pointers

  // xl / yl_ are read with NPL == 2 only.  Queries beyond Mx are clamped: computed and dropped by the caller.
  __device__ __forceinline__ PlaneWalk(const unsigned short* xh, const unsigned short* xl, int Mx,
                                       const unsigned short* yh_, const unsigned short* yl_, int Ny_, int PP_,
                                       int tiles_per_split, int ntiles, unsigned short* sm_)
      : yh(yh_), yl(yl_), Ny(Ny_), PP(PP_), sm(sm_) {
    const int tid = threadIdx.x, lane = tid & 63;
    w = tid >> 6; li = lane & 31; h = lane >> 5;
    sr = tid >> 2; sc = (tid & 3) * 8;
    q0 = blockIdx.x * PLQ; ks = blockIdx.y;
    qg = q0 + w * 32 + li;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int q = q0 + sr + 64 * i; q = q < Mx ? q : Mx - 1;
      xs[i][0] = xh + (long)q * PP + sc;
      if constexpr (NPL == 2) xs[i][1] = xl + (long)q * PP + sc;
    }
    t_beg = ks * tiles_per_split;
    t_end = t_beg + tiles_per_split; t_end = t_end < ntiles ? t_end : ntiles;
  }

  // acc[kb][r] = <y_(j0 + 32 kb + keyrow32(r, h)), x_qg>.  Starts and ends with a barrier: LDS the workgroup read before
  // the call is free once it has begun.  Keys beyond Ny are clamped: masked in the caller's epilogue.
  __device__ __forceinline__ void product(int j0, f32x16 (&acc)[2]) const {
    int j = j0 + sr; j = j < Ny ? j : Ny - 1;
    const unsigned short* ys[NPL];
    ys[0] = yh + (long)j * PP + sc;
    if constexpr (NPL == 2) ys[1] = yl + (long)j * PP + sc;
    u32x4 ky[NPL], kq[2][NPL];
    auto load = [&](int k0) {
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        ky[pl] = *reinterpret_cast<const u32x4*>(ys[pl] + k0);
        kq[0][pl] = *reinterpret_cast<const u32x4*>(xs[0][pl] + k0);
        kq[1][pl] = *reinterpret_cast<const u32x4*>(xs[1][pl] + k0);
      }
    };
    auto store = [&](unsigned short* b) {
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        *reinterpret_cast<u32x4*>(b + pl * KT + sr * PLLD + sc) = ky[pl];
        *reinterpret_cast<u32x4*>(b + NPL * KT + pl * QT + sr * PLLD + sc) = kq[0][pl];
        *reinterpret_cast<u32x4*>(b + NPL * KT + pl * QT + (sr + 64) * PLLD + sc) = kq[1][pl];
      }
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    const int ns = PP / PLBK;
    load(0);
    __syncthreads();                                                      // whoever read these buffers last is done
    store(sm);
    __syncthreads();
    for (int st = 0; st < ns; ++st) {
      const unsigned short* b = sm + (st & 1) * BUF;
      if (st + 1 < ns) load((st + 1) * PLBK);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 a[2][NPL], bq[NPL];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
            a[kb][pl] = *reinterpret_cast<const bf16x8*>(b + pl * KT + (kb * 32 + li) * PLLD + kk * 16 + 8 * h);
          bq[pl] = *reinterpret_cast<const bf16x8*>(b + NPL * KT + pl * QT + (w * 32 + li) * PLLD + kk * 16 + 8 * h);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kb][0], bq[0], acc[kb], 0, 0, 0);
          if constexpr (NPL == 2) {
            acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kb][0], bq[1], acc[kb], 0, 0, 0);
            acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kb][1], bq[0], acc[kb], 0, 0, 0);
          }
        }
      }
      if (st + 1 < ns) store(sm + ((st + 1) & 1) * BUF);
      __syncthreads();
    }
  }
};

}  // namespace
