// linear_ce_bwd.h — what the backward passes of the two Linear + cross-entropy probes (linear_ce.hip: C <= 64;
// linear_ce_tiled.hip: any C) share once their rows kernels have written G = g/M (softmax - onehot) [rows][ldg]:
//   * lce_wgrad_kernel<CT, GROUPED>: dW partials = G^T [X1|X2] over row splits, dbias partials alongside;
//   * lce_reduce_kernel: the splits summed in split order (+ the old contents when accumulating);
//   * lce_wgrad_splits / lce_wgrad_split_cap: the row-split plan; lce_check, lce_bwd_args_ok: what the entries accept;
//   * lce_bwd_tail: the launches above, then dX = G W by the exact-f32 GEMM of gemm_f32.hip, for one block of rows.
// Each file keeps its rows kernel, its plan and workspace layout, and its entry points.
#pragma once
#include "common.h"

namespace {

constexpr int LCE_WCOLS = 64;              // dW columns per wave of lce_wgrad_kernel (tests/test_gpu_classifier.py names it)
constexpr int LCE_MIN_SPLIT_ROWS = 256;    // rows per split at least: the partials stay a fraction of the X traffic
constexpr int LCE_TARGET_WGS = 512;        // two workgroups per CU

__device__ __forceinline__ f32x4 lce_x4(const float* X1, const float* X2, int K1, int K2, long row, int k) {
  const float* s = k < K1 ? X1 + row * K1 + k : X2 + row * K2 + (k - K1);
  return *reinterpret_cast<const f32x4*>(s);
}

struct LceW {
  const float *X1, *X2, *G;
  float *part, *bpart;                     // [S][C][K]; [S][16 CT], GROUPED: [S][C]
  int M, K1, K2, C, ldg, rows_per_split;   // M: rows of this launch; ldg: G's pitch (GROUPED reads it; else it is 16 CT)
};

// dW[c][k] = sum_i G[i][c] X[i][k]: the rows are the contraction, so the grid splits them (clipk_gemm_f32 has no split of
// its contraction: at C = 158 it left 24 workgroups walking 131072 rows each).  A wave owns 64 columns of dW for 16 CT
// classes and one row split, on v_mfma_f32_16x16x4_f32 straight from global memory; a lane's float4 of X supplies the B
// operand of four MFMAs, so MFMA j holds columns {kc + 4 n + j}.  dbias partials come from the same A registers.
// GROUPED = false: the CT class tiles are all of G, whose pitch is 16 CT (a constant: the address is one multiply-add).
// GROUPED = true (CT = 4): blockIdx.z picks a group of 64 classes; G's pitch is p.ldg >= C with zeros in the padding.
template <int CT, bool GROUPED>
__global__ __launch_bounds__(256) void lce_wgrad_kernel(const LceW p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int K = p.K1 + p.K2, C = p.C;
  constexpr int CP = CT * 16;
  const int kc = (blockIdx.x * 4 + wave) * LCE_WCOLS;
  if (kc >= K) return;                                       // (wave-uniform; no barrier in this kernel)
  const int s = blockIdx.y, cg = GROUPED ? blockIdx.z * 64 : 0;
  const int nct = !GROUPED ? CT : (C - cg + 15) / 16 < CT ? (C - cg + 15) / 16 : CT;   // class tiles that hold classes
  const long i0 = (long)s * p.rows_per_split;
  const long i1 = (i0 + p.rows_per_split < p.M) ? i0 + p.rows_per_split : (long)p.M;
  const int kq = kc + 4 * r;
  const bool kv = kq < K;
  const bool do_bias = p.bpart && blockIdx.x == 0 && wave == 0;

  f32x4 acc[CT][4];
  float bs[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    bs[ct] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (long i = i0; i < i1; i += 4) {
    const long row = i + q;
    const bool rv = row < i1;
    float a[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if constexpr (GROUPED)                                 // (below the pitch: the padding holds zeros)
        a[ct] = (rv && cg + ct * 16 + r < p.ldg) ? p.G[row * p.ldg + cg + ct * 16 + r] : 0.f;
      else
        a[ct] = rv ? p.G[row * CP + ct * 16 + r] : 0.f;
    }
    const f32x4 x = (rv && kv) ? lce_x4(p.X1, p.X2, p.K1, p.K2, row, kq) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (ct < nct) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], x[j], acc[ct][j], 0, 0, 0);
      }
      bs[ct] += a[ct];
    }
  }
  // accumulator element e of lane (n = r, q) of MFMA j: class cg + 16 ct + 4 q + e, column kc + 4 n + j
  if (p.part && kv) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cls = cg + ct * 16 + 4 * q + e;
        if (cls < C)
          *reinterpret_cast<f32x4*>(p.part + ((long)s * C + cls) * K + kq) =
              f32x4{acc[ct][0][e], acc[ct][1][e], acc[ct][2][e], acc[ct][3][e]};
      }
  }
  if (do_bias) {                                             // lane (r, q) summed the rows = q mod 4 of class cg + 16 ct + r
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float v = bs[ct];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int cls = cg + ct * 16 + r;
      if (q == 0 && (!GROUPED || cls < C)) p.bpart[(long)s * (GROUPED ? C : CP) + cls] = v;
    }
  }
}

// out (+)= sum_s part[s], s ascending; the fresh sum has the same bits with and without accumulate.  ldb: bpart's pitch
__global__ __launch_bounds__(256) void lce_reduce_kernel(const float* part, const float* bpart, int S, int C, int ldb, int K,
                                                         float* dW, float* db, int accumulate) {
  const long nq = dW ? (long)C * K / 4 : 0;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < nq) {
    const f32x4* src = reinterpret_cast<const f32x4*>(part) + t;
    f32x4 v = src[0];
    for (int s = 1; s < S; ++s) v += src[(long)s * nq];
    f32x4* dst = reinterpret_cast<f32x4*>(dW) + t;
    *dst = accumulate ? *dst + v : v;
  } else if (db && t - nq < C) {
    const int c = (int)(t - nq);
    float v = bpart[c];
    for (int s = 1; s < S; ++s) v += bpart[(long)s * ldb + c];
    db[c] = accumulate ? db[c] + v : v;
  }
}

// ---- host side
inline int lce_check(int M, int K1, int K2, int C, int max_classes) {
  if (M <= 0 || C <= 0 || K1 <= 0 || K2 < 0) return CLIPK_ERR_BAD_ARG;
  if (C > max_classes || (K1 & 3) || (K2 & 3) || (long)K1 + K2 > 4096) return CLIPK_ERR_UNSUPPORTED;
  return CLIPK_OK;
}

// the pointers and alignments of a backward entry (its workspace size is the entry's own test)
inline bool lce_bwd_args_ok(const float* X1, const float* X2, int K2, const float* W, const int64_t* labels, const float* lse,
                            const float* g, const float* dW, const float* dbias, const float* dX1, const float* dX2,
                            const void* workspace) {
  if (!X1 || !W || !labels || !lse || !g || (K2 > 0) != (X2 != nullptr) || (dX2 && K2 == 0)) return false;
  if (!dW && !dbias && !dX1 && !dX2) return false;
  return workspace && aligned16(X1) && aligned16(X2) && aligned16(W) && aligned16(dW) && aligned16(dX1) && aligned16(dX2) &&
         aligned16(workspace);
}

// row splits of lce_wgrad_kernel: about LCE_TARGET_WGS workgroups over (column blocks, 64-class groups, splits).
// lce_wgrad_split_cap bounds S for every row count up to `rows` (rows_per_split >= rows / cap, so S <= cap; the
// rounding of rows_per_split to 4 can leave a long block BELOW the cap that a shorter one reaches).
inline int lce_wgrad_split_cap(int rows, int K, int C) {
  const int nwg = ((K + 4 * LCE_WCOLS - 1) / (4 * LCE_WCOLS)) * ((C + 63) / 64);
  const int s = (rows + LCE_MIN_SPLIT_ROWS - 1) / LCE_MIN_SPLIT_ROWS;
  const int smax = LCE_TARGET_WGS / nwg > 1 ? LCE_TARGET_WGS / nwg : 1;
  return s < smax ? s : smax;
}
struct LceSplits { int S, rows_per_split; };
inline LceSplits lce_wgrad_splits(int rows, int K, int C) {
  const int s = lce_wgrad_split_cap(rows, K, C);
  const long rps = (((long)rows + s - 1) / s + 3) / 4 * 4;
  return {(int)(((long)rows + rps - 1) / rps), (int)rps};
}

// The backward of w.M rows behind their G: dW (+)= G^T [X1|X2] and dbias (+)= sum_i G as partials over row splits
// (w.part, w.bpart: room for lce_wgrad_splits' S), then the splits in order; dX = G W[:, source columns], contraction
// over the C classes (G's padded columns are never read).  GROUPED: any C, else C <= 64 and w.ldg = 16 ceil(C / 16).
template <bool GROUPED>
int lce_bwd_tail(LceW w, const float* W, int accumulate, float* dW, float* dbias, float* dX1, float* dX2, void* gemm_ws,
                 size_t gemm_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int K = w.K1 + w.K2, C = w.C;
  int e;
  if (dW || dbias) {
    LceW k = w;
    if (!dW) k.part = nullptr;
    if (!dbias) k.bpart = nullptr;
    const LceSplits sp = lce_wgrad_splits(w.M, K, C);
    const int S = sp.S;
    k.rows_per_split = sp.rows_per_split;
    const dim3 grid((unsigned)((K + 4 * LCE_WCOLS - 1) / (4 * LCE_WCOLS)), (unsigned)S, (unsigned)((C + 63) / 64)), block(256);
    if constexpr (GROUPED) {
      hipLaunchKernelGGL((lce_wgrad_kernel<4, true>), grid, block, 0, st, k);
    } else {
      switch ((C + 15) / 16) {
        case 1: hipLaunchKernelGGL((lce_wgrad_kernel<1, false>), grid, block, 0, st, k); break;
        case 2: hipLaunchKernelGGL((lce_wgrad_kernel<2, false>), grid, block, 0, st, k); break;
        case 3: hipLaunchKernelGGL((lce_wgrad_kernel<3, false>), grid, block, 0, st, k); break;
        default: hipLaunchKernelGGL((lce_wgrad_kernel<4, false>), grid, block, 0, st, k); break;
      }
    }
    e = clipk_check_launch();
    if (e != CLIPK_OK) return e;
    const long nthreads = (dW ? (long)C * K / 4 : 0) + (dbias ? C : 0);
    hipLaunchKernelGGL(lce_reduce_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, w.part, w.bpart, S, C,
                       GROUPED ? C : w.ldg, K, dW, dbias, accumulate);
    e = clipk_check_launch();
    if (e != CLIPK_OK) return e;
  }
  if (dX1) {
    e = clipk_gemm_f32(w.G, w.ldg, 0, W, K, 1, w.M, w.K1, C, nullptr, nullptr, nullptr, 0, nullptr, dX1, w.K1, gemm_ws,
                       gemm_bytes, stream);
    if (e != CLIPK_OK) return e;
  }
  if (dX2) {
    e = clipk_gemm_f32(w.G, w.ldg, 0, W + w.K1, K, 1, w.M, w.K2, C, nullptr, nullptr, nullptr, 0, nullptr, dX2, w.K2, gemm_ws,
                       gemm_bytes, stream);
    if (e != CLIPK_OK) return e;
  }
  return CLIPK_OK;
}

}  // namespace
