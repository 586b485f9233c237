// linear_ce.hip — Linear(K, C) + cross-entropy against integer labels for the downstream classifier probes: every head of
// old/classifier.py ends in nn.Linear(h, num_classes) and old/ablation.py:30,45 feeds its logits to nn.CrossEntropyLoss /
// torch.max.  A tall-skinny product (M rows, K <= 4096 columns, C <= 64 classes) in exact f32 (v_mfma_f32_16x16x4_f32:
// bitwise an fmaf chain), classes padded to the 16-wide MFMA tile; two row sources [X1 | X2] stand for the
// torch.cat([rna_embeds, protein_embeds], -1) of old/ablation.py:29,44 without making it.
//
//   lce_rows_kernel<CT, false>   forward: Z = [X1|X2] W^T + b per 16-row tile, then lse / target logit / first-occurrence
//                                argmax per row from the accumulators (and the logits, if asked for)
//   lce_rows_kernel<CT, true>    backward, step 1: the same Z (same code, same bits), G = g/M (softmax - onehot) -> workspace
//   lce_wgrad_kernel<CT>         backward, step 2: dW partials = G^T [X1|X2] over row splits, dbias partials alongside
//   lce_reduce_kernel            backward, step 3: the splits summed in split order (+ the old contents when accumulating)
//   dX = G W                     the tiled exact-f32 GEMM of gemm_f32.hip on the G workspace (only when asked for)
// No atomics anywhere: a result depends on the shapes alone.
//
// The operands go from global memory straight into MFMA registers: a lane's float4 along the contraction supplies four
// consecutive MFMA steps, so step j of a 16-column chunk contracts columns {4 q + j : q = 0 .. 3} - a permutation of the
// chunk's order that A and B share.  W (C x K x 4 bytes <= 1 MiB) stays cache-resident; X is streamed.
#include "common.h"
#include <math.h>

namespace {

constexpr int LCE_KSTEP = 16;              // contraction columns per main-loop step (tests/test_gpu_classifier.py names it)
constexpr int LCE_RT = 2;                  // 16-row tiles per wave
constexpr int LCE_WG_ROWS = 4 * LCE_RT * 16;
constexpr int LCE_WCOLS = 64;              // dW columns per wave of lce_wgrad_kernel
constexpr int LCE_MIN_SPLIT_ROWS = 256;    // rows per split at least: the partials stay a fraction of the X traffic
constexpr int LCE_TARGET_WGS = 512;

struct LceP {
  const float *X1, *X2, *W, *bias;
  const int64_t* labels;
  int M, K1, K2, C;
  float *lse, *tgt;                        // forward outputs
  int64_t* pred;
  float* logits;
  long ldz;
  const float *lse_in, *g;                 // backward inputs
  float* G;                                // backward: [M][16 CT]
};

__device__ __forceinline__ f32x4 lce_x4(const float* X1, const float* X2, int K1, int K2, long row, int k) {
  const float* s = k < K1 ? X1 + row * K1 + k : X2 + row * K2 + (k - K1);
  return *reinterpret_cast<const f32x4*>(s);
}

template <int CT, bool BWD>
__global__ __launch_bounds__(256) void lce_rows_kernel(LceP p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int K = p.K1 + p.K2, M = p.M, C = p.C;
  const long row0 = ((long)blockIdx.x * 4 + wave) * (LCE_RT * 16);
  if (row0 >= M) return;                                     // (wave-uniform; no barrier in this kernel)

  f32x4 acc[LCE_RT][CT];
#pragma unroll
  for (int rt = 0; rt < LCE_RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += LCE_KSTEP) {
    const int kq = k0 + 4 * q;
    const bool kv = kq < K;                                  // (K % 4 == 0: a lane's four columns are in or out together)
    f32x4 xa[LCE_RT], wb[CT];
#pragma unroll
    for (int rt = 0; rt < LCE_RT; ++rt) {
      const long row = row0 + rt * 16 + r;
      xa[rt] = (kv && row < M) ? lce_x4(p.X1, p.X2, p.K1, p.K2, row, kq) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int cls = ct * 16 + r;
      wb[ct] = (kv && cls < C) ? *reinterpret_cast<const f32x4*>(p.W + (long)cls * K + kq) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int rt = 0; rt < LCE_RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt][j], wb[ct][j], acc[rt][ct], 0, 0, 0);
  }

  // accumulator element j of lane (r, q): row 4 q + j of the tile, class 16 ct + r.  A row's classes sit on 16 lanes.
  float bz[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) bz[ct] = (p.bias && ct * 16 + r < C) ? p.bias[ct * 16 + r] : 0.f;
  const float gs = BWD ? p.g[0] / (float)M : 0.f;
#pragma unroll
  for (int rt = 0; rt < LCE_RT; ++rt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long row = row0 + rt * 16 + 4 * q + j;
      const bool rv = row < M;
      float z[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) z[ct] = (ct * 16 + r < C) ? acc[rt][ct][j] + bz[ct] : -INFINITY;
      const long lab = (rv && p.labels) ? (long)p.labels[row] : -1L;
      const bool lab_ok = lab >= 0 && lab < C;
      if constexpr (!BWD) {
        float m = z[0];
        int bi = r;
#pragma unroll
        for (int ct = 1; ct < CT; ++ct)
          if (z[ct] > m) { m = z[ct]; bi = ct * 16 + r; }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {                   // (max, lowest class) is associative: any merge order
          const float m2 = __shfl_xor(m, o, 64);
          const int b2 = __shfl_xor(bi, o, 64);
          if (m2 > m || (m2 == m && b2 < bi)) { m = m2; bi = b2; }
        }
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int cls = ct * 16 + r;
          if (cls < C) s += expf(z[ct] - m);
          if (cls == lab) t = z[ct];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          s += __shfl_xor(s, o, 64);
          t += __shfl_xor(t, o, 64);                         // one non-zero term at most
        }
        if (rv) {
          if (r == 0) {
            if (p.lse) p.lse[row] = m + logf(s);
            if (p.tgt) p.tgt[row] = lab_ok ? t : NAN;
            if (p.pred) p.pred[row] = bi;
          }
          if (p.logits) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
              if (ct * 16 + r < C) p.logits[row * p.ldz + ct * 16 + r] = z[ct];
          }
        }
      } else {
        if (rv) {
          const float l = p.lse_in[row];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const int cls = ct * 16 + r;
            float gv = 0.f;                                  // padded classes and rows with a label outside [0, C): zero
            if (lab_ok && cls < C) gv = gs * (expf(z[ct] - l) - (cls == lab ? 1.f : 0.f));
            p.G[row * (CT * 16) + cls] = gv;
          }
        }
      }
    }
  }
}

struct LceW {
  const float *X1, *X2, *G;
  float *part, *bpart;                     // [S][C][K], [S][16 CT]
  int M, K1, K2, C, rows_per_split;
};

// dW[c][k] = sum_i G[i][c] X[i][k]: the rows are the contraction.  A wave owns 64 columns of dW for every class and one
// row split; a lane's float4 of X supplies the B operand of four MFMAs, so MFMA j holds columns {kc + 4 n + j}.
template <int CT>
__global__ __launch_bounds__(256) void lce_wgrad_kernel(LceW p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int K = p.K1 + p.K2, C = p.C;
  constexpr int CP = CT * 16;
  const int kc = (blockIdx.x * 4 + wave) * LCE_WCOLS;
  if (kc >= K) return;                                       // (wave-uniform; no barrier in this kernel)
  const int s = blockIdx.y;
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
    for (int ct = 0; ct < CT; ++ct) a[ct] = rv ? p.G[row * CP + ct * 16 + r] : 0.f;
    const f32x4 x = (rv && kv) ? lce_x4(p.X1, p.X2, p.K1, p.K2, row, kq) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], x[j], acc[ct][j], 0, 0, 0);
      bs[ct] += a[ct];
    }
  }
  // accumulator element e of lane (n = r, q) of MFMA j: class 16 ct + 4 q + e, column kc + 4 n + j
  if (p.part && kv) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cls = ct * 16 + 4 * q + e;
        if (cls < C)
          *reinterpret_cast<f32x4*>(p.part + ((long)s * C + cls) * K + kq) =
              f32x4{acc[ct][0][e], acc[ct][1][e], acc[ct][2][e], acc[ct][3][e]};
      }
  }
  if (do_bias) {                                             // lane (r, q) summed the rows = q mod 4 of class 16 ct + r
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float v = bs[ct];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (q == 0) p.bpart[(long)s * CP + ct * 16 + r] = v;
    }
  }
}

// out (+)= sum_s part[s], s ascending; the fresh sum has the same bits with and without accumulate
__global__ __launch_bounds__(256) void lce_reduce_kernel(const float* part, const float* bpart, int S, int C, int CP, int K,
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
    for (int s = 1; s < S; ++s) v += bpart[(long)s * CP + c];
    db[c] = accumulate ? db[c] + v : v;
  }
}

// ---- host side
struct LcePlan {
  int CT, CP, S, rows_per_split;
  size_t g_bytes, part_bytes, bpart_bytes;
};

int lce_check(int M, int K1, int K2, int C) {
  if (M <= 0 || C <= 0 || K1 <= 0 || K2 < 0) return CLIPK_ERR_BAD_ARG;
  if (C > 64 || (K1 & 3) || (K2 & 3) || (long)K1 + K2 > 4096) return CLIPK_ERR_UNSUPPORTED;
  return CLIPK_OK;
}

LcePlan lce_plan(int M, int K1, int K2, int C) {
  LcePlan pl;
  const int K = K1 + K2;
  pl.CT = (C + 15) / 16;
  pl.CP = pl.CT * 16;
  const int nkb = (K + 4 * LCE_WCOLS - 1) / (4 * LCE_WCOLS);
  int S = (M + LCE_MIN_SPLIT_ROWS - 1) / LCE_MIN_SPLIT_ROWS;
  const int smax = LCE_TARGET_WGS / nkb > 1 ? LCE_TARGET_WGS / nkb : 1;
  if (S > smax) S = smax;
  long rps = ((long)M + S - 1) / S;
  rps = (rps + 3) / 4 * 4;
  pl.rows_per_split = (int)rps;
  pl.S = (int)(((long)M + rps - 1) / rps);
  pl.g_bytes = (size_t)M * pl.CP * sizeof(float);
  pl.part_bytes = (size_t)pl.S * C * K * sizeof(float);
  pl.bpart_bytes = (size_t)pl.S * pl.CP * sizeof(float);
  return pl;
}

template <bool BWD>
void lce_launch_rows(int CT, const LceP& p, hipStream_t st) {
  const dim3 grid((unsigned)(((long)p.M + LCE_WG_ROWS - 1) / LCE_WG_ROWS)), block(256);
  switch (CT) {
    case 1: hipLaunchKernelGGL((lce_rows_kernel<1, BWD>), grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL((lce_rows_kernel<2, BWD>), grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL((lce_rows_kernel<3, BWD>), grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL((lce_rows_kernel<4, BWD>), grid, block, 0, st, p); break;
  }
}

}  // namespace

extern "C" size_t clipk_linear_ce_workspace(int M, int K1, int K2, int C) {
  if (lce_check(M, K1, K2, C) != CLIPK_OK) return 0;
  const LcePlan pl = lce_plan(M, K1, K2, C);
  return pl.g_bytes + pl.part_bytes + pl.bpart_bytes;
}

extern "C" int clipk_linear_ce_fwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                   const int64_t* labels, int M, int C, float* lse, float* tgt, int64_t* pred,
                                   float* logits, int64_t ldz, void* stream) {
  const int rc = lce_check(M, K1, K2, C);
  if (rc != CLIPK_OK) return rc;
  if (!X1 || !W || (K2 > 0) != (X2 != nullptr) || (tgt && !labels) || (logits && ldz < C)) return CLIPK_ERR_BAD_ARG;
  if (!lse && !tgt && !pred && !logits) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X1) || !aligned16(X2) || !aligned16(W)) return CLIPK_ERR_BAD_ARG;
  LceP p{};
  p.X1 = X1; p.X2 = X2; p.W = W; p.bias = bias; p.labels = labels;
  p.M = M; p.K1 = K1; p.K2 = K2; p.C = C;
  p.lse = lse; p.tgt = tgt; p.pred = pred; p.logits = logits; p.ldz = (long)ldz;
  lce_launch_rows<false>((C + 15) / 16, p, (hipStream_t)stream);
  return clipk_check_launch();
}

extern "C" int clipk_linear_ce_bwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                   const int64_t* labels, int M, int C, const float* lse, const float* g, int accumulate,
                                   float* dW, float* dbias, float* dX1, float* dX2, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const int rc = lce_check(M, K1, K2, C);
  if (rc != CLIPK_OK) return rc;
  if (!X1 || !W || !labels || !lse || !g || (K2 > 0) != (X2 != nullptr) || (dX2 && K2 == 0)) return CLIPK_ERR_BAD_ARG;
  if (!dW && !dbias && !dX1 && !dX2) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X1) || !aligned16(X2) || !aligned16(W) || !aligned16(dW) || !aligned16(dX1) || !aligned16(dX2) ||
      !aligned16(workspace))
    return CLIPK_ERR_BAD_ARG;
  const LcePlan pl = lce_plan(M, K1, K2, C);
  if (!workspace || workspace_bytes < pl.g_bytes + pl.part_bytes + pl.bpart_bytes) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int K = K1 + K2;
  float* G = reinterpret_cast<float*>(workspace);
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pl.g_bytes);
  float* bpart = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pl.g_bytes + pl.part_bytes);

  LceP p{};
  p.X1 = X1; p.X2 = X2; p.W = W; p.bias = bias; p.labels = labels;
  p.M = M; p.K1 = K1; p.K2 = K2; p.C = C;
  p.lse_in = lse; p.g = g; p.G = G;
  lce_launch_rows<true>(pl.CT, p, st);
  int e = clipk_check_launch();
  if (e != CLIPK_OK) return e;

  if (dW || dbias) {
    LceW w{};
    w.X1 = X1; w.X2 = X2; w.G = G; w.part = dW ? part : nullptr; w.bpart = dbias ? bpart : nullptr;
    w.M = M; w.K1 = K1; w.K2 = K2; w.C = C; w.rows_per_split = pl.rows_per_split;
    const dim3 grid((unsigned)((K + 4 * LCE_WCOLS - 1) / (4 * LCE_WCOLS)), (unsigned)pl.S), block(256);
    switch (pl.CT) {
      case 1: hipLaunchKernelGGL((lce_wgrad_kernel<1>), grid, block, 0, st, w); break;
      case 2: hipLaunchKernelGGL((lce_wgrad_kernel<2>), grid, block, 0, st, w); break;
      case 3: hipLaunchKernelGGL((lce_wgrad_kernel<3>), grid, block, 0, st, w); break;
      default: hipLaunchKernelGGL((lce_wgrad_kernel<4>), grid, block, 0, st, w); break;
    }
    e = clipk_check_launch();
    if (e != CLIPK_OK) return e;
    const long nthreads = (dW ? (long)C * K / 4 : 0) + (dbias ? C : 0);
    hipLaunchKernelGGL(lce_reduce_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, part, bpart, pl.S, C,
                       pl.CP, K, dW, dbias, accumulate);
    e = clipk_check_launch();
    if (e != CLIPK_OK) return e;
  }
  // dX = G W[:, source columns]: contraction over the C classes (G's padded columns are never read)
  if (dX1) {
    e = clipk_gemm_f32(G, pl.CP, 0, W, K, 1, M, K1, C, nullptr, nullptr, nullptr, 0, nullptr, dX1, K1, nullptr, 0, stream);
    if (e != CLIPK_OK) return e;
  }
  if (dX2) {
    e = clipk_gemm_f32(G, pl.CP, 0, W + K1, K, 1, M, K2, C, nullptr, nullptr, nullptr, 0, nullptr, dX2, K2, nullptr, 0, stream);
    if (e != CLIPK_OK) return e;
  }
  return CLIPK_OK;
}
