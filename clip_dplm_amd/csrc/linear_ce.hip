// linear_ce.hip — Linear(K, C) + cross-entropy against integer labels for the downstream classifier probes: every head of
// old/classifier.py ends in nn.Linear(h, num_classes) and old/ablation.py:30,45 feeds its logits to nn.CrossEntropyLoss /
// torch.max.  A tall-skinny product (M rows, K <= 4096 columns, C <= 64 classes) in exact f32 (v_mfma_f32_16x16x4_f32:
// bitwise an fmaf chain), classes padded to the 16-wide MFMA tile; two row sources [X1 | X2] stand for the
// torch.cat([rna_embeds, protein_embeds], -1) of old/ablation.py:29,44 without making it.
//
//   lce_rows_kernel<CT, false>   forward: Z = [X1|X2] W^T + b per 16-row tile, then lse / target logit / first-occurrence
//                                argmax per row from the accumulators (and the logits, if asked for)
//   lce_rows_kernel<CT, true>    backward, step 1: the same Z (same code, same bits), G = g/M (softmax - onehot) -> workspace
//   lce_bwd_tail<false>          backward, steps 2 and 3 (linear_ce_bwd.h, shared with linear_ce_tiled.hip): dW / dbias
//                                partials over row splits by lce_wgrad_kernel<CT, false>, the splits summed in split order,
//                                and dX = G W by the exact-f32 GEMM of gemm_f32.hip (only when asked for)
// No atomics anywhere: a result depends on the shapes alone.
//
// The operands go from global memory straight into MFMA registers: a lane's float4 along the contraction supplies four
// consecutive MFMA steps, so step j of a 16-column chunk contracts columns {4 q + j : q = 0 .. 3} - a permutation of the
// chunk's order that A and B share.  W (C x K x 4 bytes <= 1 MiB) stays cache-resident; X is streamed.
#include "common.h"
#include "cloud_tile.h"                    // take_better: the (value, class) order of the argmax merge
#include "linear_ce_bwd.h"
#include <math.h>

namespace {

constexpr int LCE_KSTEP = 16;              // contraction columns per main-loop step (tests/test_gpu_classifier.py names it)
constexpr int LCE_RT = 2;                  // 16-row tiles per wave
constexpr int LCE_WG_ROWS = 4 * LCE_RT * 16;
constexpr int LCE_MAX_C = 64;              // four 16-class accumulator tiles

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
          if constexpr (CT == 2) {                           // (take_better's selects: 64 registers here against 60)
            if (m2 > m || (m2 == m && b2 < bi)) { m = m2; bi = b2; }
          } else {
            take_better(m, bi, m2, b2);
          }
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

// ---- host side
struct LcePlan {
  int CT, CP, S;                           // S: the row splits lce_bwd_tail will use (lce_wgrad_splits)
  size_t g_bytes, part_bytes, bpart_bytes;
};

LcePlan lce_plan(int M, int K1, int K2, int C) {
  LcePlan pl;
  const int K = K1 + K2;
  pl.CT = (C + 15) / 16;
  pl.CP = pl.CT * 16;
  pl.S = lce_wgrad_splits(M, K, C).S;
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
  if (lce_check(M, K1, K2, C, LCE_MAX_C) != CLIPK_OK) return 0;
  const LcePlan pl = lce_plan(M, K1, K2, C);
  return pl.g_bytes + pl.part_bytes + pl.bpart_bytes;
}

extern "C" int clipk_linear_ce_fwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                   const int64_t* labels, int M, int C, float* lse, float* tgt, int64_t* pred,
                                   float* logits, int64_t ldz, void* stream) {
  const int rc = lce_check(M, K1, K2, C, LCE_MAX_C);
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
  const int rc = lce_check(M, K1, K2, C, LCE_MAX_C);
  if (rc != CLIPK_OK) return rc;
  if (!lce_bwd_args_ok(X1, X2, K2, W, labels, lse, g, dW, dbias, dX1, dX2, workspace)) return CLIPK_ERR_BAD_ARG;
  const LcePlan pl = lce_plan(M, K1, K2, C);
  if (workspace_bytes < pl.g_bytes + pl.part_bytes + pl.bpart_bytes) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
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

  LceW w{};
  w.X1 = X1; w.X2 = X2; w.G = G; w.part = part; w.bpart = bpart;
  w.M = M; w.K1 = K1; w.K2 = K2; w.C = C; w.ldg = pl.CP;
  return lce_bwd_tail<false>(w, W, accumulate, dW, dbias, dX1, dX2, nullptr, 0, stream);
}
