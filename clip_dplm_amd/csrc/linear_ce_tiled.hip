// linear_ce_tiled.hip — Linear(K, C) + cross-entropy against integer labels for ANY class count (include/clipk.h:
// clipk_linear_ce_tiled_*).  linear_ce.hip keeps a row's whole logit vector in at most four 16-class accumulator tiles and
// stops at C = 64; the reference's own probes are far wider (run1/proposal.MD:3: 2,547 immune cell types and 158 markers;
// old/ablation.py:51 and old/classifier.py take num_classes as a free argument).  Here the classes are walked in tiles:
//
//   lcet_rows_kernel<false>   forward: a workgroup owns 64 rows of [X1|X2] and walks 64-class tiles of W with the exact-f32
//                             64 x 64 tile of sim_tile.h (classes on the MFMA rows, X rows on the lanes; the two sources
//                             are two s_tile calls into one accumulator).  Each lane keeps (m, l, best value, best class,
//                             target logit) of its row; lane halves and the two class-waves merge at the end.  Class-range
//                             splits (cloud_tile.h's key_split_plan) fill the chip when M is small.
//   lcet_finalize_kernel      the splits' partials [split][M][5] merged in split order -> lse, tgt, pred
//   lcet_rows_kernel<true>    backward, step 1: the same Z (same code, same bits), G = g/M (softmax - onehot) -> workspace,
//                             pitch C rounded up to 4 with zeros in the padding
//   lce_bwd_tail<true>        backward, steps 2 and 3 (linear_ce_bwd.h, shared with linear_ce.hip): dW / dbias partials over
//                             row splits and 64-class groups by lce_wgrad_kernel<4, true>, the splits summed in split
//                             order, and dX = G W by the exact-f32 GEMM of gemm_f32.hip, one call per source
// The backward walks the rows in slabs whose G stays below LCET_SLAB_BYTES, so that a slab's G is still in the Infinity
// Cache when its consumers read it; dW / dbias accumulate over the slabs in slab order.
// The argmax merge rule is cloud_tile.h's take_better ("larger value, then lower class"): associative, so any merge order
// gives the first occurrence.  No atomics anywhere: a result depends on the shapes alone.
#include "common.h"
#include "cloud_tile.h"                    // sim_tile.h's tile, key_split_plan, NO_KEY, take_better
#include "linear_ce_bwd.h"
#include <math.h>

#ifndef LCET_SLAB_BYTES
#define LCET_SLAB_BYTES (128ll << 20)      // G bytes per backward slab (profiles/probe/README.md has the A/B)
#endif

namespace {

constexpr int LT_ROWS = 64, LT_CLS = 64;   // X rows per workgroup, classes per tile
constexpr int LT_BK = 32;                  // K-step of the tile: 16 MFMAs per wave between barriers
constexpr int LT_NF = LT_BK / 16;          // staging float4s per thread and operand
constexpr int LT_MAX_C = 65536;
static_assert(LT_CLS == TK, "key_split_plan counts the 64-class tiles");

struct TP {
  const float *X1, *X2, *W, *bias;
  const int64_t* labels;
  int M, K1, K2, C;                        // M: rows of this launch (a slab of the backward)
  int tiles_per_split, ntiles;
  float* part;                             // forward: [split][M][5] = m, l, best value, best class (bits), target logit
  const float *lse, *g;                    // backward inputs
  float m_total;                           // backward: the batch's row count (G carries g / M of the whole batch)
  float* G;                                // backward: [M][ldg]
  int ldg;
};

template <bool BWD>
__global__ __launch_bounds__(256, 2) void lcet_rows_kernel(const TP p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (LT_BK + 4)];   // 2 buffers x (classes | rows)
  __shared__ float mrg[2][5][LT_ROWS];                                            // [class-wave][statistic][row]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;                                          // class half, row half
  const int li = lane & 31, h = lane >> 5;
  const int M = p.M, C = p.C, K = p.K1 + p.K2;
  const long r0 = (long)blockIdx.x * LT_ROWS;
  const long row = r0 + wn * 32 + li;                                             // this lane's row
  const bool rv = row < M;
  const long lab = (rv && p.labels) ? (long)p.labels[row] : -1L;
  const bool lab_ok = lab >= 0 && lab < C;
  const int labi = lab_ok ? (int)lab : -1;

  const float* x1rows[LT_NF];
  const float* x2rows[LT_NF];
#pragma unroll
  for (int i = 0; i < LT_NF; ++i) {
    long r = r0 + (tid + i * 256) / (LT_BK / 4);
    r = r < M ? r : (long)M - 1;                                                  // clamped: never stored
    x1rows[i] = p.X1 + r * p.K1;
    x2rows[i] = p.K2 ? p.X2 + r * p.K2 : p.X1;
  }
  const int t_beg = blockIdx.y * p.tiles_per_split;
  int t_end = t_beg + p.tiles_per_split;
  t_end = t_end < p.ntiles ? t_end : p.ntiles;

  float m_run = -INFINITY, l_run = 0.f, bv = -INFINITY, tg = 0.f;
  int bc = NO_KEY;
  float lse_i = 0.f, gs = 0.f;
  if constexpr (BWD) {
    lse_i = rv ? p.lse[row] : 0.f;
    gs = p.g[0] / p.m_total;
  }

  for (int kt = t_beg; kt < t_end; ++kt) {
    const int c0 = kt * LT_CLS, cb = c0 + wm * 32;
    const float* w1rows[LT_NF];
    const float* w2rows[LT_NF];
#pragma unroll
    for (int i = 0; i < LT_NF; ++i) {
      int c = c0 + (tid + i * 256) / (LT_BK / 4);
      c = c < C ? c : C - 1;                                                      // clamped: masked in the epilogue
      w1rows[i] = p.W + (long)c * K;
      w2rows[i] = w1rows[i] + p.K1;
    }
    float bz[16];                                                                 // bias of this lane's 16 classes
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cls = cb + keyrow32(r, h);
      bz[r] = (p.bias && cls < C) ? p.bias[cls] : 0.f;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<LT_BK>(acc, w1rows, x1rows, smem, p.K1, tid, wm, wn, li, h);
    if (p.K2) s_tile<LT_BK>(acc, w2rows, x2rows, smem, p.K2, tid, wm, wn, li, h);

    if constexpr (!BWD) {
      // ---- running statistics of this lane's row over its 16 classes of the tile (keyrow32 ascends with r)
      float z[16], tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cls = cb + keyrow32(r, h);
        const bool cv = cls < C;
        z[r] = cv ? acc[r] + bz[r] : -INFINITY;
        tmax = fmaxf(tmax, z[r]);
        if (cv && (z[r] > bv || bc == NO_KEY)) { bv = z[r]; bc = cls; }
        if (cls == labi) tg = z[r];
      }
      if (tmax > -INFINITY) {
        const float m_new = fmaxf(m_run, tmax);
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) a += expf(z[r] - m_new);                     // exp(-inf) = 0 for padded classes
        l_run = l_run * expf(m_run - m_new) + a;
        m_run = m_new;
      }
    } else {
      // ---- G: accumulator elements 4 a .. 4 a + 3 are four consecutive classes -> one 16-byte store
      if (rv) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int cls0 = cb + 8 * a + 4 * h;
          if (cls0 < p.ldg) {                                                     // (ldg % 4 == 0: a group is in or out whole)
            f32x4 gv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int cls = cls0 + e;
              const float z = acc[4 * a + e] + bz[4 * a + e];
              // padded classes and rows with a label outside [0, C): zero
              gv[e] = (lab_ok && cls < C) ? gs * (expf(z - lse_i) - (cls == labi ? 1.f : 0.f)) : 0.f;
            }
            *reinterpret_cast<f32x4*>(p.G + row * p.ldg + cls0) = gv;
          }
        }
      }
    }
  }

  if constexpr (!BWD) {
    // ---- merge: lane halves, then the two class-waves
    auto merge = [&](float m_o, float l_o, float bv_o, int bc_o, float tg_o) {
      const float m_n = fmaxf(m_run, m_o);
      float l_n = 0.f;
      if (m_n > -INFINITY) l_n = l_run * expf(m_run - m_n) + l_o * expf(m_o - m_n);
      m_run = m_n; l_run = l_n;
      take_better(bv, bc, bv_o, bc_o);
      tg += tg_o;                                                                // one non-zero term at most
    };
    merge(__shfl_xor(m_run, 32, 64), __shfl_xor(l_run, 32, 64), __shfl_xor(bv, 32, 64), __shfl_xor(bc, 32, 64),
          __shfl_xor(tg, 32, 64));
    const int rl = wn * 32 + li;
    if (h == 0) {
      mrg[wm][0][rl] = m_run; mrg[wm][1][rl] = l_run; mrg[wm][2][rl] = bv; mrg[wm][3][rl] = __int_as_float(bc);
      mrg[wm][4][rl] = tg;
    }
    __syncthreads();
    if (wm == 0 && h == 0 && rv) {
      merge(mrg[1][0][rl], mrg[1][1][rl], mrg[1][2][rl], __float_as_int(mrg[1][3][rl]), mrg[1][4][rl]);
      float* o = p.part + ((long)blockIdx.y * M + row) * 5;
      o[0] = m_run; o[1] = l_run; o[2] = bv; o[3] = __int_as_float(bc); o[4] = tg;
    }
  }
}

// the splits in split order -> lse / tgt / pred (each may be null)
__global__ __launch_bounds__(256) void lcet_finalize_kernel(const float* part, int S, int M, int C, const int64_t* labels,
                                                            float* lse, float* tgt, int64_t* pred) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const float* o = part + row * 5;
  float m = o[0], l = o[1], bv = o[2], tg = o[4];
  int bc = __float_as_int(o[3]);
  for (int s = 1; s < S; ++s) {
    o = part + ((long)s * M + row) * 5;
    const float m_o = o[0], l_o = o[1];
    const float m_n = fmaxf(m, m_o);
    float l_n = 0.f;
    if (m_n > -INFINITY) l_n = l * expf(m - m_n) + l_o * expf(m_o - m_n);
    m = m_n; l = l_n;
    take_better(bv, bc, o[2], __float_as_int(o[3]));
    tg += o[4];
  }
  if (lse) lse[row] = m + logf(l);
  if (tgt) {
    const long lab = (long)labels[row];
    tgt[row] = (lab >= 0 && lab < C) ? tg : NAN;
  }
  if (pred) pred[row] = bc == NO_KEY ? 0 : bc;
}

// ---- host side
size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct LcetPlan {
  int ldg, slab_rows;                      // G pitch; rows per backward slab (a multiple of 64, or all of M)
  size_t part_bytes;                       // forward partials
  size_t g_bytes, wpart_bytes, bpart_bytes, gemm_bytes;   // backward
  size_t total;
};

LcetPlan lcet_plan(int M, int K1, int K2, int C) {
  LcetPlan pl;
  pl.ldg = (C + 3) & ~3;
  long sr = (long)(LCET_SLAB_BYTES) / ((long)pl.ldg * 4) / 64 * 64;
  if (sr < 64) sr = 64;
  pl.slab_rows = sr < M ? (int)sr : M;
  pl.part_bytes = up256((size_t)key_split_plan(M, C, LT_ROWS).ksplit * M * 5 * sizeof(float));
  pl.g_bytes = up256((size_t)pl.slab_rows * pl.ldg * sizeof(float));
  const int scap = lce_wgrad_split_cap(pl.slab_rows, K1 + K2, C);       // holds for the shorter last slab too
  pl.wpart_bytes = up256((size_t)scap * C * (K1 + K2) * sizeof(float));
  pl.bpart_bytes = up256((size_t)scap * C * sizeof(float));
  // dX: the split workspace of the skinny form (<= 64 rows), for a full slab and for the shorter last one
  const int last = M % pl.slab_rows ? M % pl.slab_rows : pl.slab_rows;
  size_t gw = 0;
  for (int rows : {pl.slab_rows, last}) {
    const size_t w1 = clipk_gemm_f32_workspace(rows, K1, C, 0, 1);
    const size_t w2 = K2 ? clipk_gemm_f32_workspace(rows, K2, C, 0, 1) : 0;
    gw = gw > w1 ? gw : w1;
    gw = gw > w2 ? gw : w2;
  }
  pl.gemm_bytes = up256(gw);
  const size_t bwd = pl.g_bytes + pl.wpart_bytes + pl.bpart_bytes + pl.gemm_bytes;
  pl.total = bwd > pl.part_bytes ? bwd : pl.part_bytes;
  return pl;
}

}  // namespace

extern "C" size_t clipk_linear_ce_tiled_workspace(int M, int K1, int K2, int C) {
  if (lce_check(M, K1, K2, C, LT_MAX_C) != CLIPK_OK) return 0;
  return lcet_plan(M, K1, K2, C).total;
}

extern "C" int clipk_linear_ce_tiled_fwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                         const int64_t* labels, int M, int C, float* lse, float* tgt, int64_t* pred,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = lce_check(M, K1, K2, C, LT_MAX_C);
  if (rc != CLIPK_OK) return rc;
  if (!X1 || !W || (K2 > 0) != (X2 != nullptr) || (tgt && !labels)) return CLIPK_ERR_BAD_ARG;
  if (!lse && !tgt && !pred) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X1) || !aligned16(X2) || !aligned16(W) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  const LcetPlan pl = lcet_plan(M, K1, K2, C);
  if (!workspace || workspace_bytes < pl.part_bytes) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const KeySplitPlan g = key_split_plan(M, C, LT_ROWS);   // one workgroup per (64-row block, class split)
  TP p{};
  p.X1 = X1; p.X2 = X2; p.W = W; p.bias = bias; p.labels = labels;
  p.M = M; p.K1 = K1; p.K2 = K2; p.C = C;
  p.tiles_per_split = g.tiles_per_split; p.ntiles = g.ntiles;
  p.part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(lcet_rows_kernel<false>, dim3((unsigned)g.nqb, (unsigned)g.ksplit), dim3(256), 0, st, p);
  int e = clipk_check_launch();
  if (e != CLIPK_OK) return e;
  hipLaunchKernelGGL(lcet_finalize_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, p.part, g.ksplit, M, C, labels, lse,
                     tgt, pred);
  return clipk_check_launch();
}

extern "C" int clipk_linear_ce_tiled_bwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                         const int64_t* labels, int M, int C, const float* lse, const float* g,
                                         int accumulate, float* dW, float* dbias, float* dX1, float* dX2, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  const int rc = lce_check(M, K1, K2, C, LT_MAX_C);
  if (rc != CLIPK_OK) return rc;
  if (!lce_bwd_args_ok(X1, X2, K2, W, labels, lse, g, dW, dbias, dX1, dX2, workspace)) return CLIPK_ERR_BAD_ARG;
  const LcetPlan pl = lcet_plan(M, K1, K2, C);
  if (workspace_bytes < pl.g_bytes + pl.wpart_bytes + pl.bpart_bytes + pl.gemm_bytes) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  float* G = reinterpret_cast<float*>(ws);
  float* wpart = reinterpret_cast<float*>(ws + pl.g_bytes);
  float* bpart = reinterpret_cast<float*>(ws + pl.g_bytes + pl.wpart_bytes);
  void* gemm_ws = pl.gemm_bytes ? ws + pl.g_bytes + pl.wpart_bytes + pl.bpart_bytes : nullptr;

  for (long s0 = 0; s0 < M; s0 += pl.slab_rows) {
    const int rows = (int)(M - s0 < pl.slab_rows ? M - s0 : pl.slab_rows);
    const float* x1 = X1 + s0 * K1;
    const float* x2 = X2 ? X2 + s0 * K2 : nullptr;
    const KeySplitPlan gr = key_split_plan(rows, C, LT_ROWS);   // (G has no cross-split sum: its bits do not depend on the grid)
    TP p{};
    p.X1 = x1; p.X2 = x2; p.W = W; p.bias = bias; p.labels = labels + s0;
    p.M = rows; p.K1 = K1; p.K2 = K2; p.C = C;
    p.tiles_per_split = gr.tiles_per_split; p.ntiles = gr.ntiles;
    p.lse = lse + s0; p.g = g; p.m_total = (float)M; p.G = G; p.ldg = pl.ldg;
    hipLaunchKernelGGL(lcet_rows_kernel<true>, dim3((unsigned)gr.nqb, (unsigned)gr.ksplit), dim3(256), 0, st, p);
    int e = clipk_check_launch();
    if (e != CLIPK_OK) return e;
    LceW w{};
    w.X1 = x1; w.X2 = x2; w.G = G; w.part = wpart; w.bpart = bpart;
    w.M = rows; w.K1 = K1; w.K2 = K2; w.C = C; w.ldg = pl.ldg;
    e = lce_bwd_tail<true>(w, W, accumulate || s0 > 0, dW, dbias, dX1 ? dX1 + s0 * K1 : nullptr, dX2 ? dX2 + s0 * K2 : nullptr,
                           gemm_ws, pl.gemm_bytes, stream);
    if (e != CLIPK_OK) return e;
  }
  return CLIPK_OK;
}
