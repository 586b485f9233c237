// linear_ce_tiled.hip — Linear(K, C) + cross-entropy against integer labels for ANY class count (include/clipk.h:
// clipk_linear_ce_tiled_*).  linear_ce.hip keeps a row's whole logit vector in at most four 16-class accumulator tiles and
// stops at C = 64; the reference's own probes are far wider (run1/proposal.MD:3: 2,547 immune cell types and 158 markers;
// old/ablation.py:51 and old/classifier.py take num_classes as a free argument).  Here the classes are walked in tiles:
//
//   lcet_rows_kernel<false>   forward: a workgroup owns 64 rows of [X1|X2] and walks 64-class tiles of W with the exact-f32
//                             64 x 64 tile of sim_tile.h (classes on the MFMA rows, X rows on the lanes; the two sources
//                             are two s_tile calls into one accumulator).  Each lane keeps (m, l, best value, best class,
//                             target logit) of its row; lane halves and the two class-waves merge at the end.  Class-range
//                             splits (the plan of clipk_simce_tiled_plan) fill the chip when M is small.
//   lcet_finalize_kernel      the splits' partials [split][M][5] merged in split order -> lse, tgt, pred
//   lcet_rows_kernel<true>    backward, step 1: the same Z (same code, same bits), G = g/M (softmax - onehot) -> workspace,
//                             pitch C rounded up to 4 with zeros in the padding
//   lcet_wgrad_kernel         backward, step 2: dW partials = G^T [X1|X2] over row splits and 64-class groups, dbias
//                             partials alongside (the layout of lce_wgrad_kernel; why not clipk_gemm_f32: see there)
//   lcet_reduce_kernel        backward, step 3: the splits summed in split order (+ the old contents when accumulating)
//   dX = G W                  the tiled exact-f32 GEMM of gemm_f32.hip on G, one call per source (only when asked for)
// The backward walks the rows in slabs whose G stays below LCET_SLAB_BYTES, so that a slab's G is still in the Infinity
// Cache when its consumers read it; dW / dbias accumulate over the slabs in slab order.
// The argmax merge rule is "larger value, then lower class": associative, so any merge order gives the first occurrence.
// No atomics anywhere: a result depends on the shapes alone.
#include "common.h"
#include "sim_tile.h"
#include <math.h>

#ifndef LCET_SLAB_BYTES
#define LCET_SLAB_BYTES (128ll << 20)      // G bytes per backward slab (profiles/probe/README.md has the A/B)
#endif

namespace {

constexpr int LT_ROWS = 64, LT_CLS = 64;   // X rows per workgroup, classes per tile
constexpr int LT_BK = 32;                  // K-step of the tile: 16 MFMAs per wave between barriers
constexpr int LT_NF = LT_BK / 16;          // staging float4s per thread and operand
constexpr int LT_NONE = 0x7fffffff;        // "no class seen yet": loses every tie
constexpr int LT_TARGET_WGS = 512;         // two workgroups per CU
constexpr int LT_WCOLS = 64;               // dW columns per wave of lcet_wgrad_kernel
constexpr int LT_MIN_SPLIT_ROWS = 256;     // rows per split at least: the partials stay a fraction of the X traffic
constexpr int LT_MAX_C = 65536;

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
  int bc = LT_NONE;
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
        if (cv && (z[r] > bv || bc == LT_NONE)) { bv = z[r]; bc = cls; }
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
      if (bv_o > bv || (bv_o == bv && bc_o < bc)) { bv = bv_o; bc = bc_o; }
      tg += tg_o;                                                                 // one non-zero term at most
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
    const float m_o = o[0], l_o = o[1], bv_o = o[2];
    const int bc_o = __float_as_int(o[3]);
    const float m_n = fmaxf(m, m_o);
    float l_n = 0.f;
    if (m_n > -INFINITY) l_n = l * expf(m - m_n) + l_o * expf(m_o - m_n);
    m = m_n; l = l_n;
    if (bv_o > bv || (bv_o == bv && bc_o < bc)) { bv = bv_o; bc = bc_o; }
    tg += o[4];
  }
  if (lse) lse[row] = m + logf(l);
  if (tgt) {
    const long lab = (long)labels[row];
    tgt[row] = (lab >= 0 && lab < C) ? tg : NAN;
  }
  if (pred) pred[row] = bc == LT_NONE ? 0 : bc;
}

struct TW {
  const float *X1, *X2, *G;
  float *part, *bpart;                     // [S][C][K], [S][C]
  int M, K1, K2, C, ldg, rows_per_split;   // M: rows of this launch (a slab)
};

__device__ __forceinline__ f32x4 lcet_x4(const float* X1, const float* X2, int K1, int K2, long row, int k) {
  const float* s = k < K1 ? X1 + row * K1 + k : X2 + row * K2 + (k - K1);
  return *reinterpret_cast<const f32x4*>(s);
}

// dW[c][k] = sum_i G[i][c] X[i][k]: the rows are the contraction, so the grid splits them (clipk_gemm_f32 has no split of
// its contraction: at C = 158 it left 24 workgroups walking 131072 rows each).  The layout of lce_wgrad_kernel
// (linear_ce.hip) with a class-group dimension: a wave owns 64 classes x 64 columns of dW for one row split, on
// v_mfma_f32_16x16x4_f32 straight from global memory; a lane's float4 of X supplies the B operand of four MFMAs, so MFMA
// j holds columns {kc + 4 n + j}.  dbias partials come from the same A registers.
__global__ __launch_bounds__(256) void lcet_wgrad_kernel(const TW p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int K = p.K1 + p.K2, C = p.C;
  const int kc = (blockIdx.x * 4 + wave) * LT_WCOLS;
  if (kc >= K) return;                                       // (wave-uniform; no barrier in this kernel)
  const int s = blockIdx.y, cg = blockIdx.z * 64;
  const int nct = (C - cg + 15) / 16 < 4 ? (C - cg + 15) / 16 : 4;      // class tiles of this group that hold classes
  const long i0 = (long)s * p.rows_per_split;
  const long i1 = (i0 + p.rows_per_split < p.M) ? i0 + p.rows_per_split : (long)p.M;
  const int kq = kc + 4 * r;
  const bool kv = kq < K;
  const bool do_bias = p.bpart && blockIdx.x == 0 && wave == 0;

  f32x4 acc[4][4];
  float bs[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    bs[ct] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (long i = i0; i < i1; i += 4) {
    const long row = i + q;
    const bool rv = row < i1;
    float a[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)                           // (below the pitch: the padding holds zeros)
      a[ct] = (rv && cg + ct * 16 + r < p.ldg) ? p.G[row * p.ldg + cg + ct * 16 + r] : 0.f;
    const f32x4 x = (rv && kv) ? lcet_x4(p.X1, p.X2, p.K1, p.K2, row, kq) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
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
    for (int ct = 0; ct < 4; ++ct)
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
    for (int ct = 0; ct < 4; ++ct) {
      float v = bs[ct];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int cls = cg + ct * 16 + r;
      if (q == 0 && cls < C) p.bpart[(long)s * C + cls] = v;
    }
  }
}

// out (+)= sum_s part[s], s ascending; the fresh sum has the same bits with and without accumulate
__global__ __launch_bounds__(256) void lcet_reduce_kernel(const float* part, const float* bpart, int S, int C, int K, float* dW,
                                                          float* db, int accumulate) {
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
    for (int s = 1; s < S; ++s) v += bpart[(long)s * C + c];
    db[c] = accumulate ? db[c] + v : v;
  }
}

// ---- host side
int lcet_check(int M, int K1, int K2, int C) {
  if (M <= 0 || C <= 0 || K1 <= 0 || K2 < 0) return CLIPK_ERR_BAD_ARG;
  if (C > LT_MAX_C || (K1 & 3) || (K2 & 3) || (long)K1 + K2 > 4096) return CLIPK_ERR_UNSUPPORTED;
  return CLIPK_OK;
}

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// one workgroup per (64-row block, class split); splits so that the grid holds about two workgroups per CU
struct LcetGrid { int nrb, S, tps, ntiles; };
LcetGrid lcet_grid(int rows, int C) {
  LcetGrid g;
  g.nrb = (rows + LT_ROWS - 1) / LT_ROWS;
  g.ntiles = (C + LT_CLS - 1) / LT_CLS;
  int ks = (LT_TARGET_WGS + g.nrb - 1) / g.nrb;
  if (ks > g.ntiles) ks = g.ntiles;
  if (ks < 1) ks = 1;
  g.tps = (g.ntiles + ks - 1) / ks;
  g.S = (g.ntiles + g.tps - 1) / g.tps;
  return g;
}

struct LcetPlan {
  int ldg, slab_rows;                      // G pitch; rows per backward slab (a multiple of 64, or all of M)
  size_t part_bytes;                       // forward partials
  size_t g_bytes, wpart_bytes, bpart_bytes, gemm_bytes;   // backward
  size_t total;
};

// row splits of lcet_wgrad_kernel: about LT_TARGET_WGS workgroups over (column blocks, class groups, splits).
// lcet_wgrad_split_cap bounds S for every row count up to `rows` (rows_per_split >= rows / cap, so S <= cap; the
// rounding of rows_per_split to 4 can leave a long slab BELOW the cap that a shorter one reaches).
int lcet_wgrad_split_cap(int rows, int K, int C) {
  const int nwg = ((K + 4 * LT_WCOLS - 1) / (4 * LT_WCOLS)) * ((C + 63) / 64);
  const int s = (rows + LT_MIN_SPLIT_ROWS - 1) / LT_MIN_SPLIT_ROWS;
  const int smax = LT_TARGET_WGS / nwg > 1 ? LT_TARGET_WGS / nwg : 1;
  return s < smax ? s : smax;
}
void lcet_wgrad_splits(int rows, int K, int C, int* S, int* rows_per_split) {
  const int s = lcet_wgrad_split_cap(rows, K, C);
  long rps = ((long)rows + s - 1) / s;
  rps = (rps + 3) / 4 * 4;
  *rows_per_split = (int)rps;
  *S = (int)(((long)rows + rps - 1) / rps);
}

LcetPlan lcet_plan(int M, int K1, int K2, int C) {
  LcetPlan pl;
  pl.ldg = (C + 3) & ~3;
  long sr = (long)(LCET_SLAB_BYTES) / ((long)pl.ldg * 4) / 64 * 64;
  if (sr < 64) sr = 64;
  pl.slab_rows = sr < M ? (int)sr : M;
  pl.part_bytes = up256((size_t)lcet_grid(M, C).S * M * 5 * sizeof(float));
  pl.g_bytes = up256((size_t)pl.slab_rows * pl.ldg * sizeof(float));
  const int scap = lcet_wgrad_split_cap(pl.slab_rows, K1 + K2, C);       // holds for the shorter last slab too
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
  if (lcet_check(M, K1, K2, C) != CLIPK_OK) return 0;
  return lcet_plan(M, K1, K2, C).total;
}

extern "C" int clipk_linear_ce_tiled_fwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                         const int64_t* labels, int M, int C, float* lse, float* tgt, int64_t* pred,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = lcet_check(M, K1, K2, C);
  if (rc != CLIPK_OK) return rc;
  if (!X1 || !W || (K2 > 0) != (X2 != nullptr) || (tgt && !labels)) return CLIPK_ERR_BAD_ARG;
  if (!lse && !tgt && !pred) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X1) || !aligned16(X2) || !aligned16(W) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  const LcetPlan pl = lcet_plan(M, K1, K2, C);
  if (!workspace || workspace_bytes < pl.part_bytes) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const LcetGrid g = lcet_grid(M, C);
  TP p{};
  p.X1 = X1; p.X2 = X2; p.W = W; p.bias = bias; p.labels = labels;
  p.M = M; p.K1 = K1; p.K2 = K2; p.C = C;
  p.tiles_per_split = g.tps; p.ntiles = g.ntiles;
  p.part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(lcet_rows_kernel<false>, dim3((unsigned)g.nrb, (unsigned)g.S), dim3(256), 0, st, p);
  int e = clipk_check_launch();
  if (e != CLIPK_OK) return e;
  hipLaunchKernelGGL(lcet_finalize_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, p.part, g.S, M, C, labels, lse,
                     tgt, pred);
  return clipk_check_launch();
}

extern "C" int clipk_linear_ce_tiled_bwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                                         const int64_t* labels, int M, int C, const float* lse, const float* g,
                                         int accumulate, float* dW, float* dbias, float* dX1, float* dX2, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  const int rc = lcet_check(M, K1, K2, C);
  if (rc != CLIPK_OK) return rc;
  if (!X1 || !W || !labels || !lse || !g || (K2 > 0) != (X2 != nullptr) || (dX2 && K2 == 0)) return CLIPK_ERR_BAD_ARG;
  if (!dW && !dbias && !dX1 && !dX2) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X1) || !aligned16(X2) || !aligned16(W) || !aligned16(dW) || !aligned16(dX1) || !aligned16(dX2) ||
      !aligned16(workspace))
    return CLIPK_ERR_BAD_ARG;
  const LcetPlan pl = lcet_plan(M, K1, K2, C);
  if (!workspace || workspace_bytes < pl.g_bytes + pl.wpart_bytes + pl.bpart_bytes + pl.gemm_bytes) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int K = K1 + K2;
  char* ws = reinterpret_cast<char*>(workspace);
  float* G = reinterpret_cast<float*>(ws);
  float* wpart = reinterpret_cast<float*>(ws + pl.g_bytes);
  float* bpart = reinterpret_cast<float*>(ws + pl.g_bytes + pl.wpart_bytes);
  void* gemm_ws = pl.gemm_bytes ? ws + pl.g_bytes + pl.wpart_bytes + pl.bpart_bytes : nullptr;

  for (long s0 = 0; s0 < M; s0 += pl.slab_rows) {
    const int rows = (int)(M - s0 < pl.slab_rows ? M - s0 : pl.slab_rows);
    const int acc = (accumulate || s0 > 0) ? 1 : 0;
    const float* x1 = X1 + s0 * K1;
    const float* x2 = X2 ? X2 + s0 * K2 : nullptr;
    const LcetGrid gr = lcet_grid(rows, C);                  // (G has no cross-split sum: its bits do not depend on the grid)
    TP p{};
    p.X1 = x1; p.X2 = x2; p.W = W; p.bias = bias; p.labels = labels + s0;
    p.M = rows; p.K1 = K1; p.K2 = K2; p.C = C;
    p.tiles_per_split = gr.tps; p.ntiles = gr.ntiles;
    p.lse = lse + s0; p.g = g; p.m_total = (float)M; p.G = G; p.ldg = pl.ldg;
    hipLaunchKernelGGL(lcet_rows_kernel<true>, dim3((unsigned)gr.nrb, (unsigned)gr.S), dim3(256), 0, st, p);
    int e = clipk_check_launch();
    if (e != CLIPK_OK) return e;
    // dW (+)= G^T [X1|X2], dbias (+)= sum_i G: partials over row splits, then the splits in order
    if (dW || dbias) {
      TW w{};
      w.X1 = x1; w.X2 = x2; w.G = G; w.part = dW ? wpart : nullptr; w.bpart = dbias ? bpart : nullptr;
      w.M = rows; w.K1 = K1; w.K2 = K2; w.C = C; w.ldg = pl.ldg;
      int S;
      lcet_wgrad_splits(rows, K, C, &S, &w.rows_per_split);
      const dim3 grid((unsigned)((K + 4 * LT_WCOLS - 1) / (4 * LT_WCOLS)), (unsigned)S, (unsigned)((C + 63) / 64));
      hipLaunchKernelGGL(lcet_wgrad_kernel, grid, dim3(256), 0, st, w);
      e = clipk_check_launch();
      if (e != CLIPK_OK) return e;
      const long nthreads = (dW ? (long)C * K / 4 : 0) + (dbias ? C : 0);
      hipLaunchKernelGGL(lcet_reduce_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, wpart, bpart, S, C, K,
                         dW, dbias, acc);
      e = clipk_check_launch();
      if (e != CLIPK_OK) return e;
    }
    // dX = G W[:, source columns]: contraction over the C classes (G's padded columns are never read)
    if (dX1) {
      e = clipk_gemm_f32(G, pl.ldg, 0, W, K, 1, rows, K1, C, nullptr, nullptr, nullptr, 0, nullptr, dX1 + s0 * K1, K1, gemm_ws,
                         pl.gemm_bytes, stream);
      if (e != CLIPK_OK) return e;
    }
    if (dX2) {
      e = clipk_gemm_f32(G, pl.ldg, 0, W + K1, K, 1, rows, K2, C, nullptr, nullptr, nullptr, 0, nullptr, dX2 + s0 * K2, K2,
                         gemm_ws, pl.gemm_bytes, stream);
      if (e != CLIPK_OK) return e;
    }
  }
  return CLIPK_OK;
}
