// simce_tiled.hip — second-generation LSE pass of the fused similarity + cross-entropy (simce.hip has the contract).
//
// The first kernel gives one workgroup 32 queries and lets its waves split the contraction dimension P: every 32-key
// tile then costs a synchronous staging step, a cross-wave reduction through LDS and two barriers, and only one wave
// does the softmax — 102 us for one rank's config-3 block (512 x 4096 x 512), 16 TFLOP/s of exact-f32 matrix work.
// This one is the tiled exact-f32 GEMM of gemm_f32.hip with the softmax statistics as its epilogue:
//   * a workgroup owns 64 queries and walks 64-key tiles; per tile the 64 x 64 block of S^T = Y X^T is a BK = 16 K-loop
//     over P with register-staged double buffering (keys are the MFMA rows, queries the lanes), 4 waves = 2 (keys) x 2
//     (queries), one 32 x 32 accumulator each: nothing crosses waves inside a tile;
//   * each lane keeps the running (max, sum) of its query over the key rows it sees (16 per tile) in registers; the two
//     lane halves and the two key-waves are merged once, at the end (one lane^32 exchange, one LDS hop);
//   * key-range splits write (m, l) partials that simce_lse_finalize merges in a fixed order, as before.
// Numerics: the same k-ordered f32 fmaf chains per logit (the MFMA's arithmetic), a different but fixed summation order
// of the exponentials; deterministic.
//
// Class-aware instantiation (CLS = true, include/clipk.h: clipk_simce_lse_cls / clipk_simce_grad_cls): the same tiles
// with class ids on the pairs.  A lane loads the ids of its 16 key rows once per tile, before the tile's K-loop; keys of
// the query's class other than its diagonal enter the running (max, sum) as -inf ("mask"), and the sums the target needs
// (S over the denominator set, S over the same-class keys, their count) are kept next to (m, l) and merged in the same
// fixed order.  CLS = false is the plain kernel: every class-aware line sits under `if constexpr`.
//
// What is shared, and where: the walk over the batch-plus-cache key list is cloud_tile.h's KeyWalk<BKT, true>, the grid
// its key_split_plan; the gradient pass's second product and slab store are key_sum_tile.h's weighted key sum; the
// operand block, its host filler, the batched launches' re-basing, the class-id fetch, the d scale merge and the launch
// are simce_tile.h's, which simce_hard.hip's kernels take too.  The statistics, the G formula, the merges and the partial
// formats below are this file's own.
#include "common.h"
#include "simce_tile.h"

namespace {

// a * b as one rounded f32 product, never the first half of a contracted fma
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

struct LP {
  float* part_ml;      // [ksplit][Mx][2]
  float* pos;          // [Mx]
  // class-aware instantiation only
  int same_positive;                            // 0: same-class keys leave the denominator ("mask"), 1: they stay
  float* part_t;                                // [ksplit][Mx][3]: sum_{D_i} S, sum_{same} S, #same
  SimceOps o;
};

// ZB (with CLS): the batched launch, blockIdx.z = problem of o.z; the single-problem instantiations have none of its code
template <bool CLS, bool ZB = false>
__global__ __launch_bounds__(256, 2) void simce_lse_tiled_kernel(const LP pa) {
  LP p = pa;
  if constexpr (ZB) {                                                     // this workgroup's problem
    const long zs = simce_rebase(p.o, pa.o.z);
    p.part_ml += zs * 2; p.part_t += zs * 3; p.pos += (long)blockIdx.z * p.o.Mx;
  }
  const SimceOps& o = p.o;
  constexpr int BKL = 32;                                                 // 16 MFMAs per wave between barriers
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (BKL + 4)];   // 2 buffers x (keys | queries)
  __shared__ float mrg[2][CLS ? 5 : 2][TQ];                               // [key-wave][m | l (| sd | ss | c)][query]
  const float scale = o.scale[0];
  const KeyWalk<BKL, true> w(o.X, o.Mx, nullptr, o.Mx, o.Y, o.Ny, o.P, o.tiles_per_split, o.ntiles, smem, o.Yc, o.Nc);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;   // qg: this lane's query
  const int Nkeys = w.Nk;
  const int label = o.label_offset + qg;
  float m_run = -INFINITY, l_run = 0.f, pos_v = 0.f;
  bool pos_hit = false;
  float sd = 0.f, ss = 0.f, cnt = 0.f;                                    // CLS: sum_{D} S, sum_{same} S, #same
  int64_t cq = 0;
  if constexpr (CLS) {
    if (o.cls_x) cq = o.cls_x[qg < o.Mx ? qg : o.Mx - 1];
  }

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    int64_t ck[16];                                                       // CLS: ids of this lane's 16 key rows
    if constexpr (CLS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ck[r] = simce_key_class(o.cls_y, w.key(j0, r), o.Ny, cq);
    }
    f32x16 acc;
    w.product(j0, acc);
    // ---- softmax statistics of this lane's query over its 16 key rows of the tile
    float sv[16], tmax = -INFINITY;
    if constexpr (CLS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = w.key(j0, r);
        const float s = scale * acc[r];
        const bool diag = key == label && key < o.Ny;
        const bool same = diag || ck[r] == cq;
        const bool in_d = key < Nkeys && (p.same_positive || !same || diag);
        sv[r] = in_d ? s : -INFINITY;
        tmax = fmaxf(tmax, sv[r]);
        if (diag) { pos_v = s; pos_hit = true; }
        sd += in_d ? s : 0.f;
        ss += same ? s : 0.f;
        cnt += same ? 1.f : 0.f;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = w.key(j0, r);
        sv[r] = key < Nkeys ? scale * acc[r] : -INFINITY;
        tmax = fmaxf(tmax, sv[r]);
        if (key == label && key < o.Ny) { pos_v = sv[r]; pos_hit = true; }
      }
    }
    if (tmax > -INFINITY) {
      const float m_new = fmaxf(m_run, tmax);
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += expf(sv[r] - m_new);             // exp(-inf) = 0 for masked keys
      l_run = l_run * expf(m_run - m_new) + a;
      m_run = m_new;
    }
  }

  // ---- merge: lane halves, then the two key-waves
  {
    const float m_o = __shfl_xor(m_run, 32, 64), l_o = __shfl_xor(l_run, 32, 64);
    const float m_n = fmaxf(m_run, m_o);
    float l_n = 0.f;
    if (m_n > -INFINITY) l_n = l_run * expf(m_run - m_n) + l_o * expf(m_o - m_n);
    m_run = m_n; l_run = l_n;
  }
  if constexpr (CLS) {
    sd += __shfl_xor(sd, 32, 64); ss += __shfl_xor(ss, 32, 64); cnt += __shfl_xor(cnt, 32, 64);
  }
  if (pos_hit && qg < o.Mx) p.pos[qg] = pos_v;                            // exactly one lane of the grid holds it
  if (h == 0) { mrg[wm][0][wn * 32 + li] = m_run; mrg[wm][1][wn * 32 + li] = l_run; }
  if constexpr (CLS) {
    if (h == 0) { mrg[wm][2][wn * 32 + li] = sd; mrg[wm][3][wn * 32 + li] = ss; mrg[wm][4][wn * 32 + li] = cnt; }
  }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < o.Mx) {
    const float m1 = mrg[1][0][wn * 32 + li], l1 = mrg[1][1][wn * 32 + li];
    const float m_n = fmaxf(m_run, m1);
    float l_n = 0.f;
    if (m_n > -INFINITY) l_n = l_run * expf(m_run - m_n) + l1 * expf(m1 - m_n);
    float* out = p.part_ml + ((long)ks * o.Mx + qg) * 2;
    out[0] = m_n; out[1] = l_n;
    if constexpr (CLS) {
      float* t = p.part_t + ((long)ks * o.Mx + qg) * 3;
      t[0] = sd + mrg[1][2][wn * 32 + li]; t[1] = ss + mrg[1][3][wn * 32 + li]; t[2] = cnt + mrg[1][4][wn * 32 + li];
    }
  }
}

// ------------------------------------------------------------------------------------------------ gradient pass
// dX[q, :] = sum_key G[q, key] Y[key, :] with G = dL/dS formed from the two LSE vectors (simce.hip has the formula).
// Same 64 x 64 tiles: (1) S^T tile by the K-loop over P; (2) G in the accumulator layout (keys on rows, queries on
// lanes), written once to a 16 KiB LDS tile; (3) dX^T[p, q] += Y^T[p, key] G^T[key, q] by key_sum_tile.h's weighted key
// sum: a second MFMA product whose M dimension is p, wave w owning p in [w P/4, (w+1) P/4) for all 64 queries (up to 8
// accumulators); the key tile comes back from L2 in four 16-key blocks [16][P] staged in LDS (A operand: Y[key][p], one
// ds_read_b32 per MFMA, conflict free), G^T is the B operand straight from the LDS tile.  70 KiB of LDS and < 256 VGPRs:
// TWO workgroups per CU, so one's staging latencies sit under the other's MFMAs (with 64 KiB key halves and one
// workgroup per CU the same kernel took 79 us instead of the figure in DESIGN.md).  P <= KEYSUM_PMAX = 512 (128
// accumulator registers); larger P keeps the first-generation kernel.  Key-range splits write dX slabs that
// simce_grad_finalize sums in a fixed order.
struct GP2 {
  const float* lse_x; const float* lse_y;
  float w_row, w_col, inv_bg;
  const float* upstream;   // device scalar multiplied into inv_bg, or null
  float* slab;         // [ksplit][Mx][P]
  float* dsc_part;     // [ksplit][Mx]
  // class-aware instantiation only
  const float* cnt_x; const float* cnt_y;       // same-class counts c of the queries / of the keys (null: w = 0 side)
  int same_positive;
  float eps;
  float nkeys_y;                                // key count of the column direction (its denominator before masking)
  // batched launch: lse_x = lse_y = lse [nz][Mx], cnt_x = cnt_y = cnt [nz][Mx], upstream [nz] (or null), slab and
  // dsc_part hold the problems one after another
  SimceOps o;
};

template <bool CLS, bool ZB = false>
__global__ __launch_bounds__(256, 2) void simce_grad_tiled_kernel(const GP2 pa) {
  GP2 p = pa;
  if constexpr (ZB) {                                                     // this workgroup's problem
    const int z = blockIdx.z, r = pa.o.z.rev[z];
    const long zs = simce_rebase(p.o, pa.o.z);
    p.lse_x = pa.lse_x + (long)z * p.o.Mx; p.lse_y = pa.lse_x + (long)r * p.o.Mx;   // the keys' LSE: the reverse problem's
    p.cnt_x = pa.cnt_x + (long)z * p.o.Mx; p.cnt_y = pa.cnt_x + (long)r * p.o.Mx;
    if (pa.upstream) p.upstream = pa.upstream + z;
    p.slab += zs * p.o.P; p.dsc_part += zs;
  }
  const SimceOps& o = p.o;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                      // K-loop buffers
  float* gl = smem + KLOOP_LDS_FLOATS;                                    // G tile [64 keys][64 queries]
  float* yh = gl + TK * TQ;                                               // key block [16][YH_LD] / output transposes
  float* dsl = yh + KSB * YH_LD;                                          // [64 queries] dscale partials of key-wave 1
  const float scale = o.scale[0];
  const KeyWalk<BKG, true> w(o.X, o.Mx, nullptr, o.Mx, o.Y, o.Ny, o.P, o.tiles_per_split, o.ntiles, smem, o.Yc, o.Nc);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, qg = w.qg;
  const int Nkeys = w.Nk;
  const int label = o.label_offset + qg;
  const float lse_xi = p.lse_x[qg < o.Mx ? qg : o.Mx - 1];
  const float ibg = p.upstream ? p.inv_bg * p.upstream[0] : p.inv_bg;
  f32x16 dx[4][2];
  key_sum_zero(dx);
  float dsc = 0.f;
  int64_t cq = 0;                                 // CLS: the query's id, 1 / c_i, eps / N_i
  float inv_cx = 1.f, eps_nx = 0.f;
  if constexpr (CLS) {
    const int qc = qg < o.Mx ? qg : o.Mx - 1;
    if (o.cls_x) cq = o.cls_x[qc];
    const float cx = p.cnt_x ? p.cnt_x[qc] : 1.f;
    inv_cx = 1.f / cx;
    eps_nx = p.eps / (p.same_positive ? (float)Nkeys : (float)Nkeys - (cx - 1.f));
  }

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    f32x16 acc;
    w.product(j0, acc);                                                   // (its first barrier also frees gl / yh)
    // ---- G (accumulator layout: rows = keys, lanes = queries) -> LDS tile gl[key][query]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = wm * 32 + keyrow32(r, h);
      const int key = j0 + kl;
      const float sv = scale * acc[r];
      float gv = 0.f;
      if constexpr (CLS) {
        // w_row ([j in D_i] P_row - T[i,j]) + w_col ([i in D'_j] P_col - T'[j,i]); `same` is symmetric, so is D
        if (key < Nkeys && qg < o.Mx) {
          const bool kin = key < o.Ny;
          const bool diag = kin && key == label;
          const bool same = diag || (kin && o.cls_y && o.cls_y[key] == cq);
          const bool in_d = p.same_positive || !same || diag;
          const float hard = p.same_positive ? (same ? inv_cx : 0.f) : (diag ? 1.f : 0.f);
          // batched launch: the logit ROUNDED, as the LSE pass saw it, so that a row whose denominator is its own key
          // alone (lse = that logit) gets exp(0) - 1 = 0 exactly; in the single-problem instantiation the compiler
          // contracts scale * acc - lse (an unrounded product: 2e-9 in dX for such a row), and its bits are pinned
          const float sl = ZB ? mul_rounded(scale, acc[r]) : sv;
          gv = p.w_row * ((in_d ? expf(sl - lse_xi) : 0.f) - ((1.f - p.eps) * hard + (in_d ? eps_nx : 0.f)));
          if (kin) {
            const float cy = p.cnt_y ? p.cnt_y[key] : 1.f;
            const float hy = p.same_positive ? (same ? 1.f / cy : 0.f) : (diag ? 1.f : 0.f);
            const float ny = p.same_positive ? p.nkeys_y : p.nkeys_y - (cy - 1.f);
            gv += p.w_col * ((in_d ? expf(sl - p.lse_y[key]) : 0.f) - ((1.f - p.eps) * hy + (in_d ? p.eps / ny : 0.f)));
          }
          gv *= ibg;
        }
      } else {
        if (key < Nkeys && qg < o.Mx) {
          gv = p.w_row * expf(sv - lse_xi);
          if (key < o.Ny) {
            gv += p.w_col * expf(sv - p.lse_y[key]);
            if (key == label) gv -= (p.w_row + p.w_col);
          }
          gv *= ibg;
        }
      }
      dsc += gv * acc[r];
      gl[kl * TQ + wn * 32 + li] = gv;
    }
    key_sum_tile<true>(dx, o.Y, o.Ny, o.P, j0, gl, yh, w.tid, w.wid, li, h, o.Yc, Nkeys);   // dX^T += Y^T G^T
  }

  // ---- dX^T accumulators -> [q][p] rows of this split's slab, whole 128-B row segments; then the d scale partial
  __syncthreads();
  key_sum_store(dx, yh, p.slab, o.Mx, o.P, w.q0, w.ks, w.wid, li, h);
  simce_dscale_merge(dsc, dsl, p.dsc_part, w.ks, o.Mx, qg, wm, wn, li, h);
}

// what every gradient launch fills besides the operand block and the class-aware fields
GP2 grad_args(const float* lse_x, const float* lse_y, float w_row, float w_col, float inv_bg, const float* upstream,
              float* slab, float* dsc_part) {
  GP2 p{};
  p.lse_x = lse_x; p.lse_y = lse_y; p.w_row = w_row; p.w_col = w_col; p.inv_bg = inv_bg; p.upstream = upstream;
  p.slab = slab; p.dsc_part = dsc_part;
  return p;
}

constexpr size_t GRAD_LDS_BYTES = (size_t)SIMCE_GRAD_LDS_FLOATS * sizeof(float);

}  // namespace

extern "C" int clipk_simce_grad_tiled_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc,
                                             int P, const float* scale, int label_offset, const float* lse_x,
                                             const float* lse_y, float w_row, float w_col, float inv_bg,
                                             const float* upstream, float* slab, float* dsc_part, void* stream) {
  if (P > KEYSUM_PMAX) return CLIPK_ERR_UNSUPPORTED;
  const KeySplitPlan k = key_split_plan(Mx, Ny + Nc, TQ);
  GP2 p = grad_args(lse_x, lse_y, w_row, w_col, inv_bg, upstream, slab, dsc_part);
  p.o = simce_ops(X, Mx, Y, Ny, Yc, Nc, P, scale, label_offset, nullptr, nullptr, k);
  return simce_launch<simce_grad_tiled_kernel<false>>(p, k, 1, GRAD_LDS_BYTES, stream);
}

extern "C" int clipk_simce_grad_tiled_cls_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc,
                                                 int P, const float* scale, int label_offset, const float* lse_x,
                                                 const float* lse_y, const float* cnt_x, const float* cnt_y,
                                                 const int64_t* cls_x, const int64_t* cls_y, int same_positive,
                                                 float eps, int nkeys_y, float w_row, float w_col, float inv_bg,
                                                 const float* upstream, float* slab, float* dsc_part, void* stream) {
  if (P > KEYSUM_PMAX) return CLIPK_ERR_UNSUPPORTED;
  const KeySplitPlan k = key_split_plan(Mx, Ny + Nc, TQ);
  GP2 p = grad_args(lse_x, lse_y, w_row, w_col, inv_bg, upstream, slab, dsc_part);
  p.o = simce_ops(X, Mx, Y, Ny, Yc, Nc, P, scale, label_offset, cls_x, cls_y, k);
  p.cnt_x = cnt_x; p.cnt_y = cnt_y; p.same_positive = same_positive; p.eps = eps; p.nkeys_y = (float)nkeys_y;
  return simce_launch<simce_grad_tiled_kernel<true>>(p, k, 1, GRAD_LDS_BYTES, stream);
}

extern "C" int clipk_simce_lse_tiled_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                                            const float* scale, int label_offset, float* part_ml, float* pos,
                                            void* stream) {
  const KeySplitPlan k = key_split_plan(Mx, Ny + Nc, TQ);
  LP p{};
  p.o = simce_ops(X, Mx, Y, Ny, Yc, Nc, P, scale, label_offset, nullptr, nullptr, k);
  p.part_ml = part_ml; p.pos = pos;
  return simce_launch<simce_lse_tiled_kernel<false>>(p, k, 1, 0, stream);
}

// pos: S[i, label(i)] lands here (the class-aware finalize turns it into the target); part_t: [ksplit][Mx][3]
extern "C" int clipk_simce_lse_tiled_cls_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc,
                                                int P, const float* scale, int label_offset, const int64_t* cls_x,
                                                const int64_t* cls_y, int same_positive, float* part_ml, float* part_t,
                                                float* pos, void* stream) {
  const KeySplitPlan k = key_split_plan(Mx, Ny + Nc, TQ);
  LP p{};
  p.o = simce_ops(X, Mx, Y, Ny, Yc, Nc, P, scale, label_offset, cls_x, cls_y, k);
  p.part_ml = part_ml; p.pos = pos; p.same_positive = same_positive; p.part_t = part_t;
  return simce_launch<simce_lse_tiled_kernel<true>>(p, k, 1, 0, stream);
}

// ---- batched class-aware launches (clipk_simce_{lse,grad}_pairs_cls): zt.nz problems of shape B x B over zt.E, the
// splits of key_split_plan for the whole grid; per-problem outputs and partials follow one another
extern "C" int clipk_simce_lse_tiled_pairs_cls_launch(const PairZ* zt, int B, int P, const float* scale, int same_positive,
                                                      float* part_ml, float* part_t, float* pos, void* stream) {
  const KeySplitPlan k = key_split_plan(B, B, TQ, zt->nz);
  LP p{};
  p.o = simce_ops(nullptr, B, nullptr, B, nullptr, 0, P, scale, 0, nullptr, nullptr, k, zt);
  p.part_ml = part_ml; p.part_t = part_t; p.pos = pos; p.same_positive = same_positive;
  return simce_launch<simce_lse_tiled_kernel<true, true>>(p, k, zt->nz, 0, stream);
}

extern "C" int clipk_simce_grad_tiled_pairs_cls_launch(const PairZ* zt, int B, int P, const float* scale, const float* lse,
                                                       const float* cnt, int same_positive, float eps, float w_row,
                                                       float w_col, float inv_bg, const float* upstream, float* slab,
                                                       float* dsc_part, void* stream) {
  if (P > KEYSUM_PMAX) return CLIPK_ERR_UNSUPPORTED;
  const KeySplitPlan k = key_split_plan(B, B, TQ, zt->nz);
  GP2 p = grad_args(lse, lse, w_row, w_col, inv_bg, upstream, slab, dsc_part);
  p.o = simce_ops(nullptr, B, nullptr, B, nullptr, 0, P, scale, 0, nullptr, nullptr, k, zt);
  p.cnt_x = cnt; p.cnt_y = cnt; p.same_positive = same_positive; p.eps = eps; p.nkeys_y = (float)B;
  return simce_launch<simce_grad_tiled_kernel<true, true>>(p, k, zt->nz, GRAD_LDS_BYTES, stream);
}
