// simce_hard.hip — hard-negative-weighted InfoNCE on the tiled similarity kernels (include/clipk.h:
// clipk_simce_lse_hard / clipk_simce_grad_hard has the definition; run1/full.py:347 names the variant,
// run1/configuration_hybrid_clip.py:105-106 its weight).
//
// The importance weights w_ij = exp(beta S_ij) / mean_{Neg_i} exp(beta S_ik) turn the negatives' mass into
//   log Ng_i = log n_i + C_i - A_i,   A_i = log sum_{Neg_i} exp(beta S),   C_i = log sum_{Neg_i} exp((1 + beta) S)
// so the LSE pass is simce_tiled.hip's pass with two sums in place of one, and the gradient pass is its pass with
//   g[i,j] = exp((1 + beta) s + k1_i) - exp(beta s + k2_i)      (k1, k2: per-row coefficients the LSE finalize leaves)
// per direction in place of exp(s - lse_i).  Same tiles (sim_tile.h), same merge order, no atomics: deterministic.
//
// These are kernels of their own and not a third instantiation of simce_tiled.hip's templates: the statistics, the G
// formula, the merge and the partial format differ.  What the two files share they take from the same headers: the walk
// over the batch-plus-cache key list (cloud_tile.h's KeyWalk<BKT, true>) and the grid (key_split_plan), the gradient
// pass's second product dX^T += Y^T G^T and its slab store (key_sum_tile.h), the operand block with its host filler and
// batched re-basing, the class-id fetch, the d scale merge and the launch (simce_tile.h).
//
// One running max serves both sums: beta >= 0 makes beta s and (1 + beta) s monotone in s, so m = max_{Neg} s bounds
// both exponents by 0 (A = beta m + log a, C = (1 + beta) m + log c, and C - A = m + log c - log a needs no beta).
#include "common.h"
#include "simce_tile.h"

namespace {

struct HLP {
  float beta;
  float* part;         // [ksplit][Mx][4]: m, a = sum exp(beta (s - m)), c = sum exp((1 + beta)(s - m)), n
  float* pos;          // [Mx]
  SimceOps o;
};

// (m, a, c) <- merge with (mo, ao, co); an empty side has m = -inf and zero sums (selected out: 0 * -inf at beta = 0)
__device__ __forceinline__ void hard_merge(float& m, float& a, float& c, float mo, float ao, float co, float beta,
                                           float b1) {
  const float mn = fmaxf(m, mo);
  const float d = m - mn, dn = mo - mn;
  const bool has = m > -INFINITY, has_o = mo > -INFINITY;
  const float an = (has ? a * expf(beta * d) : 0.f) + (has_o ? ao * expf(beta * dn) : 0.f);
  const float cn = (has ? c * expf(b1 * d) : 0.f) + (has_o ? co * expf(b1 * dn) : 0.f);
  m = mn; a = an; c = cn;
}

// ZB: the batched launch, blockIdx.z = problem of o.z; the single-problem instantiation has none of its code
template <bool ZB>
__global__ __launch_bounds__(256, 2) void simce_lse_hard_kernel(const HLP pa) {
  HLP p = pa;
  if constexpr (ZB) {                                                     // this workgroup's problem
    p.part += simce_rebase(p.o, pa.o.z) * 4; p.pos += (long)blockIdx.z * p.o.Mx;
  }
  const SimceOps& o = p.o;
  constexpr int BKL = 32;
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (BKL + 4)];   // 2 buffers x (keys | queries)
  __shared__ float mrg[4][TQ];                                            // key-wave 1's m | a | c | n per query
  const float scale = o.scale[0];
  const float beta = p.beta, b1 = 1.f + p.beta;
  const KeyWalk<BKL, true> w(o.X, o.Mx, nullptr, o.Mx, o.Y, o.Ny, o.P, o.tiles_per_split, o.ntiles, smem, o.Yc, o.Nc);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;   // qg: this lane's query
  const int Nkeys = w.Nk;
  const int label = o.label_offset + qg;
  float m_run = -INFINITY, a_run = 0.f, c_run = 0.f, cnt = 0.f, pos_v = 0.f;
  bool pos_hit = false;
  int64_t cq = 0;
  if (o.cls_x) cq = o.cls_x[qg < o.Mx ? qg : o.Mx - 1];

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    int64_t ck[16];                                                       // ids of this lane's 16 key rows
#pragma unroll
    for (int r = 0; r < 16; ++r) ck[r] = simce_key_class(o.cls_y, w.key(j0, r), o.Ny, cq);
    f32x16 acc;
    w.product(j0, acc);
    // ---- the negatives of this lane's query among its 16 key rows of the tile
    float sv[16], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = w.key(j0, r);
      const float s = scale * acc[r];
      const bool diag = key == label && key < o.Ny;
      const bool neg = key < Nkeys && !diag && ck[r] != cq;
      sv[r] = neg ? s : -INFINITY;
      tmax = fmaxf(tmax, sv[r]);
      if (diag) { pos_v = s; pos_hit = true; }
      cnt += neg ? 1.f : 0.f;
    }
    if (tmax > -INFINITY) {
      const float m_new = fmaxf(m_run, tmax);
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = sv[r] - m_new;                                    // <= 0 on negatives, -inf elsewhere
        const bool neg = sv[r] > -INFINITY;
        a += neg ? expf(beta * d) : 0.f;
        c += neg ? expf(b1 * d) : 0.f;
      }
      const bool had = m_run > -INFINITY;
      const float dm = m_run - m_new;
      a_run = (had ? a_run * expf(beta * dm) : 0.f) + a;
      c_run = (had ? c_run * expf(b1 * dm) : 0.f) + c;
      m_run = m_new;
    }
  }

  // ---- merge: lane halves, then the two key-waves
  hard_merge(m_run, a_run, c_run, __shfl_xor(m_run, 32, 64), __shfl_xor(a_run, 32, 64), __shfl_xor(c_run, 32, 64), beta,
             b1);
  cnt += __shfl_xor(cnt, 32, 64);
  if (pos_hit && qg < o.Mx) p.pos[qg] = pos_v;                            // exactly one lane of the grid holds it
  if (wm == 1 && h == 0) {
    mrg[0][wn * 32 + li] = m_run; mrg[1][wn * 32 + li] = a_run; mrg[2][wn * 32 + li] = c_run; mrg[3][wn * 32 + li] = cnt;
  }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < o.Mx) {
    hard_merge(m_run, a_run, c_run, mrg[0][wn * 32 + li], mrg[1][wn * 32 + li], mrg[2][wn * 32 + li], beta, b1);
    float* out = p.part + ((long)ks * o.Mx + qg) * 4;
    out[0] = m_run; out[1] = a_run; out[2] = c_run; out[3] = cnt + mrg[3][wn * 32 + li];
  }
}

// one wave per query: lanes take the key-split partials s = lane, lane + 64, ..., merged by wave reductions (the fixed
// order of simce_lse_finalize), then the row's statistics and the gradient pass's coefficients:
//   log Ng = log n + m + log c - log a,  lse_h = logaddexp(pos, log Ng),  q = exp(log Ng - lse_h),
//   k1 = log(q (1 + beta)) - C,  k2 = log(q beta) - A   (log q = log Ng - lse_h: no log of an underflowed q)
__global__ __launch_bounds__(256) void simce_lse_hard_finalize(const float* part, int ksplit, int Mx, float beta,
                                                               const float* pos, float* lse_h, float* coef) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= Mx) return;
  part += (long)blockIdx.y * ksplit * Mx * 4;     // batched launch: blockIdx.y = problem
  pos += (long)blockIdx.y * Mx; lse_h += (long)blockIdx.y * Mx; coef += (long)blockIdx.y * 3 * Mx;
  const float b1 = 1.f + beta;
  float m = -INFINITY;
  for (int s = lane; s < ksplit; s += 64) m = fmaxf(m, part[((long)s * Mx + i) * 4]);
  m = wave_max(m);
  float a = 0.f, c = 0.f, n = 0.f;
  for (int s = lane; s < ksplit; s += 64) {
    const float* t = part + ((long)s * Mx + i) * 4;
    if (t[0] > -INFINITY) { a += t[1] * expf(beta * (t[0] - m)); c += t[2] * expf(b1 * (t[0] - m)); }
    n += t[3];
  }
  a = wave_sum(a); c = wave_sum(c); n = wave_sum(n);
  if (lane == 0) {
    const float ps = pos[i];
    float lse = ps, q = 0.f, k1 = -INFINITY, k2 = -INFINITY;             // n = 0: loss 0, zero gradient
    if (n > 0.f) {
      const float la = logf(a), lc = logf(c);
      const float lng = logf(n) + m + lc - la;
      const float mm = fmaxf(ps, lng);
      lse = mm + logf(expf(ps - mm) + expf(lng - mm));
      const float lq = lng - lse;
      q = expf(lq);
      k1 = lq + logf(b1) - (b1 * m + lc);
      if (beta > 0.f) k2 = lq + logf(beta) - (beta * m + la);
    }
    lse_h[i] = lse;
    coef[i] = q; coef[Mx + i] = k1; coef[2 * (long)Mx + i] = k2;
  }
}

// ------------------------------------------------------------------------------------------------ gradient pass
// simce_grad_tiled_kernel's structure (S^T tile, G in the accumulator layout -> LDS tile, dX^T += Y^T G^T, slabs per
// key split) with the hard-negative G.  Per logit: the key's id and its two coefficients come from L1 as lse_y[key]
// does in the plain pass (a half-wave reads one key: broadcast); keys outside Neg are selected out, never multiplied
// by a zero mask (their exponents are not bounded).
struct HGP {
  float beta;
  const float* coef_x; const float* coef_y;     // [3][Mx] / [3][Ny]: q, k1, k2 of the queries / of the keys' own direction
  float w_row, w_col, inv_bg;
  const float* upstream;   // device scalar multiplied into inv_bg, or null
  float* slab;         // [ksplit][Mx][P]
  float* dsc_part;     // [ksplit][Mx]
  // batched launch: coef_x = coef_y = coef [nz][3][Mx], upstream [nz] (or null), slab and dsc_part hold the problems one
  // after another
  SimceOps o;
};

template <bool ZB>
__global__ __launch_bounds__(256, 2) void simce_grad_hard_kernel(const HGP pa) {
  HGP p = pa;
  if constexpr (ZB) {                                                     // this workgroup's problem
    const int z = blockIdx.z, r = pa.o.z.rev[z];
    const long zs = simce_rebase(p.o, pa.o.z);
    p.coef_x = pa.coef_x + (long)z * 3 * p.o.Mx; p.coef_y = pa.coef_x + (long)r * 3 * p.o.Mx;   // the keys': the reverse problem's
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
  const float beta = p.beta, b1 = 1.f + p.beta;
  const KeyWalk<BKG, true> w(o.X, o.Mx, nullptr, o.Mx, o.Y, o.Ny, o.P, o.tiles_per_split, o.ntiles, smem, o.Yc, o.Nc);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, qg = w.qg;
  const int Nkeys = w.Nk;
  const int label = o.label_offset + qg;
  const int qc = qg < o.Mx ? qg : o.Mx - 1;
  const float qx = p.coef_x[qc], k1x = p.coef_x[o.Mx + qc], k2x = p.coef_x[2 * (long)o.Mx + qc];
  const float* k1y = p.coef_y + o.Ny;
  const float* k2y = p.coef_y + 2 * (long)o.Ny;
  const float ibg = p.upstream ? p.inv_bg * p.upstream[0] : p.inv_bg;
  f32x16 dx[4][2];
  key_sum_zero(dx);
  float dsc = 0.f;
  int64_t cq = 0;
  if (o.cls_x) cq = o.cls_x[qc];

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
      if (key < Nkeys && qg < o.Mx) {
        const bool kin = key < o.Ny;
        if (kin && key == label) {
          gv = -(p.w_row * qx + p.w_col * p.coef_y[key]) * ibg;
        } else if (!(kin && o.cls_y && o.cls_y[key] == cq)) {             // in Neg_i (and, for batch keys, i in Neg'_j)
          gv = p.w_row * (expf(fmaf(b1, sv, k1x)) - expf(fmaf(beta, sv, k2x)));
          if (kin) gv += p.w_col * (expf(fmaf(b1, sv, k1y[key])) - expf(fmaf(beta, sv, k2y[key])));
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

constexpr size_t GRAD_LDS_BYTES = (size_t)SIMCE_GRAD_LDS_FLOATS * sizeof(float);

// the LSE pass on the grid k and its finalize, for `problems` problems
template <bool ZB>
int lse_hard_launch(const HLP& p, const KeySplitPlan& k, int problems, float* lse_h, float* coef, void* stream) {
  const int rc = simce_launch<simce_lse_hard_kernel<ZB>>(p, k, problems, 0, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(simce_lse_hard_finalize, dim3((p.o.Mx + 3) / 4, problems), dim3(256), 0, (hipStream_t)stream,
                     (const float*)p.part, k.ksplit, p.o.Mx, p.beta, (const float*)p.pos, lse_h, coef);
  return clipk_check_launch();
}

// what every gradient launch fills besides the operand block
HGP grad_args(float beta, const float* coef_x, const float* coef_y, float w_row, float w_col, float inv_bg,
              const float* upstream, float* slab, float* dsc_part) {
  HGP p{};
  p.beta = beta; p.coef_x = coef_x; p.coef_y = coef_y; p.w_row = w_row; p.w_col = w_col; p.inv_bg = inv_bg;
  p.upstream = upstream; p.slab = slab; p.dsc_part = dsc_part;
  return p;
}

}  // namespace

// the tiled pass and its finalize; part: [ksplit][Mx][4] with ksplit of key_split_plan(Mx, Ny + Nc, 64)
extern "C" int clipk_simce_lse_hard_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                                           const float* scale, float beta, int label_offset, const int64_t* cls_x,
                                           const int64_t* cls_y, float* part, float* lse_h, float* pos, float* coef,
                                           void* stream) {
  const KeySplitPlan k = key_split_plan(Mx, Ny + Nc, TQ);
  HLP p{};
  p.o = simce_ops(X, Mx, Y, Ny, Yc, Nc, P, scale, label_offset, cls_x, cls_y, k);
  p.beta = beta; p.part = part; p.pos = pos;
  return lse_hard_launch<false>(p, k, 1, lse_h, coef, stream);
}

// the tiled pass only: dX slabs and dscale partials per key split (the same plan), summed by the caller
extern "C" int clipk_simce_grad_hard_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                                            const float* scale, float beta, int label_offset, const float* coef_x,
                                            const float* coef_y, const int64_t* cls_x, const int64_t* cls_y, float w_row,
                                            float w_col, float inv_bg, const float* upstream, float* slab,
                                            float* dsc_part, void* stream) {
  if (P > KEYSUM_PMAX) return CLIPK_ERR_UNSUPPORTED;
  const KeySplitPlan k = key_split_plan(Mx, Ny + Nc, TQ);
  HGP p = grad_args(beta, coef_x, coef_y, w_row, w_col, inv_bg, upstream, slab, dsc_part);
  p.o = simce_ops(X, Mx, Y, Ny, Yc, Nc, P, scale, label_offset, cls_x, cls_y, k);
  return simce_launch<simce_grad_hard_kernel<false>>(p, k, 1, GRAD_LDS_BYTES, stream);
}

// ---- batched launches (clipk_simce_{lse,grad}_pairs_hard): zt.nz problems of shape B x B over zt.E in one grid, the
// splits of key_split_plan for the whole grid; per-problem outputs and partials follow one another
extern "C" int clipk_simce_lse_pairs_hard_launch(const PairZ* zt, int B, int P, const float* scale, float beta, float* part,
                                                 float* lse_h, float* pos, float* coef, void* stream) {
  const KeySplitPlan k = key_split_plan(B, B, TQ, zt->nz);
  HLP p{};
  p.o = simce_ops(nullptr, B, nullptr, B, nullptr, 0, P, scale, 0, nullptr, nullptr, k, zt);
  p.beta = beta; p.part = part; p.pos = pos;
  return lse_hard_launch<true>(p, k, zt->nz, lse_h, coef, stream);
}

extern "C" int clipk_simce_grad_pairs_hard_launch(const PairZ* zt, int B, int P, const float* scale, float beta,
                                                  const float* coef, float w_row, float w_col, float inv_bg,
                                                  const float* upstream, float* slab, float* dsc_part, void* stream) {
  if (P > KEYSUM_PMAX) return CLIPK_ERR_UNSUPPORTED;
  const KeySplitPlan k = key_split_plan(B, B, TQ, zt->nz);
  HGP p = grad_args(beta, coef, coef, w_row, w_col, inv_bg, upstream, slab, dsc_part);
  p.o = simce_ops(nullptr, B, nullptr, B, nullptr, 0, P, scale, 0, nullptr, nullptr, k, zt);
  return simce_launch<simce_grad_hard_kernel<true>>(p, k, zt->nz, GRAD_LDS_BYTES, stream);
}
