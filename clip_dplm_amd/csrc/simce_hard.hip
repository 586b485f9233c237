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
// These are kernels of their own and not a third instantiation of simce_tiled.hip's templates, so that the plain and
// class-aware instantiations keep their code to the byte; the second product of the gradient pass (dX^T += Y^T G^T)
// and its write-back are that file's, restated.
//
// One running max serves both sums: beta >= 0 makes beta s and (1 + beta) s monotone in s, so m = max_{Neg} s bounds
// both exponents by 0 (A = beta m + log a, C = (1 + beta) m + log c, and C - A = m + log c - log a needs no beta).
#include "common.h"
#include "sim_tile.h"
#include <math.h>

namespace {

constexpr int TQ = 64, TK = 64;                   // queries per workgroup, keys per tile (simce_tiled.hip's)

struct HLP {
  const float* X; int Mx;
  const float* Y; int Ny;
  const float* Yc; int Nc;
  int P;
  const float* scale; int label_offset;
  float beta;
  float* part;         // [ksplit][Mx][4]: m, a = sum exp(beta (s - m)), c = sum exp((1 + beta)(s - m)), n
  float* pos;          // [Mx]
  int tiles_per_split, ntiles;
  const int64_t* cls_x; const int64_t* cls_y;   // [Mx] / [Ny] class ids, or both null (all distinct)
  PairZ z;                                      // batched launch: part / pos hold the problems one after another
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

// ZB: the batched launch, blockIdx.z = problem of p.z; the single-problem instantiation has none of its code
template <bool ZB>
__global__ __launch_bounds__(256, 2) void simce_lse_hard_kernel(const HLP pa) {
  HLP p = pa;
  if constexpr (ZB) {                                                     // this workgroup's problem
    const int z = blockIdx.z;
    p.X = pa.z.E + (long)pa.z.xa[z] * p.Mx * p.P;
    p.Y = p.Yc = pa.z.E + (long)pa.z.ya[z] * p.Ny * p.P;
    p.cls_x = p.cls_y = pa.z.ids[z];
    p.part += (long)z * gridDim.y * p.Mx * 4; p.pos += (long)z * p.Mx;
  }
  constexpr int BKL = 32;
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (BKL + 4)];   // 2 buffers x (keys | queries)
  __shared__ float mrg[4][TQ];                                            // key-wave 1's m | a | c | n per query
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;                                  // key half, query half
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * TQ, ks = blockIdx.y;
  const int P = p.P, Nkeys = p.Ny + p.Nc;
  const float scale = p.scale[0];
  const float beta = p.beta, b1 = 1.f + p.beta;
  const int qg = q0 + wn * 32 + li;                                       // this lane's query
  const int label = p.label_offset + qg;
  float m_run = -INFINITY, a_run = 0.f, c_run = 0.f, cnt = 0.f, pos_v = 0.f;
  bool pos_hit = false;
  int64_t cq = 0;
  if (p.cls_x) cq = p.cls_x[qg < p.Mx ? qg : p.Mx - 1];
  const float* xrows[BKL / 16];
#pragma unroll
  for (int i = 0; i < BKL / 16; ++i) {
    int q = q0 + (tid + i * 256) / (BKL / 4); q = q < p.Mx ? q : p.Mx - 1;
    xrows[i] = p.X + (long)q * P;
  }
  const int t_beg = ks * p.tiles_per_split;
  int t_end = t_beg + p.tiles_per_split; t_end = t_end < p.ntiles ? t_end : p.ntiles;

  for (int kt = t_beg; kt < t_end; ++kt) {
    const int j0 = kt * TK;
    const float* yrows[BKL / 16];
#pragma unroll
    for (int i = 0; i < BKL / 16; ++i) {
      int j = j0 + (tid + i * 256) / (BKL / 4); j = j < Nkeys ? j : Nkeys - 1;      // clamped: masked in the epilogue
      yrows[i] = (j < p.Ny) ? p.Y + (long)j * P : p.Yc + (long)(j - p.Ny) * P;
    }
    int64_t ck[16];                                                       // ids of this lane's 16 key rows
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = j0 + wm * 32 + keyrow32(r, h);
      ck[r] = (p.cls_y && key < p.Ny) ? p.cls_y[key] : ~cq;               // cache keys / no ids: never same-class
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<BKL>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
    // ---- the negatives of this lane's query among its 16 key rows of the tile
    float sv[16], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = j0 + wm * 32 + keyrow32(r, h);
      const float s = scale * acc[r];
      const bool diag = key == label && key < p.Ny;
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
  if (pos_hit && qg < p.Mx) p.pos[qg] = pos_v;                            // exactly one lane of the grid holds it
  if (wm == 1 && h == 0) {
    mrg[0][wn * 32 + li] = m_run; mrg[1][wn * 32 + li] = a_run; mrg[2][wn * 32 + li] = c_run; mrg[3][wn * 32 + li] = cnt;
  }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) {
    hard_merge(m_run, a_run, c_run, mrg[0][wn * 32 + li], mrg[1][wn * 32 + li], mrg[2][wn * 32 + li], beta, b1);
    float* o = p.part + ((long)ks * p.Mx + qg) * 4;
    o[0] = m_run; o[1] = a_run; o[2] = c_run; o[3] = cnt + mrg[3][wn * 32 + li];
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
  const float* X; int Mx;
  const float* Y; int Ny;
  const float* Yc; int Nc;
  int P;
  const float* scale; int label_offset;
  float beta;
  const float* coef_x; const float* coef_y;     // [3][Mx] / [3][Ny]: q, k1, k2 of the queries / of the keys' own direction
  float w_row, w_col, inv_bg;
  const float* upstream;   // device scalar multiplied into inv_bg, or null
  float* slab;         // [ksplit][Mx][P]
  float* dsc_part;     // [ksplit][Mx]
  int tiles_per_split, ntiles;
  const int64_t* cls_x; const int64_t* cls_y;
  // batched launch: coef_x = coef_y = coef [nz][3][Mx], upstream [nz] (or null), slab and dsc_part hold the problems one
  // after another
  PairZ z;
};

constexpr int GPMAX = 512;                         // contraction / output width limit
constexpr int YH_LD = GPMAX + 4;                   // floats per staged key row
constexpr int KSB = 16;                            // keys per staged block of the second product
constexpr int BKG = 16;                            // K-step of the S tile (LDS budget: 2 workgroups per CU)
constexpr int GRAD_LDS_FLOATS = 2 * 2 * 64 * (BKG + 4) + TK * TQ + KSB * YH_LD + 2 * TQ;

template <bool ZB>
__global__ __launch_bounds__(256, 2) void simce_grad_hard_kernel(const HGP pa) {
  HGP p = pa;
  if constexpr (ZB) {                                                     // this workgroup's problem
    const int z = blockIdx.z, r = pa.z.rev[z];
    const long zs = (long)z * gridDim.y * p.Mx;                           // rows of key-split partials before it
    p.X = pa.z.E + (long)pa.z.xa[z] * p.Mx * p.P;
    p.Y = p.Yc = pa.z.E + (long)pa.z.ya[z] * p.Ny * p.P;
    p.cls_x = p.cls_y = pa.z.ids[z];
    p.coef_x = pa.coef_x + (long)z * 3 * p.Mx; p.coef_y = pa.coef_x + (long)r * 3 * p.Mx;   // the keys': the reverse problem's
    if (pa.upstream) p.upstream = pa.upstream + z;
    p.slab += zs * p.P; p.dsc_part += zs;
  }
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                      // K-loop buffers
  float* gl = smem + 2 * 2 * 64 * (BKG + 4);                              // G tile [64 keys][64 queries]
  float* yh = gl + TK * TQ;                                               // key block [16][YH_LD] / output transposes
  float* dsl = yh + KSB * YH_LD;                                          // [64 queries] dscale partials of key-wave 1
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * TQ, ks = blockIdx.y;
  const int P = p.P, Nkeys = p.Ny + p.Nc;
  const float scale = p.scale[0];
  const float beta = p.beta, b1 = 1.f + p.beta;
  const int qg = q0 + wn * 32 + li;
  const int label = p.label_offset + qg;
  const int qc = qg < p.Mx ? qg : p.Mx - 1;
  const float qx = p.coef_x[qc], k1x = p.coef_x[p.Mx + qc], k2x = p.coef_x[2 * (long)p.Mx + qc];
  const float* k1y = p.coef_y + p.Ny;
  const float* k2y = p.coef_y + 2 * (long)p.Ny;
  const float ibg = p.upstream ? p.inv_bg * p.upstream[0] : p.inv_bg;
  const int npt = (P + 127) / 128;                                        // 32-row p tiles per wave: P/4 / 32
  const int pw = npt * 32;                                                // p rows per wave
  f32x16 dx[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) dx[a][b][r] = 0.f;
  float dsc = 0.f;
  int64_t cq = 0;
  if (p.cls_x) cq = p.cls_x[qc];

  const float* xrows[1];
  { int q = q0 + (tid >> 2); q = q < p.Mx ? q : p.Mx - 1; xrows[0] = p.X + (long)q * P; }
  auto key_row = [&](int j) {
    j = j < Nkeys ? j : Nkeys - 1;
    return (j < p.Ny) ? p.Y + (long)j * P : p.Yc + (long)(j - p.Ny) * P;
  };
  const int t_beg = ks * p.tiles_per_split;
  int t_end = t_beg + p.tiles_per_split; t_end = t_end < p.ntiles ? t_end : p.ntiles;

  for (int kt = t_beg; kt < t_end; ++kt) {
    const int j0 = kt * TK;
    const float* yrows[1] = {key_row(j0 + (tid >> 2))};
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<BKG>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);          // (its first barrier also frees gl / yh)
    // ---- G (accumulator layout: rows = keys, lanes = queries) -> LDS tile gl[key][query]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = wm * 32 + keyrow32(r, h);
      const int key = j0 + kl;
      const float sv = scale * acc[r];
      float gv = 0.f;
      if (key < Nkeys && qg < p.Mx) {
        const bool kin = key < p.Ny;
        if (kin && key == label) {
          gv = -(p.w_row * qx + p.w_col * p.coef_y[key]) * ibg;
        } else if (!(kin && p.cls_y && p.cls_y[key] == cq)) {             // in Neg_i (and, for batch keys, i in Neg'_j)
          gv = p.w_row * (expf(fmaf(b1, sv, k1x)) - expf(fmaf(beta, sv, k2x)));
          if (kin) gv += p.w_col * (expf(fmaf(b1, sv, k1y[key])) - expf(fmaf(beta, sv, k2y[key])));
          gv *= ibg;
        }
      }
      dsc += gv * acc[r];
      gl[kl * TQ + wn * 32 + li] = gv;
    }
    // ---- dX^T += Y^T G^T, the key tile in blocks of KSB keys
    for (int kb = 0; kb < TK / KSB; ++kb) {
      __syncthreads();                                                    // gl complete (kb = 0) / yh free again
      {
        // stage Y[16 keys][P]: thread -> (key = tid / 16, 16-B chunks c = tid % 16 + 16 i), loads first, then stores
        const float* yr = key_row(j0 + kb * KSB + (tid >> 4));
        float* dst = yh + (tid >> 4) * YH_LD;
#pragma unroll
        for (int g = 0; g < 2; ++g) {                                     // two groups of four: 16 staging registers
          f32x4 tmp[GPMAX / 128];
#pragma unroll
          for (int i = 0; i < GPMAX / 128; ++i) {
            const int c = (tid & 15) + 16 * (g * (GPMAX / 128) + i);
            tmp[i] = (c * 4 < P) ? ld4(yr, c * 4, P) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int i = 0; i < GPMAX / 128; ++i) {
            const int c = (tid & 15) + 16 * (g * (GPMAX / 128) + i);
            if (c * 4 < P) *reinterpret_cast<f32x4*>(dst + c * 4) = tmp[i];
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < KSB / 2; ++u) {                                 // MFMA u contracts keys 2u (h = 0) and 2u + 1
        const int kl = 2 * u + h;
        const float b0 = gl[(kb * KSB + kl) * TQ + li], b1g = gl[(kb * KSB + kl) * TQ + 32 + li];
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (a < npt) {
            const int prow = wid * pw + a * 32 + li;
            const float av = prow < P ? yh[kl * YH_LD + prow] : 0.f;
            dx[a][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, dx[a][0], 0, 0, 0);
            dx[a][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1g, dx[a][1], 0, 0, 0);
          }
      }
    }
  }

  // ---- dX^T accumulators -> [q][p] rows through LDS (one 32 x 32 block per wave at a time), whole 128-B row segments
  __syncthreads();
  float* tb = yh + wid * (32 * 33);
#pragma unroll
  for (int a = 0; a < 4; ++a) {                             // (fully unrolled: the accumulators are register arrays)
    if (a < npt) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) tb[li * 33 + keyrow32(r, h)] = dx[a][b][r];  // [query][p]
        // wave-private region: the wave's own writes are visible to its reads in program order
#pragma unroll
        for (int it = 0; it < 16; ++it) {
          const int ql = it * 2 + h;                                      // 2 query rows per pass, 32 consecutive p each
          const int q = q0 + b * 32 + ql, pp = wid * pw + a * 32 + li;
          if (q < p.Mx && pp < P) p.slab[((long)ks * p.Mx + q) * P + pp] = tb[ql * 33 + li];
        }
      }
    }
  }
  // ---- d scale partials: lane halves, then the two key-waves
  dsc += __shfl_xor(dsc, 32, 64);
  if (wm == 1 && h == 0) dsl[wn * 32 + li] = dsc;
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) p.dsc_part[(long)ks * p.Mx + qg] = dsc + dsl[wn * 32 + li];
}

}  // namespace

extern "C" void clipk_simce_tiled_plan(int Mx, int Nkeys, int* nqb, int* ksplit, int* tps, int* ntiles);
extern "C" void clipk_simce_grad_tiled_plan(int Mx, int Nkeys, int* nqb, int* ksplit, int* tps, int* ntiles);
extern "C" void clipk_simce_pairs_tiled_plan(int npairs, int B, int* nqb, int* ksplit, int* tps, int* ntiles);

// the gradient kernel's 70 KiB of dynamic LDS, allowed once per device
template <bool ZB>
static void hard_grad_attr() {
  static std::atomic<uint64_t> attr_set{0};
  clipk_once_per_device(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(simce_grad_hard_kernel<ZB>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(GRAD_LDS_FLOATS * sizeof(float)));
  });
}

// the tiled pass and its finalize; part: [ksplit][Mx][4] with ksplit of clipk_simce_tiled_plan
extern "C" int clipk_simce_lse_hard_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                                           const float* scale, float beta, int label_offset, const int64_t* cls_x,
                                           const int64_t* cls_y, float* part, float* lse_h, float* pos, float* coef,
                                           void* stream) {
  HLP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.Yc = Yc ? Yc : Y; p.Nc = Nc; p.P = P;
  p.scale = scale; p.label_offset = label_offset; p.beta = beta; p.part = part; p.pos = pos;
  p.cls_x = cls_x; p.cls_y = cls_y;
  int nqb, ksplit;
  clipk_simce_tiled_plan(Mx, Ny + Nc, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  hipLaunchKernelGGL(simce_lse_hard_kernel<false>, dim3(nqb, ksplit), dim3(256), 0, (hipStream_t)stream, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(simce_lse_hard_finalize, dim3((Mx + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float*)part,
                     ksplit, Mx, beta, (const float*)pos, lse_h, coef);
  return clipk_check_launch();
}

// the tiled pass only: dX slabs and dscale partials per key split (clipk_simce_grad_tiled_plan), summed by the caller
extern "C" int clipk_simce_grad_hard_launch(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                                            const float* scale, float beta, int label_offset, const float* coef_x,
                                            const float* coef_y, const int64_t* cls_x, const int64_t* cls_y, float w_row,
                                            float w_col, float inv_bg, const float* upstream, float* slab,
                                            float* dsc_part, void* stream) {
  if (P > GPMAX) return CLIPK_ERR_UNSUPPORTED;
  HGP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.Yc = Yc ? Yc : Y; p.Nc = Nc; p.P = P;
  p.scale = scale; p.label_offset = label_offset; p.beta = beta; p.coef_x = coef_x; p.coef_y = coef_y;
  p.w_row = w_row; p.w_col = w_col; p.inv_bg = inv_bg; p.upstream = upstream; p.slab = slab; p.dsc_part = dsc_part;
  p.cls_x = cls_x; p.cls_y = cls_y;
  int nqb, ksplit;
  clipk_simce_grad_tiled_plan(Mx, Ny + Nc, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  hard_grad_attr<false>();
  hipLaunchKernelGGL(simce_grad_hard_kernel<false>, dim3(nqb, ksplit), dim3(256), (size_t)GRAD_LDS_FLOATS * sizeof(float),
                     (hipStream_t)stream, p);
  return clipk_check_launch();
}

// ---- batched launches (clipk_simce_{lse,grad}_pairs_hard): zt.nz problems of shape B x B over zt.E in one grid, the
// splits of clipk_simce_pairs_tiled_plan; per-problem outputs and partials follow one another
extern "C" int clipk_simce_lse_pairs_hard_launch(const PairZ* zt, int B, int P, const float* scale, float beta, float* part,
                                                 float* lse_h, float* pos, float* coef, void* stream) {
  HLP p{};
  p.Mx = B; p.Ny = B; p.Nc = 0; p.P = P; p.scale = scale; p.label_offset = 0; p.beta = beta;
  p.part = part; p.pos = pos; p.z = *zt;
  int nqb, ksplit;
  clipk_simce_pairs_tiled_plan(zt->nz, B, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  hipLaunchKernelGGL(simce_lse_hard_kernel<true>, dim3(nqb, ksplit, zt->nz), dim3(256), 0, (hipStream_t)stream, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(simce_lse_hard_finalize, dim3((B + 3) / 4, zt->nz), dim3(256), 0, (hipStream_t)stream,
                     (const float*)part, ksplit, B, beta, (const float*)pos, lse_h, coef);
  return clipk_check_launch();
}

extern "C" int clipk_simce_grad_pairs_hard_launch(const PairZ* zt, int B, int P, const float* scale, float beta,
                                                  const float* coef, float w_row, float w_col, float inv_bg,
                                                  const float* upstream, float* slab, float* dsc_part, void* stream) {
  if (P > GPMAX) return CLIPK_ERR_UNSUPPORTED;
  HGP p{};
  p.Mx = B; p.Ny = B; p.Nc = 0; p.P = P; p.scale = scale; p.label_offset = 0; p.beta = beta;
  p.coef_x = coef; p.coef_y = coef; p.w_row = w_row; p.w_col = w_col; p.inv_bg = inv_bg; p.upstream = upstream;
  p.slab = slab; p.dsc_part = dsc_part; p.z = *zt;
  int nqb, ksplit;
  clipk_simce_pairs_tiled_plan(zt->nz, B, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  hard_grad_attr<true>();
  hipLaunchKernelGGL(simce_grad_hard_kernel<true>, dim3(nqb, ksplit, zt->nz), dim3(256), (size_t)GRAD_LDS_FLOATS * sizeof(float),
                     (hipStream_t)stream, p);
  return clipk_check_launch();
}
