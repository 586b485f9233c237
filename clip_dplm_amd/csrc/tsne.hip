// tsne.hip — exact t-SNE of an embedding cloud without the N x N matrix (include/clipk.h: clipk_cond_entropy_sums,
// clipk_tsne_grad and clipk_tsne_update have the formulae, the diagonal rule and the supported range).
//
//   d_ij = max(nx_i + nx_j - 2 <x_i, x_j>, 0),  m_i = min_{j != i} d_ij
//   p_{j|i} = exp(-beta_i (d_ij - m_i)) / s0_i,  P_ij = (p_{j|i} + p_{i|j}) / (2N),  w_ij = 1 / (1 + |y_i - y_j|^2)
//
// Both walks are kernel_sums_kernel<false> with another epilogue: cloud_tile.h's KeyWalk of X against itself on
// sim_tile.h's exact-f32 64 x 64 block (keys on the MFMA rows, queries on the lanes), d once per element, the row sums
// per lane, lane halves by a shuffle, the two key-waves through LDS, the key splits in split order by a finalize launch.
//   * cond_entropy_walk: the row minimum of d, and for B <= 8 candidate bandwidths PER ROW (held in the lane's registers:
//     the lane is the query) s0 = sum exp(-beta t), s1 = sum t exp(-beta t) with t = d - shift_i.  What the perplexity
//     search evaluates; the search itself is host arithmetic on [N, B] device tensors.
//   * tsne_grad_walk: both sides of a pair carry a record (norm, -beta log2 e in two parts, m, log2 s0, y0, y1), the keys'
//     staged in LDS per tile.  Per element two exp2, one rcp and no division; the logarithm only with the KL row sum.
//     The exponent is formed from (d - m): -beta (d - m) - log s0, never as a d + b with beta m folded into b - beta m
//     reaches the hundreds and the cancellation would cost the exponent its digits.
//   * tsne_tail (one workgroup, fixed order): Z = sum_i zrow_i, the KL value and the gradient norm;
//     tsne_update_kernel: the delta-bar-delta step over the 2N coordinates, Z read from device memory.
// The skipped key of a row (diag_offset) is dropped as a term - never formed and subtracted.
// No float atomics, no cooperative launch: results depend on the shapes and inputs alone.
#include "common.h"
#include "cloud_keysum.h"
#include <math.h>

namespace {

constexpr int TS_PMAX = KEYSUM_PMAX;              // contraction limit
constexpr int TS_BMAX = 8;                        // candidate bandwidths per row and launch
constexpr int REC = 8;                            // floats per point record of the gradient walk
constexpr float L_HI = 1.44269502162933349609375f, L_LO = 1.92596299112661746e-8f;   // log2(e) = L_HI + L_LO
constexpr float LN2 = 0.693147180559945309f;

// this query's skipped key, -1 where there is none (or it lies beyond N: nothing to skip)
__device__ __forceinline__ int skipped_key(long long diag_offset, int qg, int N) {
  if (diag_offset < 0) return -1;
  const long long sk = (long long)qg + diag_offset;
  return sk < (long long)N ? (int)sk : -1;
}

// ------------------------------------------------------------------------------------------------ calibration walk
struct CEP {
  const float* X; int N, P, B;
  const float* nx;                                // [N] squared norms
  const float* betas;                             // [N][B] or null (B = 0: the minimum alone)
  const float* shift;                             // [N] or null (zeros)
  long long diag_offset;
  float* min_part;                                // [ksplit][N] or null
  float* s_part;                                  // [ksplit][2][N][B]: s0 then s1 (B > 0)
  int tiles_per_split, ntiles;
};

constexpr int CE_MERGE_LD = 2 * TS_BMAX + 1;      // floats per query of the key-wave merge: s0[8], s1[8], min
constexpr int CE_LDS_FLOATS = KLOOP_LDS_FLOATS + TQ * CE_MERGE_LD;

// WANT_MIN: the row minimum is formed too (the first pass asks for it alone, B = 0)
template <bool WANT_MIN>
__global__ __launch_bounds__(256, 2) void cond_entropy_walk(const CEP p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                       // K-loop buffers
  float* mrg = smem + KLOOP_LDS_FLOATS;                                   // [64 queries][CE_MERGE_LD]: key-wave 1's sums
  const KeyWalk<BKG> w(p.X, p.N, nullptr, p.N, p.X, p.N, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  const int N = p.N, B = p.B;
  const int qc = qg < N ? qg : N - 1;
  const float nx_i = p.nx[qc];
  const float sh_i = p.shift ? p.shift[qc] : 0.f;
  // exp(-beta t) = 2^(c t) with c = -beta log2(e) held as cg + cl (kernel_sums.hip: one rounding of c would be the same
  // relative error of every exponent of the row - a shifted beta, which does not average out over the sum)
  float cg[TS_BMAX], cl[TS_BMAX], s0[TS_BMAX], s1[TS_BMAX];
#pragma unroll
  for (int b = 0; b < TS_BMAX; ++b) {
    cg[b] = cl[b] = s0[b] = s1[b] = 0.f;
    if (b < B) {
      const float gm = -p.betas[(long)qc * B + b];
      cg[b] = gm * L_HI;
      cl[b] = fmaf(gm, L_HI, -cg[b]) + gm * L_LO;
    }
  }
  const int skip = skipped_key(p.diag_offset, qg, N);
  float rmin = INFINITY;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    float nyk[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = w.key(j0, r);
      nyk[r] = p.nx[key < N ? key : N - 1];
    }
    f32x16 acc;
    w.product(j0, acc);
    float t[16];
    bool keep[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = w.key(j0, r);
      const float d = fmaxf(fmaf(-2.f, acc[r], nx_i + nyk[r]), 0.f);
      keep[r] = key < N && qg < N && key != skip;                         // the term is dropped, not subtracted
      if constexpr (WANT_MIN) rmin = keep[r] ? fminf(rmin, d) : rmin;
      t[r] = d - sh_i;
    }
#pragma unroll
    for (int b = 0; b < TS_BMAX; ++b)
      if (b < B) {                                                        // d once, B exponentials on it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float e = __builtin_amdgcn_exp2f(fmaf(cg[b], t[r], cl[b] * t[r]));
          e = keep[r] ? e : 0.f;
          s0[b] += e;
          s1[b] = fmaf(t[r], e, s1[b]);
        }
      }
  }

  // ---- partials: lane halves, then the two key-waves
  __syncthreads();
#pragma unroll
  for (int b = 0; b < TS_BMAX; ++b)
    if (b < B) {
      s0[b] += __shfl_xor(s0[b], 32, 64);
      s1[b] += __shfl_xor(s1[b], 32, 64);
    }
  rmin = fminf(rmin, __shfl_xor(rmin, 32, 64));
  float* slot = mrg + (wn * 32 + li) * CE_MERGE_LD;
  if (wm == 1 && h == 0) {
#pragma unroll
    for (int b = 0; b < TS_BMAX; ++b)
      if (b < B) { slot[b] = s0[b]; slot[TS_BMAX + b] = s1[b]; }
    slot[2 * TS_BMAX] = rmin;
  }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < N) {
    const long nb = (long)N * B;
#pragma unroll
    for (int b = 0; b < TS_BMAX; ++b)
      if (b < B) {
        p.s_part[(long)ks * 2 * nb + (long)qg * B + b] = s0[b] + slot[b];
        p.s_part[(long)ks * 2 * nb + nb + (long)qg * B + b] = s1[b] + slot[TS_BMAX + b];
      }
    if constexpr (WANT_MIN) p.min_part[(long)ks * N + qg] = fminf(rmin, slot[2 * TS_BMAX]);
  }
}

// the key splits in split order: dmin [N] (null: skipped), s0 / s1 [N][B] (null: skipped)
__global__ __launch_bounds__(256) void cond_entropy_finalize(const float* min_part, const float* s_part, int ksplit, int N,
                                                             int B, float* dmin, float* s0, float* s1) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  const long nb = (long)N * B;
  if (dmin)
    for (long i = tid; i < N; i += nth) {
      float m = min_part[i];
      for (int s = 1; s < ksplit; ++s) m = fminf(m, min_part[(long)s * N + i]);
      dmin[i] = m;
    }
  for (int o = 0; o < 2; ++o) {
    float* out = o ? s1 : s0;
    if (!out) continue;
    for (long i = tid; i < nb; i += nth) {
      float a = 0.f;
      for (int s = 0; s < ksplit; ++s) a += s_part[((long)s * 2 + o) * nb + i];
      out[i] = a;
    }
  }
}

// ------------------------------------------------------------------------------------------------ gradient walk
struct TGP {
  const float* X; int N, P, NC;                   // NC: 6 row sums with the KL term, 5 without
  const float* rec;                               // [N][REC]: nx, cg, cl, m, log2 s0, y0, y1, 0
  long long diag_offset;
  float inv2n;                                    // 1 / (2N)
  float* part;                                    // [ksplit][N][NC]
  int tiles_per_split, ntiles;
};

constexpr int TG_NC = 6;
constexpr int TG_LDS_FLOATS = KLOOP_LDS_FLOATS + TK * REC + TQ * TG_NC;

// rec[i] from the per-point vectors (the C entry's own launch: the walk reads one 32-byte record per point and side)
__global__ __launch_bounds__(256) void tsne_pack(const float* nx, const float* beta, const float* dmin, const float* log_s0,
                                                 const float* Y, int N, float* rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float gm = -beta[i];
  const float cg = gm * L_HI;
  const float cl = fmaf(gm, L_HI, -cg) + gm * L_LO;
  const float ls = log_s0[i];
  const float l2 = fmaf(ls, L_HI, ls * L_LO);                             // log2 s0
  f32x4* o = reinterpret_cast<f32x4*>(rec + (long)i * REC);
  o[0] = f32x4{nx[i], cg, cl, dmin[i]};
  o[1] = f32x4{l2, Y[2 * (long)i], Y[2 * (long)i + 1], 0.f};
}

template <bool KL>
__global__ __launch_bounds__(256, 2) void tsne_grad_walk(const TGP p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                       // K-loop buffers
  float* krec = smem + KLOOP_LDS_FLOATS;                                  // [64 keys][REC]: the tile's key records
  float* mrg = krec + TK * REC;                                           // [64 queries][6]: key-wave 1's sums
  const KeyWalk<BKG> w(p.X, p.N, nullptr, p.N, p.X, p.N, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  const int N = p.N;
  const int qc = qg < N ? qg : N - 1;
  const f32x4 qa = reinterpret_cast<const f32x4*>(p.rec + (long)qc * REC)[0];
  const f32x4 qb = reinterpret_cast<const f32x4*>(p.rec + (long)qc * REC)[1];
  const float nx_i = qa[0], cg_i = qa[1], cl_i = qa[2], m_i = qa[3], l2_i = qb[0], y0_i = qb[1], y1_i = qb[2];
  const int skip = skipped_key(p.diag_offset, qg, N);
  const float inv2n = p.inv2n;
  float a0 = 0.f, a1 = 0.f, r0 = 0.f, r1 = 0.f, zs = 0.f, kl = 0.f;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    // the tile's key records: threads 0..127 move one 16-byte half each - loaded ahead of the product, stored behind its
    // last barrier, which every wave reaches only after its reads of the previous tile's records
    f32x4 stage = {0.f, 0.f, 0.f, 0.f};
    if (w.tid < 2 * TK) {
      const int key = j0 + (w.tid >> 1);
      stage = reinterpret_cast<const f32x4*>(p.rec + (long)(key < N ? key : N - 1) * REC)[w.tid & 1];
    }
    f32x16 acc;
    w.product(j0, acc);                                                   // (ends with a barrier: krec is free)
    if (w.tid < 2 * TK) reinterpret_cast<f32x4*>(krec)[w.tid] = stage;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl_row = wm * 32 + keyrow32(r, h);
      const int key = j0 + kl_row;
      const f32x4 ka = reinterpret_cast<const f32x4*>(krec + kl_row * REC)[0];
      const f32x4 kb = reinterpret_cast<const f32x4*>(krec + kl_row * REC)[1];
      const float d = fmaxf(fmaf(-2.f, acc[r], nx_i + ka[0]), 0.f);
      const float ti = d - m_i, tj = d - ka[3];
      const float ei = __builtin_amdgcn_exp2f(fmaf(cg_i, ti, fmaf(cl_i, ti, -l2_i)));          // p_{j|i}
      const float ej = __builtin_amdgcn_exp2f(fmaf(ka[1], tj, fmaf(ka[2], tj, -kb[0])));       // p_{i|j}
      const float dy0 = y0_i - kb[1], dy1 = y1_i - kb[2];
      const float q = fmaf(dy1, dy1, fmaf(dy0, dy0, 1.f));
      const bool keep = key < N && qg < N && key != skip;                 // the term is dropped, not subtracted
      const float wq = keep ? __builtin_amdgcn_rcpf(q) : 0.f;
      const float pj = keep ? (ei + ej) * inv2n : 0.f;                    // P_ij
      const float pw = pj * wq, w2 = wq * wq;
      a0 = fmaf(pw, dy0, a0); a1 = fmaf(pw, dy1, a1);
      r0 = fmaf(w2, dy0, r0); r1 = fmaf(w2, dy1, r1);
      zs += wq;
      if constexpr (KL) {
        // log2(P_ij / w_ij).  0 log 0 = 0; v_log_f32 takes no denormals, and below the smallest normal number the term
        // is under 2^-126 x 126 - nothing in a sum whose terms reach 1 / N
        const float pq = pj * q;
        const float lg = __builtin_amdgcn_logf(pq);
        kl = pq >= 1.17549435e-38f ? fmaf(pj, lg, kl) : kl;
      }
    }
  }

  // ---- partials: lane halves, then the two key-waves
  float v[TG_NC] = {a0, a1, r0, r1, zs, kl * LN2};
  __syncthreads();
#pragma unroll
  for (int c = 0; c < TG_NC; ++c) v[c] += __shfl_xor(v[c], 32, 64);
  float* slot = mrg + (wn * 32 + li) * TG_NC;
  if (wm == 1 && h == 0) {
#pragma unroll
    for (int c = 0; c < TG_NC; ++c) slot[c] = v[c];
  }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < N) {
    float* out = p.part + ((long)ks * N + qg) * p.NC;
#pragma unroll
    for (int c = 0; c < TG_NC; ++c)
      if (c < p.NC) out[c] = v[c] + slot[c];
  }
}

// rows[i] = the key splits of part in split order, n = N * NC values
__global__ __launch_bounds__(256) void tsne_grad_finalize(const float* part, int ksplit, long n, float* rows) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < n; i += nth) {
    float a = 0.f;
    for (int s = 0; s < ksplit; ++s) a += part[(long)s * n + i];
    rows[i] = a;
  }
}

// ------------------------------------------------------------------------------------------------ tail and update
constexpr int TAIL_T = 1024;

// sum over the workgroup in a fixed order: thread t holds the strided partial, then a tree in LDS
__device__ __forceinline__ float tail_sum(float v, float* red, int t) {
  red[t] = v;
  __syncthreads();
  for (int s = TAIL_T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// grad_i = 4 (alpha attr_i - rep_i / Z), component c
__device__ __forceinline__ float grad_of(const float* row, int c, float alpha, float inv_z) {
  return 4.f * (alpha * row[c] - row[2 + c] * inv_z);
}

// one workgroup: z[0] = sum_i zrow_i; kl[0] = sum_i klrow_i + log Z (NC = 6); gnorm[0] = |grad|_2
__global__ __launch_bounds__(TAIL_T) void tsne_tail(const float* rows, int N, int NC, float alpha, float* z, float* kl,
                                                    float* gnorm) {
  __shared__ float red[TAIL_T];
  const int t = threadIdx.x;
  float zs = 0.f, ks = 0.f;
  for (int i = t; i < N; i += TAIL_T) {
    zs += rows[(long)i * NC + 4];
    if (kl && NC == 6) ks += rows[(long)i * NC + 5];
  }
  const float Z = tail_sum(zs, red, t);
  if (t == 0) z[0] = Z;
  if (kl) {
    const float K = tail_sum(ks, red, t);
    if (t == 0) kl[0] = NC == 6 ? K + logf(Z) : NAN;
  }
  if (gnorm) {
    const float inv_z = 1.f / Z;
    float g2 = 0.f;
    for (int i = t; i < N; i += TAIL_T) {
      const float g0 = grad_of(rows + (long)i * NC, 0, alpha, inv_z), g1 = grad_of(rows + (long)i * NC, 1, alpha, inv_z);
      g2 = fmaf(g0, g0, fmaf(g1, g1, g2));
    }
    const float G = tail_sum(g2, red, t);
    if (t == 0) gnorm[0] = sqrtf(G);
  }
}

__global__ __launch_bounds__(256) void tsne_update_kernel(const float* rows, int N, int NC, float alpha, float momentum,
                                                          float lr, const float* z, float* y, float* update, float* gains) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= 2 * (long)N) return;
  const float inv_z = 1.f / z[0];
  const float g = grad_of(rows + (e >> 1) * NC, (int)(e & 1), alpha, inv_z);
  const float u = update[e];
  float gn = gains[e];
  gn = (u * g < 0.f) ? gn + 0.2f : gn * 0.8f;
  gn = fmaxf(gn, 0.01f);
  const float un = momentum * u - lr * (gn * g);
  gains[e] = gn;
  update[e] = un;
  y[e] += un;
}

bool shape_ok(int N, int P) { return cloud_shape_ok(N, N, P, TS_PMAX) && N >= 3; }

size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

}  // namespace

extern "C" size_t clipk_cond_entropy_sums_workspace(int N, int P, int B) {
  if (!shape_ok(N, P) || B < 0 || B > TS_BMAX) return 0;
  const size_t ks = key_split_plan(N, N, TQ).ksplit;
  return ks * (size_t)N * (1 + 2 * (size_t)B) * sizeof(float);            // the minimum's partials, then s0 / s1's
}

extern "C" int clipk_cond_entropy_sums(const float* X, int N, int P, const float* nx, const float* betas, int B,
                                       const float* shift, long long diag_offset, float* dmin, float* s0, float* s1,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (N <= 0 || P <= 0 || B < 0 || diag_offset < -1) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(N, P) || B > TS_BMAX) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !nx || !workspace || (!dmin && !s0 && !s1)) return CLIPK_ERR_BAD_ARG;
  if ((B == 0) != (!s0 && !s1) || (B > 0 && !betas)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_cond_entropy_sums_workspace(N, P, B)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(N, N, TQ);                        // the grid of the LSE pass
  CEP p{};
  p.X = X; p.N = N; p.P = P; p.B = B; p.nx = nx; p.betas = betas; p.shift = shift; p.diag_offset = diag_offset;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  float* ws = (float*)workspace;
  p.min_part = dmin ? ws : nullptr;
  p.s_part = ws + (size_t)k.ksplit * N;
  const size_t lds = (size_t)CE_LDS_FLOATS * sizeof(float);
  if (dmin) hipLaunchKernelGGL(cond_entropy_walk<true>, dim3(k.nqb, k.ksplit), dim3(256), lds, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(cond_entropy_walk<false>, dim3(k.nqb, k.ksplit), dim3(256), lds, (hipStream_t)stream, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  long blocks = ((long)N * (B > 0 ? B : 1) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(cond_entropy_finalize, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, p.min_part, p.s_part,
                     k.ksplit, N, B, dmin, s0, s1);
  return clipk_check_launch();
}

extern "C" size_t clipk_tsne_grad_workspace(int N, int P, int want_kl) {
  if (!shape_ok(N, P)) return 0;
  const size_t ks = key_split_plan(N, N, TQ).ksplit;
  return ((size_t)N * REC + pad4(ks * (size_t)N * (want_kl ? 6 : 5))) * sizeof(float);   // the records, then the partials
}

extern "C" int clipk_tsne_grad(const float* X, int N, int P, const float* nx, const float* beta, const float* dmin,
                               const float* log_s0, const float* Y, long long diag_offset, int want_kl, float* rows,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (N <= 0 || P <= 0 || diag_offset < -1) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(N, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !nx || !beta || !dmin || !log_s0 || !Y || !rows || !workspace) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_tsne_grad_workspace(N, P, want_kl)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(N, N, TQ);                        // the grid of the LSE pass
  float* ws = (float*)workspace;
  TGP p{};
  p.X = X; p.N = N; p.P = P; p.NC = want_kl ? 6 : 5; p.rec = ws; p.diag_offset = diag_offset;
  p.inv2n = (float)(1.0 / (2.0 * N));
  p.part = ws + (size_t)N * REC;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  hipLaunchKernelGGL(tsne_pack, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, nx, beta, dmin, log_s0, Y, N, ws);
  int rc = clipk_check_launch();
  if (rc) return rc;
  const size_t lds = (size_t)TG_LDS_FLOATS * sizeof(float);
  if (want_kl) hipLaunchKernelGGL(tsne_grad_walk<true>, dim3(k.nqb, k.ksplit), dim3(256), lds, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(tsne_grad_walk<false>, dim3(k.nqb, k.ksplit), dim3(256), lds, (hipStream_t)stream, p);
  rc = clipk_check_launch();
  if (rc) return rc;
  const long n = (long)N * p.NC;
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(tsne_grad_finalize, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, p.part, k.ksplit, n, rows);
  return clipk_check_launch();
}

extern "C" int clipk_tsne_update(const float* rows, int N, int ncomp, float alpha, float momentum, float lr, float* Y,
                                 float* update, float* gains, float* z, float* kl, float* gnorm, void* stream) {
  if (N <= 0 || (ncomp != 5 && ncomp != 6)) return CLIPK_ERR_BAD_ARG;
  if (N < 3) return CLIPK_ERR_UNSUPPORTED;
  if (!rows || !z || (kl && ncomp != 6)) return CLIPK_ERR_BAD_ARG;
  if ((Y || update || gains) && !(Y && update && gains)) return CLIPK_ERR_BAD_ARG;
  hipLaunchKernelGGL(tsne_tail, dim3(1), dim3(TAIL_T), 0, (hipStream_t)stream, rows, N, ncomp, alpha, z, kl, gnorm);
  int rc = clipk_check_launch();
  if (rc || !Y) return rc;                                                // Y == NULL: the reductions alone
  const long blocks = (2 * (long)N + 255) / 256;
  hipLaunchKernelGGL(tsne_update_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, rows, N, ncomp, alpha,
                     momentum, lr, z, Y, update, gains);
  return clipk_check_launch();
}
