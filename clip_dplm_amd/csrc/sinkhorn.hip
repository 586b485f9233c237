// sinkhorn.hip — entropic optimal transport between two embedding clouds without the M x N matrix
// (include/clipk.h: clipk_sim_lse_bias / clipk_sinkhorn_apply have the formulae).
//
// A Sinkhorn half-iteration is a row log-sum-exp of S_ij + bias_j with S = scale <x_i, y_j>, and everything one wants
// from the plan P_ij = exp(S_ij + u_i + v_j) is a P-weighted sum over the keys.  Both walk the key tiles as
// cloud_tile.h's KeyWalk does on sim_tile.h's exact-f32 64 x 64 block (keys on the MFMA rows, queries on the lanes), with
// the key-side bias and the potentials where simce_tiled.hip has the cross-entropy's labels:
//   * sinkhorn_lse_kernel: 64 queries per workgroup, 64-key tiles, a running (max, sum) per lane, key-range splits as
//     (m, l) partials; sinkhorn_lse_finalize merges them in a fixed order, forms logw - LSE, applies the averaged update
//     of the symmetric problem and leaves each row's marginal-error term for sinkhorn_err_reduce (one workgroup, fixed
//     order: the error scalar is as deterministic as the potentials);
//   * sinkhorn_lse_x3_kernel: the same pass with the product as a bf16x3 split on v_mfma_f32_32x32x16_bf16 (plane_tile.h's
//     PlaneWalk: 128-query blocks, its own plan), feeding the same finalize and error kernels (clipk_sim_lse_bias_x3);
//   * sinkhorn_apply_kernel: S tile -> P tile into LDS -> key_sum_tile.h's weighted key sum (bary^T = Y^T P^T), mass and
//     cost from the same P values; key-split slabs are summed in split order by split_sum_finalize.
// No float atomics, no cooperative launch: results depend on the shapes alone.
#include "common.h"
#include "cloud_tile.h"
#include "plane_tile.h"
#include <math.h>

namespace {

constexpr int LSE_PMAX = 768;                     // contraction limit of the LSE pass

struct SLP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P;
  const float* scale;
  const float* bias;   // [Ny] or null (zeros)
  float* part_ml;      // [ksplit][Mx][2]
  int tiles_per_split, ntiles;
};

__global__ __launch_bounds__(256, 2) void sinkhorn_lse_kernel(const SLP p) {
  constexpr int BKL = 32;                                                 // 16 MFMAs per wave between barriers
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (BKL + 4)];   // 2 buffers x (keys | queries)
  __shared__ float mrg[2][TQ];                                            // key-wave 1's [m | l][query]
  const float scale = p.scale[0];
  const KeyWalk<BKL> w(p.X, p.Mx, nullptr, p.Mx, p.Y, p.Ny, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  float m_run = -INFINITY, l_run = 0.f;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    float bk[16];                                                         // bias of this lane's 16 key rows
#pragma unroll
    for (int r = 0; r < 16; ++r) bk[r] = w.key_bias(p.bias, j0, r);
    f32x16 acc;
    w.product(j0, acc);
    float sv[16], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sv[r] = w.key(j0, r) < p.Ny ? scale * acc[r] + bk[r] : -INFINITY;
      tmax = fmaxf(tmax, sv[r]);
    }
    if (tmax > -INFINITY) {
      const float m_new = fmaxf(m_run, tmax);
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += expf(sv[r] - m_new);              // exp(-inf) = 0 for masked keys
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
  if (wm == 1 && h == 0) { mrg[0][wn * 32 + li] = m_run; mrg[1][wn * 32 + li] = l_run; }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) {
    const float m1 = mrg[0][wn * 32 + li], l1 = mrg[1][wn * 32 + li];
    const float m_n = fmaxf(m_run, m1);
    float l_n = 0.f;
    if (m_n > -INFINITY) l_n = l_run * expf(m_run - m_n) + l1 * expf(m1 - m_n);
    float* o = p.part_ml + ((long)ks * p.Mx + qg) * 2;
    o[0] = m_n; o[1] = l_n;
  }
}

// ------------------------------------------------------------------------------------------------ bf16x3 LSE pass
// The same half-iteration with the product on the bf16 matrix pipe: A = hi.hi + hi.lo + lo.hi over the planes
// clipk_split_bf16 writes (row pitch PP = P rounded up to 32, pads zero: no K tail, every staging load 16 bytes).  The
// tile walk is plane_tile.h's PlaneWalk<2>, shared with retrieval.hip's sim_cand_kernel: 128 queries x 64 keys per
// workgroup, wave w owns queries [32 w, +32) against all 64 keys (two 32 x 32 accumulators of v_mfma_f32_32x32x16_bf16
// sharing one query fragment, three MFMAs per fragment pair), LDS rows of 80 bytes, two staging buffers (60 KiB: two
// workgroups per CU).  The epilogue is sinkhorn_lse_kernel's running (max, sum) per lane over the lane's 32 keys of the
// tile; a wave holds all 64 keys of its queries, so only the two lane halves are merged and the workgroup needs no merge
// slots.  The (m, l) partials have sinkhorn_lse_kernel's format: sinkhorn_lse_finalize and sinkhorn_err_reduce serve both.
// The exponentials are __expf (v_exp_f32 of the argument times log2 e): the argument is <= 0, its rounding moves a term
// by |arg| 2^-24 relative, and 32 of them per tile and lane sit on the VALU, which does not overlap this SIMD's MFMAs.
static_assert(PLK == TK, "key_split_plan counts tiles of TK keys");

struct SLPX {
  const unsigned short* xh; const unsigned short* xl; int Mx;
  const unsigned short* yh; const unsigned short* yl; int Ny;
  int PP;
  const float* scale;
  const float* bias;   // [Ny] or null (zeros)
  float* part_ml;      // [ksplit][Mx][2]
  int tiles_per_split, ntiles;
};

__global__ __launch_bounds__(256, 2) void sinkhorn_lse_x3_kernel(const SLPX p) {
  __shared__ __attribute__((aligned(16))) unsigned short sm[PlaneWalk<2>::LDS_ELEMS];
  const float scale = p.scale[0];
  const PlaneWalk<2> wk(p.xh, p.xl, p.Mx, p.yh, p.yl, p.Ny, p.PP, p.tiles_per_split, p.ntiles, sm);
  const int h = wk.h, ks = wk.ks, qg = wk.qg, Ny = p.Ny;
  float m_run = -INFINITY, l_run = 0.f;

  for (int kt = wk.t_beg; kt < wk.t_end; ++kt) {
    const int j0 = kt * PLK;
    const int kb0 = j0 + 4 * h;                                           // key of acc[kb][r]: kb0 + 32 kb + (keyrow32(r, 0))
    float bk[2][16];                                                      // bias of this lane's 32 keys
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb0 + 32 * kb + keyrow32(r, 0);
        bk[kb][r] = (p.bias && key < Ny) ? p.bias[key] : 0.f;
      }
    f32x16 acc[2];
    wk.product(j0, acc);
    // ---- running (max, sum) over the lane's 32 keys of this tile
    float sv[2][16], tmax = -INFINITY;
    const bool full = j0 + PLK <= Ny;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = scale * acc[kb][r] + bk[kb][r];
        sv[kb][r] = (full || kb0 + 32 * kb + keyrow32(r, 0) < Ny) ? s : -INFINITY;
        tmax = fmaxf(tmax, sv[kb][r]);
      }
    if (tmax > -INFINITY) {
      const float m_new = fmaxf(m_run, tmax);
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { a0 += __expf(sv[0][r] - m_new); a1 += __expf(sv[1][r] - m_new); }   // exp(-inf) = 0
      l_run = l_run * __expf(m_run - m_new) + (a0 + a1);
      m_run = m_new;
    }
  }

  // ---- merge the two lane halves (a wave holds every key of its queries)
  const float m_o = __shfl_xor(m_run, 32, 64), l_o = __shfl_xor(l_run, 32, 64);
  const float m_n = fmaxf(m_run, m_o);
  float l_n = 0.f;
  if (m_n > -INFINITY) l_n = l_run * __expf(m_run - m_n) + l_o * __expf(m_o - m_n);
  if (h == 0 && qg < p.Mx) {
    float* o = p.part_ml + ((long)ks * p.Mx + qg) * 2;
    o[0] = m_n; o[1] = l_n;
  }
}

// one wave per query: lanes take the key-split partials s = lane, lane + 64, ..., merged by wave reductions (fixed order).
// nv = logw - LSE; with prev: err_rows[i] = w_i |exp(prev_i - nv) - 1| (row i's share of the L1 marginal error of the
// potential being replaced) and, if `average`, out = (prev + nv) / 2.  prev is read before out is written: prev == out
// is fine.
__global__ __launch_bounds__(256) void sinkhorn_lse_finalize(const float* part_ml, int ksplit, int Mx, const float* logw,
                                                             const float* prev, int average, float* out,
                                                             float* err_rows) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= Mx) return;
  float m = -INFINITY;
  for (int s = lane; s < ksplit; s += 64) m = fmaxf(m, part_ml[((long)s * Mx + i) * 2]);
  m = wave_max(m);
  float l = 0.f;
  for (int s = lane; s < ksplit; s += 64) {
    const float ms = part_ml[((long)s * Mx + i) * 2], ls = part_ml[((long)s * Mx + i) * 2 + 1];
    if (ms > -INFINITY) l += ls * expf(ms - m);
  }
  l = wave_sum(l);
  if (lane == 0) {
    const float lw = logw ? logw[i] : 0.f, ll = logf(l);
    float nv = lw - (m + ll);
    if (prev) {
      const float pv = prev[i];
      if (err_rows) {
        // d = prev - nv = ((prev - logw) + m) + log l is small while its terms are not: the two large sums are taken with
        // their rounding errors (two-sum), so that d does not inherit the half ulp of |nv|
        const float s1 = pv - lw, b1 = s1 - pv, e1 = (pv - (s1 - b1)) + (-lw - b1);
        const float s2 = s1 + m, b2 = s2 - s1, e2 = (s1 - (s2 - b2)) + (m - b2);
        const float d = (s2 + ll) + (e1 + e2);
        err_rows[i] = expf(lw) * fabsf(expf(d) - 1.f);
      }
      if (average) nv = 0.5f * (pv + nv);
    }
    out[i] = nv;
  }
}

// err[0] += sum_i err_rows[i]: one workgroup, strided partial sums per thread, then a tree over the 1024 threads
__global__ __launch_bounds__(1024) void sinkhorn_err_reduce(const float* err_rows, int Mx, float* err) {
  __shared__ float red[1024];
  float a = 0.f;
  for (int i = threadIdx.x; i < Mx; i += 1024) a += err_rows[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) err[0] += red[0];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ apply pass
// (cloud_keysum.h here and not at the top: kernels lie in the code object in the order of their definitions, and its
// split_sum_finalize stays where sinkhorn_apply_finalize was, behind the LSE kernels)
#include "cloud_keysum.h"

namespace {

constexpr int APMAX = KEYSUM_PMAX;                // contraction / output width limit of the apply pass

// Same 64 x 64 tiles as simce_grad_tiled_kernel: (1) S^T tile by the K-loop over P; (2) the plan's entries in the
// accumulator layout (keys on rows, queries on lanes), mass and cost summed per lane, the tile written once to a 16 KiB
// LDS tile; (3) bary^T[p, q] += Y^T[p, key] P^T[key, q] by key_sum_tile.h's weighted key sum.  70 KiB of LDS: two
// workgroups per CU.  Without bary the kernel stops after (2).
struct SAP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P;
  const float* scale;
  const float* u; const float* v;     // [Mx] / [Ny] scaled log-potentials
  const float* nx; const float* ny;   // [Mx] / [Ny] squared norms (cost only)
  float* slab;         // [ksplit][Mx][P] or null
  float* mass_part;    // [ksplit][Mx]
  float* cost_part;    // [ksplit][Mx] or null
  int tiles_per_split, ntiles;
};

constexpr int APPLY_LDS_ROWS = KLOOP_LDS_FLOATS + 2 * TQ;                 // K-loop buffers + mass / cost merge slots
constexpr int APPLY_LDS_FLOATS = APPLY_LDS_ROWS + KEYSUM_LDS_FLOATS;      // + plan tile + staged key block (BARY)

// BARY = false: mass and cost only - no accumulators of the second product, 21 KiB of LDS
template <bool BARY>
__global__ __launch_bounds__(256, 2) void sinkhorn_apply_kernel(const SAP p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                      // K-loop buffers
  float* mcl = smem + KLOOP_LDS_FLOATS;                                   // [mass | cost][64 queries] of key-wave 1
  float* gl = mcl + 2 * TQ;                                               // BARY: plan tile [64 keys][64 queries]
  float* yh = gl + TK * TQ;                                               // BARY: key block [16][YH_LD] / output transposes
  // This kernel keeps its own walk (KeyWalk<BKG>'s statements): on KeyWalk the <false> instantiation came out 4
  // instructions shorter with its K-loop 4 bytes further on, and the mass / cost pass measured 0.7 - 0.8 % slower at
  // 8192 x 8192 x 512 in each of three comparisons (profiles/cloud_tile/README.md).  As written here it is the
  // instruction stream it was before the fold.
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * TQ, ks = blockIdx.y;
  const int P = p.P, Ny = p.Ny;
  const float scale = p.scale[0];
  const int qg = q0 + wn * 32 + li;
  const int qc = qg < p.Mx ? qg : p.Mx - 1;
  const float u_i = p.u[qc];
  const bool want_cost = p.cost_part != nullptr;
  const float nx_i = want_cost ? p.nx[qc] : 0.f;
  f32x16 dx[4][2];                                                        // (BARY only)
  if constexpr (BARY) key_sum_zero(dx);
  float mass = 0.f, cst = 0.f;

  const float* xrows[1];
  { int q = q0 + (tid >> 2); q = q < p.Mx ? q : p.Mx - 1; xrows[0] = p.X + (long)q * P; }
  auto key_row = [&](int j) {
    j = j < Ny ? j : Ny - 1;
    return p.Y + (long)j * P;
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
    // ---- plan entries (accumulator layout: rows = keys, lanes = queries) -> LDS tile gl[key][query]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = wm * 32 + keyrow32(r, h);
      const int key = j0 + kl;
      float pv = 0.f;
      if (key < Ny && qg < p.Mx) {
        pv = expf(scale * acc[r] + u_i + p.v[key]);
        if (want_cost) cst += pv * (nx_i + p.ny[key] - 2.f * acc[r]);
      }
      mass += pv;
      if constexpr (BARY) gl[kl * TQ + wn * 32 + li] = pv;
    }
    if constexpr (BARY) key_sum_tile(dx, p.Y, Ny, P, j0, gl, yh, tid, wid, li, h);   // bary^T += Y^T P^T
  }

  __syncthreads();
  if constexpr (BARY) key_sum_store(dx, yh, p.slab, p.Mx, P, q0, ks, wid, li, h);
  // ---- mass / cost partials: lane halves, then the two key-waves
  mass += __shfl_xor(mass, 32, 64);
  cst += __shfl_xor(cst, 32, 64);
  if (wm == 1 && h == 0) { mcl[wn * 32 + li] = mass; mcl[TQ + wn * 32 + li] = cst; }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) {
    p.mass_part[(long)ks * p.Mx + qg] = mass + mcl[wn * 32 + li];
    if (want_cost) p.cost_part[(long)ks * p.Mx + qg] = cst + mcl[TQ + wn * 32 + li];
  }
}

size_t lse_workspace_bytes(const KeySplitPlan& k, int Mx) {
  return ((size_t)k.ksplit * Mx * 2 + (size_t)Mx) * sizeof(float);        // (m, l) partials, then the error terms
}

// what follows either LSE pass: the (m, l) partials at the head of the workspace -> out, the rows' error terms behind
// them -> err
int lse_finish(void* workspace, const KeySplitPlan& k, int Mx, const float* logw, const float* prev, int average, float* out,
               float* err, hipStream_t stream) {
  const float* part_ml = (const float*)workspace;
  float* err_rows = (float*)workspace + (size_t)k.ksplit * Mx * 2;
  hipLaunchKernelGGL(sinkhorn_lse_finalize, dim3((Mx + 3) / 4), dim3(256), 0, stream, part_ml, k.ksplit, Mx, logw, prev,
                     average, out, err ? err_rows : (float*)nullptr);
  int rc = clipk_check_launch();
  if (rc || !err) return rc;
  hipLaunchKernelGGL(sinkhorn_err_reduce, dim3(1), dim3(1024), 0, stream, (const float*)err_rows, Mx, err);
  return clipk_check_launch();
}

}  // namespace

extern "C" int clipk_sim_lse_bias_x3_plan(int Mx, int Ny, int* nqb, int* ksplit) {
  if (Mx <= 0 || Ny <= 0 || !nqb || !ksplit) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, PLQ);
  *nqb = k.nqb; *ksplit = k.ksplit;
  return CLIPK_OK;
}

extern "C" size_t clipk_sim_lse_bias_x3_workspace(int Mx, int Ny, int P) {
  if (!cloud_shape_ok(Mx, Ny, P, LSE_PMAX)) return 0;
  return lse_workspace_bytes(key_split_plan(Mx, Ny, PLQ), Mx);
}

extern "C" int clipk_sim_lse_bias_x3(const void* Xhi, const void* Xlo, int Mx, const void* Yhi, const void* Ylo, int Ny,
                                     int P, const float* scale, const float* bias, const float* logw, const float* prev,
                                     int average, float* out, float* err, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (!cloud_shape_ok(Mx, Ny, P, LSE_PMAX)) return CLIPK_ERR_UNSUPPORTED;
  if (!Xhi || !Xlo || !Yhi || !Ylo || !scale || !out || !workspace) return CLIPK_ERR_BAD_ARG;
  if ((average || err) && !prev) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(Xhi) || !aligned16(Xlo) || !aligned16(Yhi) || !aligned16(Ylo) || !aligned16(workspace))
    return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_lse_bias_x3_workspace(Mx, Ny, P)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, PLQ);
  SLPX p{};
  p.xh = static_cast<const unsigned short*>(Xhi); p.xl = static_cast<const unsigned short*>(Xlo); p.Mx = Mx;
  p.yh = static_cast<const unsigned short*>(Yhi); p.yl = static_cast<const unsigned short*>(Ylo); p.Ny = Ny;
  p.PP = (P + 31) & ~31; p.scale = scale; p.bias = bias; p.part_ml = (float*)workspace;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  hipLaunchKernelGGL(sinkhorn_lse_x3_kernel, dim3(k.nqb, k.ksplit), dim3(256), 0, (hipStream_t)stream, p);
  const int rc = clipk_check_launch();
  if (rc) return rc;
  return lse_finish(workspace, k, Mx, logw, prev, average, out, err, (hipStream_t)stream);
}

extern "C" int clipk_sim_lse_bias_plan(int Mx, int Ny, int* nqb, int* ksplit) {
  if (Mx <= 0 || Ny <= 0 || !nqb || !ksplit) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);
  *nqb = k.nqb; *ksplit = k.ksplit;
  return CLIPK_OK;
}

extern "C" size_t clipk_sim_lse_bias_workspace(int Mx, int Ny, int P) {
  if (!cloud_shape_ok(Mx, Ny, P, LSE_PMAX)) return 0;
  return lse_workspace_bytes(key_split_plan(Mx, Ny, TQ), Mx);
}

extern "C" int clipk_sim_lse_bias(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale,
                                  const float* bias, const float* logw, const float* prev, int average, float* out,
                                  float* err, void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (!cloud_shape_ok(Mx, Ny, P, LSE_PMAX)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !scale || !out || !workspace) return CLIPK_ERR_BAD_ARG;
  if ((average || err) && !prev) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_lse_bias_workspace(Mx, Ny, P)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);
  SLP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale; p.bias = bias; p.part_ml = (float*)workspace;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  hipLaunchKernelGGL(sinkhorn_lse_kernel, dim3(k.nqb, k.ksplit), dim3(256), 0, (hipStream_t)stream, p);
  const int rc = clipk_check_launch();
  if (rc) return rc;
  return lse_finish(workspace, k, Mx, logw, prev, average, out, err, (hipStream_t)stream);
}

extern "C" size_t clipk_sinkhorn_apply_workspace(int Mx, int Ny, int P) {
  if (!cloud_shape_ok(Mx, Ny, P, APMAX)) return 0;
  const size_t ks = key_split_plan(Mx, Ny, TQ).ksplit;
  return ks * Mx * ((size_t)P + 2) * sizeof(float);                       // bary slabs, mass and cost partials
}

extern "C" int clipk_sinkhorn_apply(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale,
                                    const float* u, const float* v, const float* nx, const float* ny, float* mass,
                                    float* bary, float* cost, void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (!cloud_shape_ok(Mx, Ny, P, APMAX)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !scale || !u || !v || !workspace || (!mass && !bary && !cost)) return CLIPK_ERR_BAD_ARG;
  if (cost && (!nx || !ny)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace) || (bary && !aligned16(bary))) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sinkhorn_apply_workspace(Mx, Ny, P)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);
  const int ks = k.ksplit;
  SAP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale; p.u = u; p.v = v; p.nx = nx; p.ny = ny;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  float* ws = (float*)workspace;
  const size_t slab_n = (size_t)ks * Mx * P;                              // (a multiple of 4 floats: the partials stay aligned)
  p.slab = bary ? ws : nullptr;
  p.mass_part = ws + slab_n;
  p.cost_part = cost ? ws + slab_n + (size_t)ks * Mx : nullptr;
  if (bary) {
    const size_t lds = (size_t)APPLY_LDS_FLOATS * sizeof(float);
    static std::atomic<uint64_t> attr_set{0};
    clipk_once_per_device(attr_set, [&] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sinkhorn_apply_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    hipLaunchKernelGGL(sinkhorn_apply_kernel<true>, dim3(k.nqb, ks), dim3(256), lds, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(sinkhorn_apply_kernel<false>, dim3(k.nqb, ks), dim3(256), (size_t)APPLY_LDS_ROWS * sizeof(float),
                       (hipStream_t)stream, p);
  }
  const int rc = clipk_check_launch();
  if (rc) return rc;
  launch_split_sum_finalize(p.slab, p.mass_part, p.cost_part, ks, Mx, P, bary, mass, cost, (hipStream_t)stream);
  return clipk_check_launch();
}
