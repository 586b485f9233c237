// kernel_sums.hip — row sums over a mixture of Gaussian kernels between two embedding clouds without the M x N matrix
// (include/clipk.h: clipk_kernel_sums has the formulae, the diagonal rule and the supported range).
//
//   K_ij = sum_b weights[b] exp(-gammas[b] d2_ij),  d2_ij = max(nx_i + ny_j - 2 <x_i, y_j>, 0)
//   ksum[i] = sum_j K_ij,  kbary[i, :] = sum_j K_ij y_j
//
// The structure is sinkhorn.hip's apply pass, built from the same pieces of cloud_tile.h on sim_tile.h's exact-f32
// 64 x 64 block (keys on the MFMA rows, queries on the lanes): (1) the S^T tile by the K-loop over P; (2) d2 once per
// element, the B exponentials on it, the row sum per lane and - with kbary - the weight tile written once to LDS;
// (3) kbary^T[p, q] += Y^T[p, key] K^T[key, q] by the weighted key sum.  Key-split slabs and row partials are summed in
// split order by split_sum_finalize.  One tile walk serves every bandwidth: a mixture costs B exponentials per element,
// not B walks.
// The values lie in (0, 1]: no running maximum.  The skipped key of a row (diag_offset) is dropped as a term - it is
// never formed and subtracted - so a self block's sum holds no trace of its computed d2_ii.
// No float atomics, no cooperative launch: results depend on the shapes and inputs alone.
#include "common.h"
#include "cloud_keysum.h"
#include <math.h>

namespace {

constexpr int KPMAX = KEYSUM_PMAX;                // contraction / output width limit
constexpr int KBMAX = 8;                          // bandwidths per launch

struct KSP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P, B;
  const float* gammas; const float* weights;      // [B], device
  const float* nx; const float* ny;               // [Mx] / [Ny] squared norms
  long long diag_offset;                          // -1: none; row i skips key i + diag_offset
  float* slab;         // [ksplit][Mx][P] or null
  float* sum_part;     // [ksplit][Mx]
  int tiles_per_split, ntiles;
};

constexpr int KS_LDS_ROWS = KLOOP_LDS_FLOATS + TQ;                        // K-loop buffers + the row-sum merge slots
constexpr int KS_LDS_FLOATS = KS_LDS_ROWS + KEYSUM_LDS_FLOATS;            // + weight tile + staged key block (BARY)

// BARY = false: the row sums only - no accumulators of the second product, 21 KiB of LDS
template <bool BARY>
__global__ __launch_bounds__(256, 2) void kernel_sums_kernel(const KSP p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                       // K-loop buffers
  float* mcl = smem + KLOOP_LDS_FLOATS;                                   // [64 queries]: row sums of key-wave 1
  float* gl = mcl + TQ;                                                   // BARY: weight tile [64 keys][64 queries]
  float* yh = gl + TK * TQ;                                               // BARY: key block [16][YH_LD] / output transposes
  const KeyWalk<BKG> w(p.X, p.Mx, nullptr, p.Mx, p.Y, p.Ny, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  const int lane = w.tid & 63;
  const int Ny = p.Ny, B = p.B;
  const int qc = qg < p.Mx ? qg : p.Mx - 1;
  const float nx_i = p.nx[qc];
  // exp(-gamma d2) = 2^(c d2) with c = -gamma log2(e) held as cg + cl (log2(e) = L_HI + L_LO, the product's own rounding
  // error in cl): one rounding of c would be the same relative error of every exponent of a bandwidth - a shifted gamma,
  // which does not average out over a sum as the per-element roundings do.  Lane b of every wave holds bandwidth b's
  // constants; the loop over the B bandwidths (a run-time count) reads them back with v_readlane.
  constexpr float L_HI = 1.44269502162933349609375f, L_LO = 1.92596299112661746e-8f;
  float cgv = 0.f, clv = 0.f, wgv = 0.f;
  if (lane < B) {
    const float gm = -p.gammas[lane];
    cgv = gm * L_HI;
    clv = fmaf(gm, L_HI, -cgv) + gm * L_LO;
    wgv = p.weights[lane];
  }
  auto lane_value = [](float v, int b) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b)); };
  // this query's skipped key, -1 where there is none (or it lies beyond Ny: nothing to skip)
  int skip = -1;
  if (p.diag_offset >= 0) {
    const long long sk = (long long)qg + p.diag_offset;
    if (sk < (long long)Ny) skip = (int)sk;
  }
  f32x16 dx[4][2];                                                        // (BARY only)
  if constexpr (BARY) key_sum_zero(dx);
  float rsum = 0.f;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    // squared norms of this lane's 16 key rows: fetched ahead of the K-loop where the registers allow it (not BARY)
    float nyk[16];
    auto key_norm = [&](int r) {
      const int key = w.key(j0, r);
      return p.ny[key < Ny ? key : Ny - 1];
    };
    if constexpr (!BARY) {
#pragma unroll
      for (int r = 0; r < 16; ++r) nyk[r] = key_norm(r);
    }
    f32x16 acc;
    w.product(j0, acc);                                                   // (its first barrier also frees gl / yh)
    // ---- kernel values (accumulator layout: rows = keys, lanes = queries) -> LDS tile gl[key][query]
    float d2[16], kv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ny_j = BARY ? key_norm(r) : nyk[r];
      d2[r] = fmaxf(fmaf(-2.f, acc[r], nx_i + ny_j), 0.f);
      kv[r] = 0.f;
    }
    for (int b = 0; b < B; ++b) {                                         // d2 once, B exponentials on it
      const float cg = lane_value(cgv, b), cl = lane_value(clv, b), wg = lane_value(wgv, b);
#pragma unroll
      for (int r = 0; r < 16; ++r) kv[r] = fmaf(wg, __builtin_amdgcn_exp2f(fmaf(cg, d2[r], cl * d2[r])), kv[r]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = wm * 32 + keyrow32(r, h);
      const int key = j0 + kl;
      if (key >= Ny || qg >= p.Mx || key == skip) kv[r] = 0.f;            // the term is dropped, not subtracted
      rsum += kv[r];
      if constexpr (BARY) gl[kl * TQ + wn * 32 + li] = kv[r];
    }
    if constexpr (BARY)                                                   // kbary^T += Y^T K^T
      key_sum_tile(dx, p.Y, Ny, p.P, j0, gl, yh, w.tid, w.wid, li, h);
  }

  __syncthreads();
  if constexpr (BARY) key_sum_store(dx, yh, p.slab, p.Mx, p.P, w.q0, ks, w.wid, li, h);
  // ---- row-sum partials: lane halves, then the two key-waves
  rsum += __shfl_xor(rsum, 32, 64);
  if (wm == 1 && h == 0) mcl[wn * 32 + li] = rsum;
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) p.sum_part[(long)ks * p.Mx + qg] = rsum + mcl[wn * 32 + li];
}

bool shape_ok(int Mx, int Ny, int P, int B) {
  return Mx > 0 && Ny > 0 && P > 0 && !(P & 3) && P <= KPMAX && B >= 1 && B <= KBMAX;
}

}  // namespace

extern "C" size_t clipk_kernel_sums_workspace(int Mx, int Ny, int P, int B) {
  if (!shape_ok(Mx, Ny, P, B)) return 0;
  const size_t ks = key_split_plan(Mx, Ny, TQ).ksplit;
  return ks * Mx * ((size_t)P + 1) * sizeof(float);                       // kbary slabs, then the row-sum partials
}

extern "C" int clipk_kernel_sums(const float* X, int Mx, const float* Y, int Ny, int P, const float* gammas,
                                 const float* weights, int B, const float* nx, const float* ny, long long diag_offset,
                                 float* ksum, float* kbary, void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0 || B <= 0 || diag_offset < -1) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(Mx, Ny, P, B)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !gammas || !weights || !nx || !ny || !workspace || (!ksum && !kbary)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace) || (kbary && !aligned16(kbary))) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_kernel_sums_workspace(Mx, Ny, P, B)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);                      // the grid of the LSE pass
  const int ks = k.ksplit;
  KSP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.B = B; p.gammas = gammas; p.weights = weights; p.nx = nx; p.ny = ny;
  p.diag_offset = diag_offset;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  float* ws = (float*)workspace;
  const size_t slab_n = (size_t)ks * Mx * P;                              // (a multiple of 4 floats: the partials stay aligned)
  p.slab = kbary ? ws : nullptr;
  p.sum_part = ws + slab_n;
  if (kbary) {
    const size_t lds = (size_t)KS_LDS_FLOATS * sizeof(float);
    static std::atomic<uint64_t> attr_set{0};
    clipk_once_per_device(attr_set, [&] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_sums_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    hipLaunchKernelGGL(kernel_sums_kernel<true>, dim3(k.nqb, ks), dim3(256), lds, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(kernel_sums_kernel<false>, dim3(k.nqb, ks), dim3(256), (size_t)KS_LDS_ROWS * sizeof(float),
                       (hipStream_t)stream, p);
  }
  int rc = clipk_check_launch();
  if (rc) return rc;
  launch_split_sum_finalize(p.slab, p.sum_part, nullptr, ks, Mx, P, kbary, ksum, nullptr, (hipStream_t)stream);
  return clipk_check_launch();
}
