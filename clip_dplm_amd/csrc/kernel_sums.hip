// kernel_sums.hip — row sums over a mixture of Gaussian kernels between two embedding clouds without the M x N matrix
// (include/clipk.h: clipk_kernel_sums has the formulae, the diagonal rule and the supported range).
//
//   K_ij = sum_b weights[b] exp(-gammas[b] d2_ij),  d2_ij = max(nx_i + ny_j - 2 <x_i, y_j>, 0)
//   ksum[i] = sum_j K_ij,  kbary[i, :] = sum_j K_ij y_j
//
// The structure is sinkhorn.hip's apply pass on sim_tile.h's exact-f32 64 x 64 block (keys on the MFMA rows, queries on
// the lanes): (1) the S^T tile by the K-loop over P; (2) d2 once per element, the B exponentials on it, the row sum per
// lane and - with kbary - the weight tile written once to LDS; (3) kbary^T[p, q] += Y^T[p, key] K^T[key, q] as a second
// MFMA product with the key rows staged in LDS.  Key-split slabs and row partials are summed in split order by
// kernel_sums_finalize.  One tile walk serves every bandwidth: a mixture costs B exponentials per element, not B walks.
// The values lie in (0, 1]: no running maximum.  The skipped key of a row (diag_offset) is dropped as a term - it is
// never formed and subtracted - so a self block's sum holds no trace of its computed d2_ii.
// No float atomics, no cooperative launch: results depend on the shapes and inputs alone.
#include "common.h"
#include "sim_tile.h"
#include <math.h>

namespace {

constexpr int TQ = 64, TK = 64;                   // queries per workgroup, keys per tile
constexpr int KPMAX = 512;                        // contraction / output width limit
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

constexpr int YH_LD = KPMAX + 4;                  // floats per staged key row
constexpr int KSB = 16;                           // keys per staged block of the second product
constexpr int BKG = 16;                           // K-step of the S tile (LDS budget: 2 workgroups per CU)
constexpr int KS_LDS_ROWS = 2 * 2 * 64 * (BKG + 4) + TQ;                  // K-loop buffers + the row-sum merge slots
constexpr int KS_LDS_FLOATS = KS_LDS_ROWS + TK * TQ + KSB * YH_LD;        // + weight tile + staged key block (BARY)

// BARY = false: the row sums only - no accumulators of the second product, 21 KiB of LDS
template <bool BARY>
__global__ __launch_bounds__(256, 2) void kernel_sums_kernel(const KSP p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                       // K-loop buffers
  float* mcl = smem + 2 * 2 * 64 * (BKG + 4);                             // [64 queries]: row sums of key-wave 1
  float* gl = mcl + TQ;                                                   // BARY: weight tile [64 keys][64 queries]
  float* yh = gl + TK * TQ;                                               // BARY: key block [16][YH_LD] / output transposes
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * TQ, ks = blockIdx.y;
  const int P = p.P, Ny = p.Ny, B = p.B;
  const int qg = q0 + wn * 32 + li;
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
  const int npt = (P + 127) / 128;                                        // 32-row p tiles per wave: P/4 / 32
  const int pw = npt * 32;                                                // p rows per wave
  f32x16 dx[BARY ? 4 : 1][2];
#pragma unroll
  for (int a = 0; a < (BARY ? 4 : 1); ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) dx[a][b][r] = 0.f;
  float rsum = 0.f;

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
    // squared norms of this lane's 16 key rows: fetched ahead of the K-loop where the registers allow it (not BARY)
    float nyk[16];
    auto key_norm = [&](int r) {
      const int key = j0 + wm * 32 + keyrow32(r, h);
      return p.ny[key < Ny ? key : Ny - 1];
    };
    if constexpr (!BARY) {
#pragma unroll
      for (int r = 0; r < 16; ++r) nyk[r] = key_norm(r);
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<BKG>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);          // (its first barrier also frees gl / yh)
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
    if constexpr (BARY) {
    // ---- kbary^T += Y^T K^T, the key tile in blocks of KSB keys
    for (int kb = 0; kb < TK / KSB; ++kb) {
      __syncthreads();                                                    // gl complete (kb = 0) / yh free again
      {
        // stage Y[16 keys][P]: thread -> (key = tid / 16, 16-B chunks c = tid % 16 + 16 i), loads first, then stores
        const float* yr = key_row(j0 + kb * KSB + (tid >> 4));
        float* dst = yh + (tid >> 4) * YH_LD;
#pragma unroll
        for (int g = 0; g < 2; ++g) {                                     // two groups of four: 16 staging registers
          f32x4 tmp[KPMAX / 128];
#pragma unroll
          for (int i = 0; i < KPMAX / 128; ++i) {
            const int c = (tid & 15) + 16 * (g * (KPMAX / 128) + i);
            tmp[i] = (c * 4 < P) ? ld4(yr, c * 4, P) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int i = 0; i < KPMAX / 128; ++i) {
            const int c = (tid & 15) + 16 * (g * (KPMAX / 128) + i);
            if (c * 4 < P) *reinterpret_cast<f32x4*>(dst + c * 4) = tmp[i];
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < KSB / 2; ++u) {                                 // MFMA u contracts keys 2u (h = 0) and 2u + 1
        const int kl = 2 * u + h;
        const float b0 = gl[(kb * KSB + kl) * TQ + li], b1 = gl[(kb * KSB + kl) * TQ + 32 + li];
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (a < npt) {
            const int prow = wid * pw + a * 32 + li;
            const float av = prow < P ? yh[kl * YH_LD + prow] : 0.f;
            dx[a][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, dx[a][0], 0, 0, 0);
            dx[a][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, dx[a][1], 0, 0, 0);
          }
      }
    }
    }
  }

  __syncthreads();
  if constexpr (BARY) {
    // ---- kbary^T accumulators -> [q][p] rows through LDS (one 32 x 32 block per wave at a time)
    float* tb = yh + wid * (32 * 33);
#pragma unroll
    for (int a = 0; a < 4; ++a) {                           // (fully unrolled: the accumulators are register arrays)
      if (a < npt) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 16; ++r) tb[li * 33 + keyrow32(r, h)] = dx[a][b][r];  // [query][p]
          // wave-private region: the wave's own writes are visible to its reads in program order
#pragma unroll
          for (int it = 0; it < 16; ++it) {
            const int ql = it * 2 + h;                                    // 2 query rows per pass, 32 consecutive p each
            const int q = q0 + b * 32 + ql, pp = wid * pw + a * 32 + li;
            if (q < p.Mx && pp < P) p.slab[((long)ks * p.Mx + q) * P + pp] = tb[ql * 33 + li];
          }
        }
      }
    }
  }
  // ---- row-sum partials: lane halves, then the two key-waves
  rsum += __shfl_xor(rsum, 32, 64);
  if (wm == 1 && h == 0) mcl[wn * 32 + li] = rsum;
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) p.sum_part[(long)ks * p.Mx + qg] = rsum + mcl[wn * 32 + li];
}

// slabs and row partials summed in split order (a fixed order: deterministic)
__global__ __launch_bounds__(256) void kernel_sums_finalize(const float* slab, const float* sum_part, int ksplit, int Mx,
                                                            int P, float* kbary, float* ksum) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  if (kbary) {
    const long n4 = (long)Mx * P / 4, slab_n = (long)Mx * P;
    for (long i = tid; i < n4; i += nth) {
      f32x4 a = reinterpret_cast<const f32x4*>(slab)[i];
      for (int s = 1; s < ksplit; ++s) a += reinterpret_cast<const f32x4*>(slab + (long)s * slab_n)[i];
      reinterpret_cast<f32x4*>(kbary)[i] = a;
    }
  }
  if (ksum) {
    for (long i = tid; i < Mx; i += nth) {
      float a = 0.f;
      for (int s = 0; s < ksplit; ++s) a += sum_part[(long)s * Mx + i];
      ksum[i] = a;
    }
  }
}

bool shape_ok(int Mx, int Ny, int P, int B) {
  return Mx > 0 && Ny > 0 && P > 0 && !(P & 3) && P <= KPMAX && B >= 1 && B <= KBMAX;
}

// the grid of the LSE pass (clipk_sim_lse_bias_plan); its splits are ceil(ntiles / ksplit) tiles long
void plan(int Mx, int Ny, int* nqb, int* ksplit, int* tps, int* ntiles) {
  (void)clipk_sim_lse_bias_plan(Mx, Ny, nqb, ksplit);
  *ntiles = (Ny + TK - 1) / TK;
  *tps = (*ntiles + *ksplit - 1) / *ksplit;
}

}  // namespace

extern "C" size_t clipk_kernel_sums_workspace(int Mx, int Ny, int P, int B) {
  if (!shape_ok(Mx, Ny, P, B)) return 0;
  int nqb, ks, tps, nt;
  plan(Mx, Ny, &nqb, &ks, &tps, &nt);
  return (size_t)ks * Mx * ((size_t)P + 1) * sizeof(float);               // kbary slabs, then the row-sum partials
}

extern "C" int clipk_kernel_sums(const float* X, int Mx, const float* Y, int Ny, int P, const float* gammas,
                                 const float* weights, int B, const float* nx, const float* ny, long long diag_offset,
                                 float* ksum, float* kbary, void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0 || B <= 0 || diag_offset < -1) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(Mx, Ny, P, B)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !gammas || !weights || !nx || !ny || !workspace || (!ksum && !kbary)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace) || (kbary && !aligned16(kbary))) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_kernel_sums_workspace(Mx, Ny, P, B)) return CLIPK_ERR_BAD_ARG;
  KSP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.B = B; p.gammas = gammas; p.weights = weights; p.nx = nx; p.ny = ny;
  p.diag_offset = diag_offset;
  int nqb, ks;
  plan(Mx, Ny, &nqb, &ks, &p.tiles_per_split, &p.ntiles);
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
    hipLaunchKernelGGL(kernel_sums_kernel<true>, dim3(nqb, ks), dim3(256), lds, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(kernel_sums_kernel<false>, dim3(nqb, ks), dim3(256), (size_t)KS_LDS_ROWS * sizeof(float),
                       (hipStream_t)stream, p);
  }
  int rc = clipk_check_launch();
  if (rc) return rc;
  long blocks = kbary ? ((long)Mx * P / 4 + 255) / 256 : (Mx + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(kernel_sums_finalize, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)p.slab,
                     (const float*)p.sum_part, ks, Mx, P, kbary, ksum);
  return clipk_check_launch();
}
