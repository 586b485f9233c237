// label_dist_sums.hip — per-label sums of point-to-point distances between two embedding clouds without the M x N matrix
// (include/clipk.h: clipk_label_dist_sums has the formulae, the diagonal rule and the supported range).
//
//   out[i, g] = sum over { j : labels[j] = g, j != i + diag_offset } of d(x_i, y_j)
//
// What the silhouette width is made of (clip_dplm_amd.cluster.silhouette_samples).  With the Euclidean distance the
// square root keeps the sum from reducing to cluster sums: it is an N x N tile walk with a one-hot second product.
// The structure is kernel_sums_kernel<true> with another element function and the labels in place of the key rows:
// (1) the S^T tile by the K-loop over P; (2) the distance of every element, written once to the LDS tile
// gl[key][query]; (3) out^T[g, q] += H^T[g, key] D[key, q] as the second MFMA product, H the one-hot of the tile's
// labels, staged in LDS from the labels (16 label loads per 16-key block) - no N x G one-hot matrix exists in memory.  Key-split slabs
// are summed in split order by split_sum_finalize.
// Two forms of step (3).  G > 64: the contraction of key_sum_tile.h's key_sum_tile, wave w owning label rows
// [w G/4, (w+1) G/4) - for G <= 128 that is 32 rows per wave, so few labels leave waves idle at the barriers of the four
// key blocks.  G <= 64: one or two 32-row blocks hold every label, so the four waves split the tile's 64 KEYS instead
// (16 each, one staging of the whole one-hot, two barriers in place of eight) and their partial accumulators are merged
// through LDS in wave order after the walk (measured: profiles/silhouette).
// The skipped key of a row (diag_offset) is dropped as a term - never formed and subtracted: a computed d2_ii of
// rounding size would enter as its square root.
// clipk_label_kernel_sums is the same walk with one more element function (MODE_KERNEL): the per-row Gaussian of
// tsne.hip's cond_entropy_walk, w = exp(-beta_i (d2 - shift_i)), on the d2 of the sqeuclidean mode - the label masses LISI
// is made of (clip_dplm_amd.mixing).  beta_i, c in two parts and shift_i sit in the row's lane next to nx_i.  Its finalize
// (label_kernel_finalize) also forms the row statistics, so the Mx x G result need not be written at all.
// No float atomics, no cooperative launch: results depend on the shapes and inputs alone.
#include "common.h"
#include "cloud_keysum.h"
#include <math.h>

namespace {

constexpr int LD_PMAX = KEYSUM_PMAX;              // contraction limit
constexpr int LD_GMAX = KEYSUM_PMAX;              // labels per launch: the second product's output width
constexpr int LD_GSMALL = 64;                     // at most this many labels: the key-split form of the second product
enum { MODE_EUCLIDEAN = 0, MODE_SQEUCLIDEAN = 1, MODE_COSINE = 2, MODE_KERNEL = 3 };  // 3: clipk_label_kernel_sums' own
constexpr float L_HI = 1.44269502162933349609375f, L_LO = 1.92596299112661746e-8f;   // log2(e) = L_HI + L_LO

struct LDP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P, G, Gp;                                   // Gp: G rounded up to a multiple of 4, the row stride of slab and out
  const int* labels;                              // [Ny]
  const float* nx; const float* ny;               // [Mx] / [Ny] squared norms (not read in the cosine mode)
  long long diag_offset;                          // -1: none; row i skips key i + diag_offset
  float* slab;                                    // [ksplit][Mx][Gp]
  int tiles_per_split, ntiles;
  const float* beta; const float* shift;          // MODE_KERNEL: [Mx] per-row bandwidths, [Mx] shifts or null (zeros)
};

constexpr int LD_LDS_FLOATS = KLOOP_LDS_FLOATS + KEYSUM_LDS_FLOATS;       // K-loop buffers + distance tile + staged block

// the label of key j as a column of this launch, -1 where it has none (beyond Ny, or outside [0, G))
__device__ __forceinline__ int label_column(const int* labels, int j, int Ny, int G) {
  const int lab = j < Ny ? labels[j] : -1;
  return (unsigned)lab < (unsigned)G ? lab : -1;
}

// the one-hot of 16 keys' labels in key_sum_stage's place: yh[key][g] for g < Gp.  Thread -> (key = tid / 16, 16-B chunks
// c = tid % 16 + 16 i): 16 distinct label loads per block
__device__ __forceinline__ void label_stage(const int* labels, int Ny, int G, int Gp, int j0, int kb, float* yh, int tid) {
  const int lab = label_column(labels, j0 + kb * KSB + (tid >> 4), Ny, G);
  float* dst = yh + (tid >> 4) * YH_LD;
#pragma unroll
  for (int i = 0; i < LD_GMAX / 64; ++i) {
    const int c4 = 4 * ((tid & 15) + 16 * i);
    if (c4 < Gp) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (lab == c4 + e) ? 1.f : 0.f;
      *reinterpret_cast<f32x4*>(dst + c4) = o;
    }
  }
}

// dx += yh^T[g, 16 keys] gl[16 keys of block kb, q]: wave wid's label rows, all 64 queries.  The contraction half of
// key_sum_tile.h's key_sum_tile, kept here: split out of that function it changes what its three callers compile to.
__device__ __forceinline__ void label_contract(f32x16 (&dx)[4][2], int Gp, int kb, const float* gl, const float* yh, int wid,
                                               int li, int h) {
  const int npt = (Gp + 127) / 128;                                       // 32-row label tiles per wave
  const int pw = npt * 32;                                                // label rows per wave
#pragma unroll
  for (int u = 0; u < KSB / 2; ++u) {                                     // MFMA u contracts keys 2u (h = 0) and 2u + 1
    const int kl = 2 * u + h;
    const float b0 = gl[(kb * KSB + kl) * TQ + li], b1 = gl[(kb * KSB + kl) * TQ + 32 + li];
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < npt) {
        const int prow = wid * pw + a * 32 + li;
        const float av = prow < Gp ? yh[kl * YH_LD + prow] : 0.f;
        dx[a][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, dx[a][0], 0, 0, 0);
        dx[a][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, dx[a][1], 0, 0, 0);
      }
  }
}

// NRB = 0: the row-split form of the second product (any G); NRB = 1, 2: the key-split form for G <= 32 NRB
template <int MODE, int NRB>
__global__ __launch_bounds__(256, 2) void label_dist_sums_kernel(const LDP p) {
  constexpr bool SMALLG = NRB > 0;
  constexpr int OH_LD = 32 * NRB + 4;                                     // floats per one-hot row of the key-split form
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                       // K-loop buffers
  float* gl = smem + KLOOP_LDS_FLOATS;                                    // distance tile [64 keys][64 queries]
  float* yh = gl + TK * TQ;                                               // one-hot block / merge slots / output transposes
  const KeyWalk<BKG> w(p.X, p.Mx, nullptr, p.Mx, p.Y, p.Ny, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  const int tid = w.tid, wid = w.wid, Ny = p.Ny, G = p.G, Gp = p.Gp;
  float nx_i = 0.f;
  if constexpr (MODE != MODE_COSINE) nx_i = p.nx[qg < p.Mx ? qg : p.Mx - 1];
  // MODE_KERNEL: exp(-beta t) = 2^(c t) with c = -beta log2(e) held as cg + cl, the row's own (the lane is the query), and
  // t = d - shift_i: d, t and the exponent exactly as tsne.hip's cond_entropy_walk forms them
  float cg = 0.f, cl = 0.f, sh_i = 0.f;
  if constexpr (MODE == MODE_KERNEL) {
    const int qc = qg < p.Mx ? qg : p.Mx - 1;
    const float gm = -p.beta[qc];
    cg = gm * L_HI;
    cl = fmaf(gm, L_HI, -cg) + gm * L_LO;
    sh_i = p.shift ? p.shift[qc] : 0.f;
  }
  // this query's skipped key, -1 where there is none (or it lies beyond Ny: nothing to skip)
  int skip = -1;
  if (p.diag_offset >= 0) {
    const long long sk = (long long)qg + p.diag_offset;
    if (sk < (long long)Ny) skip = (int)sk;
  }
  f32x16 dx[SMALLG ? NRB : 4][2];
#pragma unroll
  for (int a = 0; a < (SMALLG ? NRB : 4); ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) dx[a][0][r] = dx[a][1][r] = 0.f;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    f32x16 acc;
    w.product(j0, acc);                                                   // (its first barrier also frees gl / yh)
    // ---- distances (accumulator layout: rows = keys, lanes = queries) -> LDS tile gl[key][query]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = wm * 32 + keyrow32(r, h);
      const int key = j0 + kl;
      float d;
      if constexpr (MODE == MODE_COSINE) {
        d = fmaxf(1.f - acc[r], 0.f);
      } else {
        const float ny_j = p.ny[key < Ny ? key : Ny - 1];
        d = fmaxf(fmaf(-2.f, acc[r], nx_i + ny_j), 0.f);
        if constexpr (MODE == MODE_EUCLIDEAN) d = __builtin_amdgcn_sqrtf(d);          // v_sqrt_f32: 1 ulp
        if constexpr (MODE == MODE_KERNEL) {
          const float t = d - sh_i;
          d = __builtin_amdgcn_exp2f(fmaf(cg, t, cl * t));                            // one v_exp_f32, no division
        }
      }
      if (key >= Ny || qg >= p.Mx || key == skip) d = 0.f;                // the term is dropped, not subtracted
      gl[kl * TQ + wn * 32 + li] = d;
    }
    // ---- out^T += H^T D
    if constexpr (SMALLG) {
      // the one-hot of all 64 keys, oh[key][32 NRB labels]: thread -> (key = tid / 4, 8 NRB columns)
      {
        const int lab = label_column(p.labels, j0 + (tid >> 2), Ny, G);
        const int c0 = (tid & 3) * 8 * NRB;
        float* dst = yh + (tid >> 2) * OH_LD + c0;
#pragma unroll
        for (int i4 = 0; i4 < 2 * NRB; ++i4) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (lab == c0 + 4 * i4 + e) ? 1.f : 0.f;
          *reinterpret_cast<f32x4*>(dst + 4 * i4) = o;
        }
      }
      __syncthreads();                                                    // gl and oh complete
#pragma unroll
      for (int u = 0; u < KSB / 2; ++u) {                                 // wave wid contracts keys [16 wid, +16)
        const int kl = wid * KSB + 2 * u + h;
        const float b0 = gl[kl * TQ + li], b1 = gl[kl * TQ + 32 + li];
#pragma unroll
        for (int a = 0; a < NRB; ++a) {
          const float av = yh[kl * OH_LD + a * 32 + li];
          dx[a][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, dx[a][0], 0, 0, 0);
          dx[a][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, dx[a][1], 0, 0, 0);
        }
      }
    } else {
      for (int kb = 0; kb < TK / KSB; ++kb) {
        __syncthreads();                                                  // gl complete (kb = 0) / yh free again
        label_stage(p.labels, Ny, G, Gp, j0, kb, yh, tid);
        __syncthreads();
        label_contract(dx, Gp, kb, gl, yh, wid, li, h);
      }
    }
  }

  __syncthreads();
  if constexpr (SMALLG) {
    // ---- the four waves' key partials, added in wave order; then rows [q][g] of this split's slab from wave 0.
    // The merge slots [wave 1..3][block a][half b][r][lane] lie over gl and yh (contiguous, free after the barrier).
    constexpr int WSLOT = NRB * 2 * 16 * 64;
    static_assert(3 * WSLOT <= KEYSUM_LDS_FLOATS && 64 * OH_LD <= KSB * YH_LD, "merge slots / one-hot within gl + yh");
    if (wid > 0) {
      float* mrg = gl + (wid - 1) * WSLOT;
#pragma unroll
      for (int a = 0; a < NRB; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) mrg[((a * 2 + b) * 16 + r) * 64 + (tid & 63)] = dx[a][b][r];
    }
    __syncthreads();
    if (wid == 0) {
      for (int ow = 0; ow < 3; ++ow)
#pragma unroll
        for (int a = 0; a < NRB; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) dx[a][b][r] += gl[ow * WSLOT + ((a * 2 + b) * 16 + r) * 64 + tid];
#pragma unroll
      for (int a = 0; a < NRB; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int q = w.q0 + b * 32 + li;
#pragma unroll
          for (int i4 = 0; i4 < 4; ++i4) {                                // accumulator rows 4 i4 .. + 3: labels g0 .. g0 + 3
            const int g0 = a * 32 + keyrow32(4 * i4, h);
            if (q < p.Mx && g0 < Gp) {
              const f32x4 v = {dx[a][b][4 * i4], dx[a][b][4 * i4 + 1], dx[a][b][4 * i4 + 2], dx[a][b][4 * i4 + 3]};
              *reinterpret_cast<f32x4*>(p.slab + ((long)ks * p.Mx + q) * Gp + g0) = v;
            }
          }
        }
    }
  } else {
    // (the thread index through an opaque copy: the store's address arithmetic starts here and holds no register - nor a
    // spill slot - across the walk)
    int t2 = tid;
    asm volatile("" : "+v"(t2));
    key_sum_store(dx, yh, p.slab, p.Mx, Gp, w.q0, ks, t2 >> 6, t2 & 31, (t2 >> 5) & 1);
  }
}

bool shape_ok(int Mx, int Ny, int P, int G) {
  return cloud_shape_ok(Mx, Ny, P, LD_PMAX) && G >= 1 && G <= LD_GMAX;
}

template <int MODE, int NRB>
void launch_walk(const LDP& p, dim3 grid, hipStream_t stream) {
  const size_t lds = (size_t)LD_LDS_FLOATS * sizeof(float);
  static std::atomic<uint64_t> attr_set{0};
  clipk_once_per_device(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(label_dist_sums_kernel<MODE, NRB>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  hipLaunchKernelGGL((label_dist_sums_kernel<MODE, NRB>), grid, dim3(256), lds, stream, p);
}

template <int MODE>
void launch_mode(const LDP& p, dim3 grid, hipStream_t stream) {
  if (p.G <= 32) launch_walk<MODE, 1>(p, grid, stream);
  else if (p.G <= LD_GSMALL) launch_walk<MODE, 2>(p, grid, stream);
  else launch_walk<MODE, 0>(p, grid, stream);
}

// the walk of either entry on the grid of the LSE pass: p without its plan and slab
void launch_label_walk(LDP& p, int mode, const KeySplitPlan& k, void* workspace, hipStream_t stream) {
  p.Gp = (p.G + 3) & ~3;
  p.slab = (float*)workspace;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  const dim3 grid(k.nqb, k.ksplit);
  if (mode == MODE_EUCLIDEAN) launch_mode<MODE_EUCLIDEAN>(p, grid, stream);
  else if (mode == MODE_SQEUCLIDEAN) launch_mode<MODE_SQEUCLIDEAN>(p, grid, stream);
  else if (mode == MODE_COSINE) launch_mode<MODE_COSINE>(p, grid, stream);
  else launch_mode<MODE_KERNEL>(p, grid, stream);
}

// clipk_label_kernel_sums' finalize, one row per thread: the key-split slabs in split order, label by label in ascending
// order; out (null: never written), and from the same summed values mass = sum_g, sumsq = sum_g ^2, the arg max (equal
// values: the lower label) and its value.  The values are sums of non-negative terms: -1 loses to every one of them.
__global__ __launch_bounds__(256) void label_kernel_finalize(const float* slab, int ksplit, int Mx, int G, int Gp, float* out,
                                                             float* mass, float* sumsq, int* top, float* best) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  const long slab_n = (long)Mx * Gp;
  for (long i = tid; i < Mx; i += nth) {
    float m = 0.f, q = 0.f, bv = -1.f;
    int bg = 0;
    for (int g4 = 0; g4 < Gp; g4 += 4) {
      const long at = i * Gp + g4;
      f32x4 a = *reinterpret_cast<const f32x4*>(slab + at);
      for (int s = 1; s < ksplit; ++s) a += *reinterpret_cast<const f32x4*>(slab + (long)s * slab_n + at);
      if (out) *reinterpret_cast<f32x4*>(out + at) = a;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (g4 + e < G) {
          m += a[e];
          q = fmaf(a[e], a[e], q);
          if (a[e] > bv) { bv = a[e]; bg = g4 + e; }
        }
    }
    if (mass) mass[i] = m;
    if (sumsq) sumsq[i] = q;
    if (top) top[i] = bg;
    if (best) best[i] = bv;
  }
}

}  // namespace

extern "C" size_t clipk_label_dist_sums_workspace(int Mx, int Ny, int P, int G) {
  if (!shape_ok(Mx, Ny, P, G)) return 0;
  const size_t ks = key_split_plan(Mx, Ny, TQ).ksplit;
  return ks * Mx * (size_t)((G + 3) & ~3) * sizeof(float);                // the slabs
}

extern "C" int clipk_label_dist_sums(const float* X, int Mx, const float* Y, int Ny, int P, const int* labels, int G,
                                     int mode, const float* nx, const float* ny, long long diag_offset, float* out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0 || G <= 0 || diag_offset < -1 || mode < 0 || mode > MODE_COSINE) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(Mx, Ny, P, G)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !labels || !out || !workspace || (mode != MODE_COSINE && (!nx || !ny))) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(out) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_label_dist_sums_workspace(Mx, Ny, P, G)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);                      // the grid of the LSE pass
  LDP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.G = G; p.labels = labels; p.nx = nx; p.ny = ny;
  p.diag_offset = diag_offset;
  launch_label_walk(p, mode, k, workspace, (hipStream_t)stream);
  int rc = clipk_check_launch();
  if (rc) return rc;
  launch_split_sum_finalize(p.slab, nullptr, nullptr, k.ksplit, Mx, p.Gp, out, nullptr, nullptr, (hipStream_t)stream);
  return clipk_check_launch();
}

extern "C" size_t clipk_label_kernel_sums_workspace(int Mx, int Ny, int P, int G) {
  return clipk_label_dist_sums_workspace(Mx, Ny, P, G);                   // the same slabs
}

extern "C" int clipk_label_kernel_sums(const float* X, int Mx, const float* Y, int Ny, int P, const int* labels, int G,
                                       const float* beta, const float* shift, const float* nx, const float* ny,
                                       long long diag_offset, float* out, float* mass, float* sumsq, int* top, float* best,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0 || G <= 0 || diag_offset < -1) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(Mx, Ny, P, G)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !labels || !beta || !nx || !ny || !workspace) return CLIPK_ERR_BAD_ARG;
  if (!out && !mass && !sumsq && !top && !best) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || (out && !aligned16(out)) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_label_kernel_sums_workspace(Mx, Ny, P, G)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);                      // the grid of the LSE pass
  LDP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.G = G; p.labels = labels; p.nx = nx; p.ny = ny;
  p.diag_offset = diag_offset; p.beta = beta; p.shift = shift;
  launch_label_walk(p, MODE_KERNEL, k, workspace, (hipStream_t)stream);
  int rc = clipk_check_launch();
  if (rc) return rc;
  int blocks = (Mx + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(label_kernel_finalize, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p.slab, k.ksplit, Mx, G, p.Gp, out,
                     mass, sumsq, top, best);
  return clipk_check_launch();
}
