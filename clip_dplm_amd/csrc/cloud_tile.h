// cloud_tile.h — what the point-cloud kernels (sinkhorn.hip, sinkhorn_sample.hip, auction.hip, kernel_sums.hip, kmeans.hip,
// label_dist_sums.hip) and the tiled InfoNCE kernels (simce_tiled.hip, simce_hard.hip) share on top of sim_tile.h's
// exact-f32 64 x 64 block (keys on the MFMA rows, queries on the lanes):
//   * KeyWalk: one workgroup's walk over the 64-key tiles of its key split - coordinates, staging rows, the S^T product;
//     with CACHE the key list is two segments, batch keys and cache keys (the InfoNCE kernels);
//   * key_split_plan: the (query block, key split) grid on the host (simce.hip, linear_ce_tiled.hip take it from here
//     too); cloud_shape_ok: the shapes the passes accept;
//   * NO_KEY, better_key, take_better: the (value, key) order of the sampler's and the top-two pass's merges.
// Each kernel keeps what it does with the products, its merge rule and its own partial format.  The weighted key sum
// behind the walk is in key_sum_tile.h; sinkhorn_apply_kernel has the walk in its own body.
#pragma once
#include "common.h"
#include "sim_tile.h"

namespace {

constexpr int TQ = 64, TK = 64;                   // queries per workgroup, keys per tile
constexpr int NO_KEY = 0x7fffffff;                // loses every tie: a lane that saw no key below Ny

// what the f32 passes accept: positive sizes, rows of whole 16-byte chunks, a contraction of at most pmax
inline bool cloud_shape_ok(int Mx, int Ny, int P, int pmax) { return Mx > 0 && Ny > 0 && P > 0 && !(P & 3) && P <= pmax; }

// The order of (value, key) pairs, the same at every merge level: the higher value wins, equal values go to the lower key.
__device__ __forceinline__ bool better_key(float zo, int ko, float z, int k) { return zo > z || (zo == z && ko < k); }

__device__ __forceinline__ void take_better(float& z, int& k, float zo, int ko) {
  if (better_key(zo, ko, z, k)) { z = zo; k = ko; }
}

// ------------------------------------------------------------------------------------------------ key-split plan
struct KeySplitPlan { int nqb, ksplit, tiles_per_split, ntiles; };

// one workgroup per (query_block-query block, key split); splits so that the grid holds >= 2 workgroups per CU.
// problems > 1: that many same-shape problems in one grid (blockIdx.z = problem); the splits are chosen for the WHOLE
// grid nqb x ksplit x problems, not as if each problem had the chip to itself
inline KeySplitPlan key_split_plan(int M, int N, int query_block, int problems = 1) {
  KeySplitPlan k;
  k.nqb = (M + query_block - 1) / query_block;
  k.ntiles = (N + TK - 1) / TK;
  const int wgs = k.nqb * (problems > 0 ? problems : 1);
  int ks = (512 + wgs - 1) / wgs;
  if (ks > k.ntiles) ks = k.ntiles;
  if (ks < 1) ks = 1;
  k.tiles_per_split = (k.ntiles + ks - 1) / ks;
  k.ksplit = (k.ntiles + k.tiles_per_split - 1) / k.tiles_per_split;
  return k;
}

// ------------------------------------------------------------------------------------------------ tile walk
// Workgroup (blockIdx.x, blockIdx.y) = (query block, key split), 256 threads.  Wave (wm, wn) holds keys [32 wm, +32) x
// queries [32 wn, +32) of each tile; lane li of half h holds query position qg and the 16 keys key(j0, r).  BKT is the
// K-step of s_tile: 32 (16 MFMAs per wave between barriers) or 16 (half the LDS, for kernels that need the rest).
// CACHE: keys [Ny, Nk) are the rows of a second segment Yc (the InfoNCE cache); without it Nk = Ny and Yc is unused.
template <int BKT, bool CACHE = false>
struct KeyWalk {
  const float* Y; int Ny, P;
  const float* Yc; int Nk;                        // CACHE: the second key segment, the length of the whole key list
  float* smem;                                    // 2 buffers x (keys | queries) x 64 x (BKT + 4) floats
  int tid, wid, wm, wn, li, h;
  int q0, ks, qg;
  int t_beg, t_end;                               // this split's tiles
  const float* xrows[BKT / 16];                   // this thread's query staging rows

  // Query position q < nrows stands for row rows[q] of X [Mx][P], or for row q without a list (then nrows <= Mx).
  // Positions beyond nrows are clamped: computed and dropped by the caller.
  __device__ __forceinline__ KeyWalk(const float* X, int Mx, const int* rows, int nrows, const float* Y_, int Ny_, int P_,
                                     int tiles_per_split, int ntiles, float* smem_, const float* Yc_ = nullptr, int Nc = 0)
      : Y(Y_), Ny(Ny_), P(P_), Yc(Yc_), Nk(Ny_ + Nc), smem(smem_) {
    tid = threadIdx.x; wid = tid >> 6;
    const int lane = tid & 63;
    wm = wid >> 1; wn = wid & 1;                                          // key half, query half
    li = lane & 31; h = lane >> 5;
    q0 = blockIdx.x * TQ; ks = blockIdx.y;
    qg = q0 + wn * 32 + li;
#pragma unroll
    for (int i = 0; i < BKT / 16; ++i) {
      int q = q0 + (tid + i * 256) / (BKT / 4); q = q < nrows ? q : nrows - 1;
      if (rows) {
        q = rows[q];
        q = q < 0 ? 0 : (q < Mx ? q : Mx - 1);                            // a bad list entry reads a valid row
      }
      xrows[i] = X + (long)q * P;
    }
    t_beg = ks * tiles_per_split;
    t_end = t_beg + tiles_per_split; t_end = t_end < ntiles ? t_end : ntiles;
  }

  __device__ __forceinline__ const float* key_row(int j) const {
    if constexpr (CACHE) {
      j = j < Nk ? j : Nk - 1;                                            // clamped: masked in the caller's epilogue
      return (j < Ny) ? Y + (long)j * P : Yc + (long)(j - Ny) * P;
    } else {
      j = j < Ny ? j : Ny - 1;                                            // clamped: masked in the caller's epilogue
      return Y + (long)j * P;
    }
  }

  // the key of accumulator row r of the tile at j0
  __device__ __forceinline__ int key(int j0, int r) const { return j0 + wm * 32 + keyrow32(r, h); }

  // bias of key(j0, r) (null: zeros, as beyond Ny), for the lane's 16 key rows ahead of the product.  The loop over r
  // stays with the caller: as a loop in here the 16 loads compile to 16 address computations in place of one base with
  // immediate offsets (sinkhorn_lse_kernel: +50 instructions, +16 VGPRs).
  __device__ __forceinline__ float key_bias(const float* bias, int j0, int r) const {
    const int k = key(j0, r);
    return (bias && k < Ny) ? bias[k] : 0.f;
  }

  // acc[r] = <y_key(j0, r), x_qg>.  Starts and ends with a barrier (s_tile): LDS the workgroup read before the call is
  // free once it has begun.
  __device__ __forceinline__ void product(int j0, f32x16& acc) const {
    const float* yrows[BKT / 16];
#pragma unroll
    for (int i = 0; i < BKT / 16; ++i) yrows[i] = key_row(j0 + (tid + i * 256) / (BKT / 4));
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<BKT>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
  }
};

}  // namespace
