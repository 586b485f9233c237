// sinkhorn_sample.hip — draw j ~ P(. | i) from the entropic plan without the M x N matrix (include/clipk.h:
// clipk_sim_sample has the contract).
//
// The conditional of the plan P_ij = exp(S_ij + u_i + v_j) along a row is softmax_j(S_ij + v_j): u_i is constant along
// the row and drops out.  Adding Gumbel noise G_ij to every logit and taking the arg max draws from that softmax, so a
// draw is the tile walk of sinkhorn.hip's sinkhorn_lse_kernel (cloud_tile.h's KeyWalk: 64 queries per workgroup, 64-key
// tiles on sim_tile.h's exact-f32 block, keys on the MFMA rows, queries on the lanes, the key-range split plan of
// clipk_sim_lse_bias_plan) with a running (best value, best key) per lane in place of (max, sum):
//   z_ij = scale <x_i, y_j> + bias_j + G(seed, stream_i, j),   stream_i = stream_offset + i   (64-bit)
// The noise is a pure function of (seed, stream, key): Philox4x32-10 keyed by the seed, counter (j >> 2, stream lo,
// stream hi, 0), key j takes output word j & 3.  A lane's 16 accumulator rows are four aligned groups of four
// consecutive keys (keyrow32), so that is one Philox call per group.  U = ((w >> 9) + 0.5) 2^-23, G = -log(-log U).
// Merge rule, the same at every level (lane halves, the two key-waves, key splits in sinkhorn_sample_finalize): the
// higher z wins, equal z goes to the lower key.  The rule is associative and commutative, so the winner depends on
// (inputs, seed, stream) and never on the grid.  No float atomics, no cooperative launch.
#include "common.h"
#include "cloud_tile.h"
#include <math.h>

namespace {

constexpr int SAMPLE_PMAX = 768;                  // contraction limit (that of the LSE pass)

struct SSP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P;
  const float* scale;
  const float* bias;            // [Ny] or null (zeros)
  const long long* seed_offset; // device: {seed, stream_offset}
  float* part_z;                // [ksplit][Mx]
  int* part_k;                  // [ksplit][Mx]
  int tiles_per_split, ntiles;
};

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c = u32x4{hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// U = ((w >> 9) + 0.5) 2^-23 = (2 (w >> 9) + 1) 2^-24, exact in f32 and inside (0, 1).  -log U goes through the full
// logf (relative accuracy also next to 1, where -log U ~ 1 - U falls to 2^-24), not the bare hardware log2
__device__ __forceinline__ float gumbel(unsigned w) {
  const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
  return -logf(-logf(u));
}

__global__ __launch_bounds__(256, 2) void sinkhorn_sample_kernel(const SSP p) {
  constexpr int BKL = 32;                                                 // 16 MFMAs per wave between barriers
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (BKL + 4)];   // 2 buffers x (keys | queries)
  __shared__ float mrg_z[TQ];                                             // key-wave 1's best value / key per query
  __shared__ int mrg_k[TQ];
  const float scale = p.scale[0];
  const unsigned long long seed = (unsigned long long)p.seed_offset[0];
  const unsigned long long stream0 = (unsigned long long)p.seed_offset[1];
  const KeyWalk<BKL> w(p.X, p.Mx, nullptr, p.Mx, p.Y, p.Ny, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  const int Ny = p.Ny;
  const unsigned long long sid = stream0 + (unsigned long long)qg;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  const unsigned s_lo = (unsigned)sid, s_hi = (unsigned)(sid >> 32);
  float z_run = -INFINITY;
  int k_run = NO_KEY;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    float bk[16];                                                         // bias of this lane's 16 key rows
#pragma unroll
    for (int r = 0; r < 16; ++r) bk[r] = w.key_bias(p.bias, j0, r);
    f32x16 acc;
    w.product(j0, acc);
    // keys in rising order within the lane (tiles rise, keyrow32 rises with r): `>` keeps the lower key of a tie
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = j0 + wm * 32 + 8 * g + 4 * h;                        // keyrow32(4 g, h): four consecutive keys
      if (kb < Ny) {
        const u32x4 w = philox4x32_10(u32x4{(unsigned)kb >> 2, s_lo, s_hi, 0u}, k0, k1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float z = (scale * acc[r] + bk[r]) + gumbel(w[e]);
          if (kb + e < Ny && z > z_run) { z_run = z; k_run = kb + e; }
        }
      }
    }
  }

  // ---- merge: lane halves, then the two key-waves
  take_better(z_run, k_run, __shfl_xor(z_run, 32, 64), __shfl_xor(k_run, 32, 64));
  if (wm == 1 && h == 0) { mrg_z[wn * 32 + li] = z_run; mrg_k[wn * 32 + li] = k_run; }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < p.Mx) {
    take_better(z_run, k_run, mrg_z[wn * 32 + li], mrg_k[wn * 32 + li]);
    p.part_z[(long)ks * p.Mx + qg] = z_run;
    p.part_k[(long)ks * p.Mx + qg] = k_run;
  }
}

// one thread per query: the key-split partials in split order under the same rule
__global__ __launch_bounds__(256) void sinkhorn_sample_finalize(const float* part_z, const int* part_k, int ksplit, int Mx,
                                                                long long* idx, float* score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Mx) return;
  float z = part_z[i];
  int k = part_k[i];
  for (int s = 1; s < ksplit; ++s) take_better(z, k, part_z[(long)s * Mx + i], part_k[(long)s * Mx + i]);
  idx[i] = k;
  if (score) score[i] = z;
}

}  // namespace

extern "C" size_t clipk_sim_sample_workspace(int Mx, int Ny, int P) {
  if (!cloud_shape_ok(Mx, Ny, P, SAMPLE_PMAX)) return 0;
  const size_t ks = key_split_plan(Mx, Ny, TQ).ksplit;
  return ks * Mx * (sizeof(float) + sizeof(int));                         // best values, then best keys
}

extern "C" int clipk_sim_sample(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale,
                                const float* bias, const long long* seed_offset, long long* idx, float* score,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (!cloud_shape_ok(Mx, Ny, P, SAMPLE_PMAX)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !scale || !seed_offset || !idx || !workspace) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_sample_workspace(Mx, Ny, P)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(Mx, Ny, TQ);                      // the grid of the LSE pass
  const int ks = k.ksplit;
  SSP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale; p.bias = bias; p.seed_offset = seed_offset;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  p.part_z = (float*)workspace;
  p.part_k = (int*)(p.part_z + (size_t)ks * Mx);
  hipLaunchKernelGGL(sinkhorn_sample_kernel, dim3(k.nqb, ks), dim3(256), 0, (hipStream_t)stream, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(sinkhorn_sample_finalize, dim3((Mx + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const float*)p.part_z, (const int*)p.part_k, ks, Mx, idx, score);
  return clipk_check_launch();
}
