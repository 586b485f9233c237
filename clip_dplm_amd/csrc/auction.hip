// auction.hip — the exact (non-entropic) coupling of two equal-size clouds by the auction algorithm without the N x N
// matrix (include/clipk.h: clipk_sim_top2_bias and clipk_auction_rounds have the contracts).
//
// A bidding round needs, for every still-unassigned row i, the best and the second-best value of
//   z_ij = 2 <x_i, y_j> - |y_j|^2 - price_j = 2 <x_i, y_j> + bias_j
// over all keys j: the tile walk of sinkhorn_sample.hip's sinkhorn_sample_kernel without the Philox part (cloud_tile.h's
// KeyWalk: 64 queries per workgroup, 64-key tiles on sim_tile.h's exact-f32 block, keys on the MFMA rows, queries on the
// lanes) with a running (best, arg best, runner-up) per lane, over a LIST of query rows whose length is read from device
// memory.
// Merge rule of (z1, k1, z2) triples, the same at every level (within a lane, lane halves, the two key-waves, key splits
// in the finalize launch): the higher z1 wins, equal z1 goes to the lower key, the runner-up is the maximum of what is
// left (the loser's z1, the winner's z2).  A triple stands for (the first element under the order (z down, key up), the
// largest value among the others) of a multiset, so the merge is associative and commutative and the result depends on
// the inputs alone, never on the grid or on n_active.  No float atomics, no cooperative launch.
//
// The key split is this entry's own: late auction rounds have ONE query block walking every key, and the plan of
// clipk_sim_lse_bias (splits for >= 512 workgroups at the FULL row count, which is what sizes the grid when the active
// count lives in device memory) would leave that block a handful of long serial walks.  Here a split is TOP2_TPS tiles
// (longer only beyond 256 splits) whatever the row count (DESIGN.md §3.15 has the measurement); blocks beyond n_active
// return before their first barrier.
//
// One auction round is three launches (offers [N] 64-bit words are zero between rounds; the first launch of a call
// clears them without reading, so the workspace may hold anything and the call enqueues kernels only):
//   auction_resolve_compact  one workgroup: every key with an offer frees its previous owner, takes the winner and lowers
//                            its bias by the offer (sets `stalled` when that leaves the bias unchanged), clears the offer;
//                            then the unassigned rows are compacted in rising row order and counted
//   top2_kernel              the bids of the listed rows (scale 2, the device count)
//   top2_finalize            merges the key splits and offers inc = gap + eps to the chosen key: a 64-bit integer
//                            atomicMax on (bits of inc, complement of the row) - inc >= 0, so its bit pattern is ordered,
//                            the larger offer wins, an equal offer goes to the lower row, and integer max does not depend
//                            on the order of arrival
// and a call ends with one more auction_resolve_compact, which leaves the state consistent and the count current.
#include "common.h"
#include "cloud_tile.h"
#include <math.h>

#ifndef TOP2_TPS
#define TOP2_TPS 2                                 // 64-key tiles per key split
#endif

namespace {

constexpr int TOP2_PMAX = 768;                    // contraction limit (that of the LSE pass)
constexpr int AUCTION_NMAX = 65536;               // one workgroup compacts the rows
constexpr int RC_THREADS = 1024;
constexpr int TOP2_KSMAX = 256;                   // key splits at most: one per CU

struct T2P {
  const float* X; int Mx;
  const int* rows; int Mr;      // list of query rows (null: 0 .. Mr - 1)
  const int* n_active;          // device count (null: Mr)
  const float* Y; int Ny;
  int P;
  const float* scale;
  const float* bias;            // [Ny] or null (zeros)
  float* part_z1;               // [ksplit][Mr]
  int* part_k;                  // [ksplit][Mr]
  float* part_z2;               // [ksplit][Mr]
  int tiles_per_split, ntiles;
};

__device__ __forceinline__ int active_count(const int* n_active, int Mr) {
  if (!n_active) return Mr;
  const int n = n_active[0];
  return n < 0 ? 0 : (n < Mr ? n : Mr);
}

// (z1, k1, z2) <- merge with (zo1, ko, zo2)
__device__ __forceinline__ void merge_top2(float& z1, int& k1, float& z2, float zo1, int ko, float zo2) {
  if (better_key(zo1, ko, z1, k1)) { z2 = fmaxf(z1, zo2); z1 = zo1; k1 = ko; }
  else z2 = fmaxf(z2, zo1);
}

__global__ __launch_bounds__(256, 2) void top2_kernel(const T2P p) {
  constexpr int BKL = 32;                                                 // 16 MFMAs per wave between barriers
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (BKL + 4)];   // 2 buffers x (keys | queries)
  __shared__ float mrg_z1[TQ], mrg_z2[TQ];                                // key-wave 1's triple per query
  __shared__ int mrg_k[TQ];
  const int q0 = blockIdx.x * TQ;
  const int na = active_count(p.n_active, p.Mr);
  if (q0 >= na) return;                                                   // the whole workgroup, before any barrier
  const float scale = p.scale[0];
  const KeyWalk<BKL> w(p.X, p.Mx, p.rows, na, p.Y, p.Ny, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;   // qg: this lane's list position
  float z1 = -INFINITY, z2 = -INFINITY;
  int k1 = NO_KEY;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    float bk[16];                                                         // bias of this lane's 16 key rows
#pragma unroll
    for (int r = 0; r < 16; ++r) bk[r] = w.key_bias(p.bias, j0, r);
    f32x16 acc;
    w.product(j0, acc);
    // keys in rising order within the lane (tiles rise, keyrow32 rises with r): `>` keeps the lower key of a tie, and
    // the tied value becomes the runner-up
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = w.key(j0, r);
      const float z = scale * acc[r] + bk[r];
      if (key < p.Ny) {
        if (z > z1) { z2 = z1; z1 = z; k1 = key; }
        else z2 = fmaxf(z2, z);
      }
    }
  }

  // ---- merge: lane halves, then the two key-waves
  merge_top2(z1, k1, z2, __shfl_xor(z1, 32, 64), __shfl_xor(k1, 32, 64), __shfl_xor(z2, 32, 64));
  if (wm == 1 && h == 0) { mrg_z1[wn * 32 + li] = z1; mrg_k[wn * 32 + li] = k1; mrg_z2[wn * 32 + li] = z2; }
  __syncthreads();
  if (wm == 0 && h == 0 && qg < na) {
    merge_top2(z1, k1, z2, mrg_z1[wn * 32 + li], mrg_k[wn * 32 + li], mrg_z2[wn * 32 + li]);
    const long o = (long)ks * p.Mr + qg;
    p.part_z1[o] = z1; p.part_k[o] = k1; p.part_z2[o] = z2;
  }
}

// one thread per list position: the key-split partials under the same rule.  With `offers` (an auction round) the bid
// goes straight to the chosen key: inc = gap + eps[0] from list row rows[r]
__global__ __launch_bounds__(256) void top2_finalize(const float* part_z1, const int* part_k, const float* part_z2, int ksplit,
                                                     int Mr, int Ny, const int* n_active, int* idx, float* best, float* gap,
                                                     const int* rows, const float* eps, unsigned long long* offers) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= active_count(n_active, Mr)) return;
  float z1 = part_z1[r], z2 = part_z2[r];
  int k1 = part_k[r];
  for (int s = 1; s < ksplit; ++s) {
    const long o = (long)s * Mr + r;
    merge_top2(z1, k1, z2, part_z1[o], part_k[o], part_z2[o]);
  }
  const float g = z1 - z2;                                                // + inf with a single key
  if (idx) idx[r] = k1;
  if (best) best[r] = z1;
  if (gap) gap[r] = g;
  if (offers && (unsigned)k1 < (unsigned)Ny) {                            // (no key at all: every value was NaN or -inf)
    const float inc = g + eps[0];
    const unsigned row = (unsigned)rows[r];
    atomicMax(&offers[k1], ((unsigned long long)__float_as_uint(inc) << 32) | (unsigned long long)(~row));
  }
}

// ---- one workgroup: resolve the offers of the round before, then compact the unassigned rows in rising row order.
// Every thread owns a run of `chunk` consecutive rows / keys (N <= 65536: at most 64).
__global__ __launch_bounds__(RC_THREADS) void auction_resolve_compact(int N, int* assigned, int* owner, float* bias,
                                                                       unsigned long long* offers, int fresh, int* list,
                                                                       int* n_unassigned, int* stalled, float* two) {
  __shared__ int wave_tot[RC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int chunk = (N + RC_THREADS - 1) / RC_THREADS;
  const int beg = tid * chunk;
  int end = beg + chunk; end = end < N ? end : N;
  if (tid == 0) two[0] = 2.0f;                                            // the scale of the bids
  bool stall = false;
  for (int j = beg; j < end; ++j) {
    if (fresh) { offers[j] = 0ull; continue; }                            // a call's first launch: no offers yet
    const unsigned long long o = offers[j];
    if (o == 0ull) continue;
    offers[j] = 0ull;
    const int row = (int)~(unsigned)o;
    if ((unsigned)row >= (unsigned)N) continue;                           // (not an offer of top2_finalize)
    const float inc = __uint_as_float((unsigned)(o >> 32));
    // the previous owner is assigned, so it did not bid and wins nothing: no two threads write one `assigned` entry
    const int prev = owner[j];
    if (prev >= 0 && prev < N) assigned[prev] = -1;
    owner[j] = row;
    assigned[row] = j;
    const float b = bias[j], nb = b - inc;
    stall |= nb == b;
    bias[j] = nb;
  }
  if (stall) stalled[0] = 1;
  __syncthreads();                                                        // (global writes of this workgroup, visible to it)
  int cnt = 0;
  for (int i = beg; i < end; ++i) cnt += assigned[i] < 0;
  int incl = cnt;                                                         // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_tot[wid] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < RC_THREADS / 64; ++w) {
    const int t = wave_tot[w];
    base += w < wid ? t : 0;
    total += t;
  }
  int pos = base + incl - cnt;
  for (int i = beg; i < end; ++i)
    if (assigned[i] < 0) list[pos++] = i;
  if (tid == 0) n_unassigned[0] = total;
}

// TOP2_TPS tiles per split whatever the row count, longer splits only beyond TOP2_KSMAX of them (the partials are
// 12 bytes per row and split)
void plan(int Mr, int Ny, int* nqb, int* ksplit, int* tps, int* ntiles) {
  *nqb = (Mr + TQ - 1) / TQ;
  *ntiles = (Ny + TK - 1) / TK;
  *tps = TOP2_TPS;
  if ((*ntiles + *tps - 1) / *tps > TOP2_KSMAX) *tps = (*ntiles + TOP2_KSMAX - 1) / TOP2_KSMAX;
  *ksplit = (*ntiles + *tps - 1) / *tps;
}

size_t top2_ws_bytes(int Mr, int Ny) {
  int nqb, ks, tps, nt;
  plan(Mr, Ny, &nqb, &ks, &tps, &nt);
  return (size_t)ks * Mr * (2 * sizeof(float) + sizeof(int));
}

// the two launches of a top-two pass; workspace checked by the caller
int launch_top2(T2P p, void* workspace, int* idx, float* best, float* gap, const float* eps, unsigned long long* offers,
                hipStream_t stream) {
  int nqb, ks;
  plan(p.Mr, p.Ny, &nqb, &ks, &p.tiles_per_split, &p.ntiles);
  p.part_z1 = (float*)workspace;
  p.part_z2 = p.part_z1 + (size_t)ks * p.Mr;
  p.part_k = (int*)(p.part_z2 + (size_t)ks * p.Mr);
  hipLaunchKernelGGL(top2_kernel, dim3(nqb, ks), dim3(256), 0, stream, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(top2_finalize, dim3((p.Mr + 255) / 256), dim3(256), 0, stream, (const float*)p.part_z1,
                     (const int*)p.part_k, (const float*)p.part_z2, ks, p.Mr, p.Ny, p.n_active, idx, best, gap, p.rows, eps, offers);
  return clipk_check_launch();
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" int clipk_sim_top2_bias_plan(int Mr, int Ny, int* nqb, int* ksplit) {
  if (Mr <= 0 || Ny <= 0 || !nqb || !ksplit) return CLIPK_ERR_BAD_ARG;
  int tps, nt;
  plan(Mr, Ny, nqb, ksplit, &tps, &nt);
  return CLIPK_OK;
}

extern "C" size_t clipk_sim_top2_bias_workspace(int Mr, int Ny, int P) {
  if (!cloud_shape_ok(Mr, Ny, P, TOP2_PMAX)) return 0;
  return top2_ws_bytes(Mr, Ny);
}

extern "C" int clipk_sim_top2_bias(const float* X, int Mx, const int* rows, int Mr, const int* n_active, const float* Y,
                                   int Ny, int P, const float* scale, const float* bias, int* idx, float* best, float* gap,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (Mx <= 0 || Mr <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (!cloud_shape_ok(Mr, Ny, P, TOP2_PMAX)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !scale || !idx || !workspace) return CLIPK_ERR_BAD_ARG;
  if (!rows && Mr > Mx) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_top2_bias_workspace(Mr, Ny, P)) return CLIPK_ERR_BAD_ARG;
  T2P p{};
  p.X = X; p.Mx = Mx; p.rows = rows; p.Mr = Mr; p.n_active = n_active; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale;
  p.bias = bias;
  return launch_top2(p, workspace, idx, best, gap, nullptr, nullptr, (hipStream_t)stream);
}

// workspace: offers [N] u64 | list [N] i32 | the scale 2 (f32) | the top-two partials
extern "C" size_t clipk_auction_rounds_workspace(int N, int P) {
  if (!cloud_shape_ok(N, N, P, TOP2_PMAX) || N > AUCTION_NMAX) return 0;
  return round16((size_t)N * 8) + round16((size_t)N * 4) + 16 + top2_ws_bytes(N, N);
}

extern "C" int clipk_auction_rounds(const float* X, const float* Y, int N, int P, float* bias, const float* eps,
                                    int* assigned, int* owner, int* n_unassigned, int* stalled, int n_rounds,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (N <= 0 || P <= 0 || n_rounds < 0) return CLIPK_ERR_BAD_ARG;
  if (!cloud_shape_ok(N, N, P, TOP2_PMAX) || N > AUCTION_NMAX) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !Y || !bias || !eps || !assigned || !owner || !n_unassigned || !stalled || !workspace) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_auction_rounds_workspace(N, P)) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)workspace;
  unsigned long long* offers = (unsigned long long*)w; w += round16((size_t)N * 8);
  int* list = (int*)w; w += round16((size_t)N * 4);
  float* two = (float*)w; w += 16;
  T2P p{};
  p.X = X; p.Mx = N; p.rows = list; p.Mr = N; p.n_active = n_unassigned; p.Y = Y; p.Ny = N; p.P = P; p.scale = two;
  p.bias = bias;
  for (int r = 0; r <= n_rounds; ++r) {
    hipLaunchKernelGGL(auction_resolve_compact, dim3(1), dim3(RC_THREADS), 0, st, N, assigned, owner, bias, offers,
                       r == 0 ? 1 : 0, list, n_unassigned, stalled, two);
    int rc = clipk_check_launch();
    if (rc) return rc;
    if (r == n_rounds) break;
    rc = launch_top2(p, w, nullptr, nullptr, nullptr, eps, offers, st);
    if (rc) return rc;
  }
  return CLIPK_OK;
}
