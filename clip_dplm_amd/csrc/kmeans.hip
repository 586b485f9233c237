// kmeans.hip — one Lloyd iteration over an embedding cloud without the N x K score matrix leaving the workgroup
// (include/clipk.h: clipk_kmeans_step has the formulae, the tie rule and the supported range).
//
//   score_ic = 2 <x_i, c_c> - nc_c,  labels[i] = argmax_c score_ic (equal scores: the lower c),  best[i] = max_c score_ic
//   sums[c, :] = sum_{i: labels[i] = c} x_i,  counts[c] = #{i: labels[i] = c}
//
// The structure is kernel_sums_kernel<true> with the roles turned round: the centroids are the (at most 64) queries on
// the lanes, the points are the keys the walk runs over, and the weight tile is a one-hot: (1) the S^T tile by the
// K-loop over P; (2) the scores into the LDS tile gl[point][centroid], an arg max along each point's row, the row
// overwritten with its one-hot; (3) sums^T[p, c] += X^T[p, point] W[point, c] by the weighted key sum; the counts are
// the tile's column sums.  One launch reads each tile of X once for assignment and update.
// With the labels given there is no product: the one-hot tile comes from the labels, for any number of 64-centroid
// blocks.  Key-split slabs and count partials are summed in split order by split_sum_finalize.
// No float atomics, no cooperative launch: results depend on the shapes and inputs alone.
#include "common.h"
#include "cloud_keysum.h"
#include <math.h>

namespace {

constexpr int KM_PMAX = KEYSUM_PMAX;              // contraction / output width limit
constexpr int KM_KMAX_FUSED = TQ;                 // centroids of the fused mode: one query block
constexpr int KM_KMAX = 65536;                    // centroids with the labels given
constexpr int KM_NMAX = 1 << 24;                  // the counts are exact f32 integers

struct KMP {
  const float* X; int N;                          // points: the keys
  const float* C; int K;                          // centroids: the queries
  int P;
  const float* nc;                                // [K] squared norms of the centroids (zeros: cosine form)
  const int* labels_in;                           // [N] (labels-given mode)
  int* labels; float* best;                       // [N] (fused mode)
  float* slab;         // [ksplit][K][P]
  float* cnt_part;     // [ksplit][K]
  int tiles_per_split, ntiles;
};

constexpr int KM_CNT_FLOATS = 4 * TQ;                                     // the count merge slots of the four waves
template <bool FUSED>
constexpr int km_lds_floats() { return (FUSED ? KLOOP_LDS_FLOATS : 0) + KM_CNT_FLOATS + KEYSUM_LDS_FLOATS; }

// FUSED = false: the labels are given - no S product and no K-loop buffers
template <bool FUSED>
__global__ __launch_bounds__(256, 2) void kmeans_step_kernel(const KMP p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);                       // K-loop buffers (FUSED)
  float* cl = smem + (FUSED ? KLOOP_LDS_FLOATS : 0);                      // [4 waves][64 centroids]: count partials
  float* gl = cl + KM_CNT_FLOATS;                                         // score / one-hot tile [64 points][64 centroids]
  float* yh = gl + TK * TQ;                                               // point block [16][YH_LD] / output transposes
  const KeyWalk<BKG> w(p.C, p.K, nullptr, p.K, p.X, p.N, p.P, p.tiles_per_split, p.ntiles, smem);
  const int wm = w.wm, wn = w.wn, li = w.li, h = w.h, ks = w.ks, qg = w.qg;
  const int tid = w.tid, N = p.N, K = p.K;
  const int row = tid >> 2, part = tid & 3;                               // arg max: four threads per point row
  float* g = gl + row * TQ + part * 16;                                   // this thread's 16 centroids of its row
  float nc_q = 0.f;
  if constexpr (FUSED) nc_q = p.nc[qg < K ? qg : K - 1];
  f32x16 dx[4][2];
  key_sum_zero(dx);
  float cnt = 0.f;

  for (int kt = w.t_beg; kt < w.t_end; ++kt) {
    const int j0 = kt * TK;
    const int point = j0 + row;
    int arg;                                                              // this row's centroid within the block, -1: none
    if constexpr (FUSED) {
      f32x16 acc;
      w.product(j0, acc);                                                 // (its first barrier also frees gl / yh)
      // ---- scores (accumulator layout: rows = points, lanes = centroids) -> LDS tile gl[point][centroid]
#pragma unroll
      for (int r = 0; r < 16; ++r)
        gl[(wm * 32 + keyrow32(r, h)) * TQ + wn * 32 + li] = qg < K ? fmaf(2.f, acc[r], -nc_q) : -INFINITY;
      __syncthreads();
      // ---- arg max along the row: 16 centroids per thread in rising order, then the four threads of the row
      float bv = -INFINITY;
      int bq = part * 16;
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v[e] > bv) { bv = v[e]; bq = part * 16 + 4 * i4 + e; }      // strictly greater: a tie keeps the lower index
      }
#pragma unroll
      for (int m = 1; m < 4; m <<= 1) {
        const float ov = __shfl_xor(bv, m, 64);
        const int oq = __shfl_xor(bq, m, 64);
        if (ov > bv || (ov == bv && oq < bq)) { bv = ov; bq = oq; }
      }
      if (part == 0 && point < N) { p.labels[point] = bq; p.best[point] = bv; }
      arg = point < N ? bq : -1;                                          // points beyond N: all zeros
    } else {
      arg = point < N ? p.labels_in[point] - w.q0 : -1;                   // outside this block: matches no column
      __syncthreads();                                                    // the last tile's readers of gl are done
    }
    // ---- the row becomes its one-hot (each thread overwrites the 16 entries it alone has read)
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (arg == part * 16 + 4 * i4 + e) ? 1.f : 0.f;
      *reinterpret_cast<f32x4*>(g + 4 * i4) = o;
    }
    key_sum_tile(dx, p.X, N, p.P, j0, gl, yh, tid, w.wid, li, h);         // sums^T += X^T W
    // ---- counts: the tile's column sums, 16 point rows per wave (gl stays as it is until the next tile's first barrier)
#pragma unroll
    for (int i = 0; i < 16; ++i) cnt += gl[(w.wid * 16 + i) * TQ + (tid & 63)];
  }

  __syncthreads();
  key_sum_store(dx, yh, p.slab, K, p.P, w.q0, ks, w.wid, li, h);
  cl[tid] = cnt;                                                          // [wave][centroid]
  __syncthreads();
  if (tid < TQ && w.q0 + tid < K)
    p.cnt_part[(long)ks * K + w.q0 + tid] = (cl[tid] + cl[TQ + tid]) + (cl[2 * TQ + tid] + cl[3 * TQ + tid]);
}

bool shape_ok(int N, int K, int P, bool fused) {
  return N > 0 && N <= KM_NMAX && K > 0 && K <= (fused ? KM_KMAX_FUSED : KM_KMAX) && P > 0 && !(P & 3) && P <= KM_PMAX;
}

template <bool FUSED>
void launch_step(const KMP& p, dim3 grid, hipStream_t stream) {
  const size_t lds = (size_t)km_lds_floats<FUSED>() * sizeof(float);
  static std::atomic<uint64_t> attr_set{0};
  clipk_once_per_device(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_step_kernel<FUSED>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  hipLaunchKernelGGL(kmeans_step_kernel<FUSED>, grid, dim3(256), lds, stream, p);
}

}  // namespace

extern "C" size_t clipk_kmeans_step_workspace(int N, int K, int P) {
  if (!shape_ok(N, K, P, false)) return 0;
  const size_t ks = key_split_plan(K, N, TQ).ksplit;
  return ks * K * ((size_t)P + 1) * sizeof(float);                        // sum slabs, then the count partials
}

extern "C" int clipk_kmeans_step(const float* X, int N, const float* Cn, int K, int P, const float* nc,
                                 const int* labels_in, int* labels, float* best, float* sums, float* counts,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const bool fused = labels_in == nullptr;
  if (N <= 0 || K <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (!shape_ok(N, K, P, fused)) return CLIPK_ERR_UNSUPPORTED;
  if (!X || !sums || !counts || !workspace) return CLIPK_ERR_BAD_ARG;
  if (fused && (!Cn || !nc || !labels || !best)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(sums) || !aligned16(workspace) || (fused && !aligned16(Cn))) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_kmeans_step_workspace(N, K, P)) return CLIPK_ERR_BAD_ARG;
  const KeySplitPlan k = key_split_plan(K, N, TQ);                        // centroid blocks x point splits
  const int ks = k.ksplit;
  KMP p{};
  p.X = X; p.N = N; p.C = fused ? Cn : X; p.K = K; p.P = P; p.nc = nc; p.labels_in = labels_in;
  p.labels = labels; p.best = best;
  p.tiles_per_split = k.tiles_per_split; p.ntiles = k.ntiles;
  float* ws = (float*)workspace;
  p.slab = ws;
  p.cnt_part = ws + (size_t)ks * K * P;                                   // (a multiple of 4 floats: the partials stay aligned)
  if (fused) launch_step<true>(p, dim3(k.nqb, ks), (hipStream_t)stream);
  else launch_step<false>(p, dim3(k.nqb, ks), (hipStream_t)stream);
  int rc = clipk_check_launch();
  if (rc) return rc;
  launch_split_sum_finalize(p.slab, p.cnt_part, nullptr, ks, K, P, sums, counts, nullptr, (hipStream_t)stream);
  return clipk_check_launch();
}
