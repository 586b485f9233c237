// retrieval.hip — cross-modal retrieval over an embedding gallery without materialising the logits:
//   clipk_sim_topk : the k best keys of every query,  S[i,j] = scale <X_i, Y_j>
//   clipk_sim_rank : the 0-based rank of every query's labelled positive, and its score
//   clipk_sim_knn  : clipk_sim_topk with a key-side bias, one skipped key per row and a resume cursor (the KNN
//                    instantiation of sim_topk_kernel; every addition sits under `if constexpr`)
// All walk the tiled exact-f32 similarity block of the fused softmax statistics (sim_tile.h: 64 queries per workgroup,
// 64-key tiles, keys on the MFMA rows, queries on the lanes, key-range splits on grid y) and replace its epilogue.
//
// Ordering contract: score descending, equal scores (IEEE: -0 == +0) by the lower key index.  It is a total order, so the
// top-k set, its order and every rank are bitwise independent of the split plan.
//
// Top-k: lane (li, h) of key-wave wm owns 16 of every 64-key tile for its query and meets its keys in ascending index
// order; it keeps the best KP (k rounded up to 1 / 8 / 16 / 32 / 64) in registers, sorted.  Per tile the common case is
// one max over the 16 scores and one compare with the list's last entry; only a lane whose tile holds a better score
// takes the insertion path.  Each of the four owners of a query writes its list to the workspace and topk_merge_kernel
// reduces the 4 x ksplit lists per query in a fixed tree (16 lists per workgroup, rank of every candidate by binary search
// in the other sorted lists).
//
// Rank: one extra tile per workgroup computes S[i, l_i] from a gathered tile whose key rows are the labels' rows, with
// the same K-loop and the same query rows, so it has the bits the counting loop sees at that key; every score then costs
// one compare pair against it.  Per-split counts are summed by sim_rank_finalize.  The class-filtered rank (CLS = true)
// loads the gallery ids of a lane's 16 key rows once per tile, before its K-loop, and counts only keys of other classes;
// CLS = false is the plain kernel (the filter sits under `if constexpr`).
#include "common.h"
#include "sim_tile.h"
#include "plane_tile.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int RQ = 64, RK = 64;          // queries per workgroup, keys per tile
constexpr int RBK = 32;                  // K-step of the tile loop (as the LSE pass: 16 MFMAs per wave between barriers)
constexpr int MG = 16;                   // lists merged by one workgroup of the finalize tree
constexpr int EMPTY = INT_MAX;           // key index of an unfilled list slot (its score is -inf)

__device__ __forceinline__ int key_off(int r) { return (r & 3) + 8 * (r >> 2); }   // keyrow32(r, h) - 4 h

// stage rows of the workgroup's 64 queries (clamped: rows past Mx are computed and dropped)
__device__ __forceinline__ void query_rows(const float* (&xrows)[RBK / 16], const float* X, int Mx, int P, int q0, int tid) {
#pragma unroll
  for (int i = 0; i < RBK / 16; ++i) {
    int q = q0 + (tid + i * 256) / (RBK / 4); q = q < Mx ? q : Mx - 1;
    xrows[i] = X + (long)q * P;
  }
}
__device__ __forceinline__ void key_rows(const float* (&yrows)[RBK / 16], const float* Y, int Ny, int P, int j0, int tid) {
#pragma unroll
  for (int i = 0; i < RBK / 16; ++i) {
    int j = j0 + (tid + i * 256) / (RBK / 4); j = j < Ny ? j : Ny - 1;
    yrows[i] = Y + (long)j * P;
  }
}

// sorted insert of (v, j), v > s[KP - 1]; j is larger than every index in the list, so v goes after its equals
template <int KP>
__device__ __forceinline__ void list_insert(float (&s)[KP], int (&ix)[KP], float v, int j) {
#pragma unroll
  for (int t = KP - 1; t > 0; --t) {
    if (s[t - 1] < v) { s[t] = s[t - 1]; ix[t] = ix[t - 1]; }
    else if (s[t] < v) { s[t] = v; ix[t] = j; }
  }
  if (s[0] < v) { s[0] = v; ix[0] = j; }
}

struct TKP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P; float scale;
  float* part_s; int* part_i;            // [4 ksplit][Mx][KP]
  int tiles_per_split, ntiles;
  // KNN instantiation only
  const float* bias;                     // [Ny] or null
  long long diag_offset;                 // row i skips key i + diag_offset; -1: no key skipped
  const float* after_s; const int64_t* after_i;   // [Mx] cursor in the total order, or null
};

// KNN: z = fl(fl(scale s) + bias[key]) replaces the score and a key that is the row's own (key == q + diag_offset), at or
// before the cursor (after_s, after_i)[q] in the total order, or past Ny counts as -inf: it then fails the tile-maximum
// test and the insertion test like any weak key, so the common path stays one max and one compare per tile.
template <int KP, bool KNN>
__global__ __launch_bounds__(256, 2) void sim_topk_kernel(const TKP p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (RBK + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * RQ, ks = blockIdx.y;
  const int P = p.P, Ny = p.Ny;
  const float scale = p.scale;
  const float* xrows[RBK / 16];
  query_rows(xrows, p.X, p.Mx, P, q0, tid);
  float s[KP];
  int ix[KP];
#pragma unroll
  for (int t = 0; t < KP; ++t) { s[t] = -INFINITY; ix[t] = EMPTY; }
  const int t_beg = ks * p.tiles_per_split;
  int t_end = t_beg + p.tiles_per_split; t_end = t_end < p.ntiles ? t_end : p.ntiles;
  float cur_s = INFINITY;                                                 // KNN: the cursor and the skipped key of this
  int cur_i = -1, skip = -1;                                              // lane's query (no cursor: every z < +inf)
  // KNN: bias[j0 .. j0 + 64) of the tile goes through LDS, loaded one tile ahead by threads 0..63 so that the load is
  // in flight under the K-loop at the price of one register.  Double-buffered: a buffer is rewritten two tiles after it
  // was read, and s_tile's unconditional barriers lie between (and between a tile's write and its read).
  __shared__ __attribute__((aligned(16))) float bl[KNN ? 2 : 1][KNN ? RK : 4];
  const bool biased = KNN && p.bias != nullptr;
  float bnext = 0.f;
  if constexpr (KNN) {
    if (biased && tid < RK) { const int key = t_beg * RK + tid; bnext = p.bias[key < Ny ? key : Ny - 1]; }
    const int q = q0 + wn * 32 + li, qc = q < p.Mx ? q : p.Mx - 1;
    if (p.after_s) cur_s = p.after_s[qc];
    if (p.after_i) { const int64_t a = p.after_i[qc]; cur_i = a < 0 ? -1 : a > INT_MAX ? INT_MAX : (int)a; }
    const long long d = p.diag_offset < 0 ? -1 : (long long)q + p.diag_offset;
    skip = d < Ny ? (int)d : -1;
  }

  for (int kt = t_beg; kt < t_end; ++kt) {
    const int j0 = kt * RK;
    const float* yrows[RBK / 16];
    key_rows(yrows, p.Y, Ny, P, j0, tid);
    const int kb = j0 + wm * 32 + 4 * h;                                  // key of accumulator row r: kb + key_off(r)
    if constexpr (KNN) {                                                  // this tile's biases to LDS, the next tile's in flight
      if (biased && tid < RK) {
        bl[kt & 1][tid] = bnext;
        const int key = j0 + RK + tid;
        bnext = p.bias[key < Ny ? key : Ny - 1];
      }
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<RBK>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
    float tmax = -INFINITY;
    if constexpr (KNN) {                                                  // acc <- z, or -inf where not eligible
      f32x4 bz[4];                                                        // bias of row r: bz[r >> 2][r & 3]
      if (biased) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bz[g] = *reinterpret_cast<const f32x4*>(&bl[kt & 1][wm * 32 + 4 * h + 8 * g]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + key_off(r);
        float z = __fmul_rn(scale, acc[r]);
        if (biased) z = __fadd_rn(z, bz[r >> 2][r & 3]);
        const bool ok = (key < Ny) & (key != skip) & ((z < cur_s) | ((z == cur_s) & (key > cur_i)));
        acc[r] = ok ? z : -INFINITY;
        tmax = fmaxf(tmax, acc[r]);
      }
    } else if (j0 + RK <= Ny) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, scale * acc[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) if (kb + key_off(r) < Ny) tmax = fmaxf(tmax, scale * acc[r]);
    }
    if (tmax > s[KP - 1]) {                                               // rare once the list is full
      unsigned m = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kb + key_off(r) < Ny && (KNN ? acc[r] : scale * acc[r]) > s[KP - 1]) m |= 1u << r;
      while (m) {                                                         // ascending r = ascending key
        const int r = __builtin_ctz(m);
        m &= m - 1;
        float a = acc[0];
#pragma unroll
        for (int rr = 1; rr < 16; ++rr) a = (r == rr) ? acc[rr] : a;     // no dynamic register indexing
        const float v = KNN ? a : scale * a;
        if (v > s[KP - 1]) list_insert<KP>(s, ix, v, kb + key_off(r));
      }
    }
  }

  const int qg = q0 + wn * 32 + li;
  if (qg < p.Mx) {
    const long o = ((long)(ks * 4 + wm * 2 + h) * p.Mx + qg) * KP;
#pragma unroll
    for (int t = 0; t < KP; ++t) { p.part_s[o + t] = s[t]; p.part_i[o + t] = ix[t]; }
  }
}

// One round of the finalize tree: workgroup (q, g) merges lists [g MG, g MG + MG) of query q (each sorted, KP entries)
// into list g of `out_*`, or - last round, one group - into the k results.  The rank of a candidate is the number of
// candidates that precede it in the order, summed over the lists by binary search; real keys are distinct, so the
// ranks of real candidates are exactly 0 .. R - 1.
template <int KP>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* in_s, const int* in_i, int L, int Mx,
                                                         float* out_s, int* out_i, float* fin_s, int64_t* fin_i,
                                                         int k, int Ny) {
  __shared__ float ss[MG * KP];
  __shared__ int si[MG * KP];
  __shared__ int nreal;
  const int tid = threadIdx.x, q = blockIdx.x, g = blockIdx.y;
  const int l0 = g * MG, nl = (L - l0) < MG ? (L - l0) : MG, n = nl * KP;
  if (tid == 0) nreal = 0;
  for (int e = tid; e < n; e += 256) {
    const long o = ((long)(l0 + e / KP) * Mx + q) * KP + e % KP;
    ss[e] = in_s[o]; si[e] = in_i[o];
  }
  __syncthreads();
  int mine = 0;
  for (int e = tid; e < n; e += 256) mine += si[e] != EMPTY;
  if (mine) atomicAdd(&nreal, mine);
  __syncthreads();
  const int R = nreal, kout = fin_s ? k : KP;
  for (int e = tid; e < n; e += 256) {
    const int j = si[e];
    if (j == EMPTY) continue;
    const float v = ss[e];
    int rank = 0;
    for (int l = 0; l < nl; ++l) {
      int lo = 0, hi = KP;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float w = ss[l * KP + mid];
        if (w > v || (w == v && si[l * KP + mid] < j)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < kout) {
      if (fin_s) { fin_s[(long)q * k + rank] = v; fin_i[(long)q * k + rank] = j; }
      else { const long o = ((long)g * Mx + q) * KP + rank; out_s[o] = v; out_i[o] = j; }
    }
  }
  for (int t = R + tid; t < kout; t += 256) {                             // fewer than k real keys: NaN inputs, or
                                                                          // clipk_sim_knn (Ny = 0 here: index -1)
    if (fin_s) { fin_s[(long)q * k + t] = -INFINITY; fin_i[(long)q * k + t] = t < Ny ? t : Ny - 1; }
    else { const long o = ((long)g * Mx + q) * KP + t; out_s[o] = -INFINITY; out_i[o] = EMPTY; }
  }
}

struct RKP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P; float scale;
  const int64_t* labels; int64_t label_offset;
  int* part_cnt;                         // [ksplit][Mx]
  float* pos;                            // [Mx]
  int tiles_per_split, ntiles;
  const int64_t* cls;                    // [Ny] gallery class ids (CLS instantiation only)
};

__device__ __forceinline__ int label_of(const int64_t* labels, int64_t label_offset, int q, int Ny) {
  const int64_t l = labels ? labels[q] : label_offset + q;
  return (l >= 0 && l < Ny) ? (int)l : -1;                                // -1: out of range, reported as rank -1
}

template <bool CLS>
__global__ __launch_bounds__(256, 2) void sim_rank_kernel(const RKP p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (RBK + 4)];
  __shared__ int labl[RQ];
  __shared__ float posl[RQ];
  __shared__ int cntl[RQ];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * RQ, ks = blockIdx.y;
  const int P = p.P, Ny = p.Ny;
  const float scale = p.scale;
  const float* xrows[RBK / 16];
  query_rows(xrows, p.X, p.Mx, P, q0, tid);
  if (tid < RQ) {
    const int q = q0 + tid;
    labl[tid] = label_of(p.labels, p.label_offset, q < p.Mx ? q : p.Mx - 1, Ny);
  }
  __syncthreads();

  // ---- S[q, l_q]: the gathered tile whose key row kl is the label row of query q0 + kl; its diagonal lies in the
  // waves with wm == wn, key row li of lane (li, h = (li >> 2) & 1) at accumulator row (li & 3) + 4 (li >> 3)
  {
    const float* yrows[RBK / 16];
#pragma unroll
    for (int i = 0; i < RBK / 16; ++i) {
      const int l = labl[(tid + i * 256) / (RBK / 4)];
      yrows[i] = p.Y + (long)(l < 0 ? 0 : l) * P;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<RBK>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
    if (wm == wn) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (keyrow32(r, h) == li) posl[wn * 32 + li] = scale * acc[r];
    }
    __syncthreads();
  }
  const float pv = posl[wn * 32 + li];
  const int lab = labl[wn * 32 + li];
  int64_t lcl = 0;                                                        // CLS: the positive's class
  if constexpr (CLS) lcl = p.cls[lab < 0 ? 0 : lab];
  int cnt = 0;
  const int t_beg = ks * p.tiles_per_split;
  int t_end = t_beg + p.tiles_per_split; t_end = t_end < p.ntiles ? t_end : p.ntiles;

  for (int kt = t_beg; kt < t_end; ++kt) {
    const int j0 = kt * RK;
    const float* yrows[RBK / 16];
    key_rows(yrows, p.Y, Ny, P, j0, tid);
    const int kb = j0 + wm * 32 + 4 * h;
    bool other[16];                                                       // CLS: key of another class than the positive
    if constexpr (CLS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + key_off(r);
        other[r] = key < Ny && p.cls[key] != lcl;
      }
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<RBK>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
    if constexpr (CLS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sv = scale * acc[r];
        cnt += other[r] & ((sv > pv) | ((sv == pv) & (kb + key_off(r) < lab)));
      }
    } else if (j0 + RK <= Ny) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sv = scale * acc[r];
        cnt += (sv > pv) | ((sv == pv) & (kb + key_off(r) < lab));
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sv = scale * acc[r];
        const int key = kb + key_off(r);
        cnt += (key < Ny) & ((sv > pv) | ((sv == pv) & (key < lab)));
      }
    }
  }

  // ---- the four owners of a query: lane halves, then the two key-waves
  cnt += __shfl_xor(cnt, 32, 64);
  if (wm == 1 && h == 0) cntl[wn * 32 + li] = cnt;
  __syncthreads();
  const int qg = q0 + wn * 32 + li;
  if (wm == 0 && h == 0 && qg < p.Mx) {
    p.part_cnt[(long)ks * p.Mx + qg] = cnt + cntl[wn * 32 + li];
    if (ks == 0) p.pos[qg] = lab >= 0 ? pv : __builtin_nanf("");
  }
}

__global__ void sim_rank_finalize(const int* part_cnt, int ksplit, int Mx, const int64_t* labels, int64_t label_offset,
                                  int Ny, int64_t* rank) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Mx) return;
  int64_t r = 0;
  for (int s = 0; s < ksplit; ++s) r += part_cnt[(long)s * Mx + q];
  rank[q] = label_of(labels, label_offset, q, Ny) >= 0 ? r : -1;
}

// plan: one workgroup per (query block of qb, key split), >= 2 workgroups per CU (the LSE pass's plan); the option
// retrieval_splits (> 0) fixes the split count instead
void plan(int Mx, int Ny, int qb, int* nqb, int* ksplit, int* tps, int* ntiles) {
  *nqb = (Mx + qb - 1) / qb;
  *ntiles = (Ny + RK - 1) / RK;
  const int opt = clipk_opt_get(OPT_RETRIEVAL_SPLITS);
  int ks = opt > 0 ? opt : (512 + *nqb - 1) / *nqb;
  if (ks > 65535) ks = 65535;
  if (ks > *ntiles) ks = *ntiles;
  if (ks < 1) ks = 1;
  *tps = (*ntiles + ks - 1) / ks;
  *ksplit = (*ntiles + *tps - 1) / *tps;
}

int kpad(int k) { return k <= 1 ? 1 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

// clipk_sim_knn leaves the 32-slot instance out: beyond 16 results the 64-slot one is the faster at every large shape
// measured (clipk_sim_topk shows the same inversion and keeps its instances)
int kpad_knn(int k) { return k <= 16 ? kpad(k) : 64; }

bool shape_ok(int Mx, int Ny, int P) { return Mx > 0 && Ny > 0 && P > 0 && Ny <= INT_MAX - RK; }

// KNN: p carries bias / diag_offset / after_*, and the unfilled result slots get index -1 (fill_Ny = 0)
template <int KP, bool KNN = false>
int topk_launch(const float* X, int Mx, const float* Y, int Ny, int P, float scale, int k, float* scores, int64_t* idx,
                char* ws, hipStream_t st, TKP p = TKP{}) {
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale;
  const int fill_Ny = KNN ? 0 : Ny;
  int nqb, ksplit;
  plan(Mx, Ny, RQ, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  const int la = 4 * ksplit, lb = (la + MG - 1) / MG;
  const size_t per_list = (size_t)Mx * KP;
  float* a_s = reinterpret_cast<float*>(ws);
  int* a_i = reinterpret_cast<int*>(a_s + la * per_list);
  float* b_s = reinterpret_cast<float*>(a_i + la * per_list);
  int* b_i = reinterpret_cast<int*>(b_s + lb * per_list);
  p.part_s = a_s; p.part_i = a_i;
  hipLaunchKernelGGL((sim_topk_kernel<KP, KNN>), dim3(nqb, ksplit), dim3(256), 0, st, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  const float* src_s = a_s; const int* src_i = a_i;
  float* dst_s = b_s; int* dst_i = b_i;
  for (int L = la;;) {
    const int groups = (L + MG - 1) / MG;
    if (groups == 1) {
      hipLaunchKernelGGL(topk_merge_kernel<KP>, dim3(Mx, 1), dim3(256), 0, st, src_s, src_i, L, Mx,
                         (float*)nullptr, (int*)nullptr, scores, idx, k, fill_Ny);
      return clipk_check_launch();
    }
    hipLaunchKernelGGL(topk_merge_kernel<KP>, dim3(Mx, groups), dim3(256), 0, st, src_s, src_i, L, Mx, dst_s, dst_i,
                       (float*)nullptr, (int64_t*)nullptr, k, fill_Ny);
    if ((rc = clipk_check_launch())) return rc;
    L = groups;
    float* ts = const_cast<float*>(src_s); int* ti = const_cast<int*>(src_i);  // ping-pong: A holds >= every later L
    src_s = dst_s; src_i = dst_i; dst_s = ts; dst_i = ti;
  }
}

}  // namespace

extern "C" size_t clipk_sim_topk_workspace(int Mx, int Ny, int P, int k) {
  if (!shape_ok(Mx, Ny, P) || k < 1 || k > 64 || k > Ny) return 0;
  int nqb, ksplit, tps, nt;
  plan(Mx, Ny, RQ, &nqb, &ksplit, &tps, &nt);
  const size_t la = 4 * (size_t)ksplit, lb = (la + MG - 1) / MG;
  return (la + lb) * (size_t)Mx * kpad(k) * (sizeof(float) + sizeof(int));
}

extern "C" int clipk_sim_topk(const float* X, int Mx, const float* Y, int Ny, int P, float scale, int k, float* scores,
                              int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !Y || !scores || !idx || !workspace) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0 || k <= 0 || k > Ny) return CLIPK_ERR_BAD_ARG;
  if (k > 64 || P % 4 || !shape_ok(Mx, Ny, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(Y)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_topk_workspace(Mx, Ny, P, k)) return CLIPK_ERR_BAD_ARG;
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  switch (kpad(k)) {
    case 1: return topk_launch<1>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st);
    case 8: return topk_launch<8>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st);
    case 16: return topk_launch<16>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st);
    case 32: return topk_launch<32>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st);
    default: return topk_launch<64>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st);
  }
}

extern "C" size_t clipk_sim_knn_workspace(int Mx, int Ny, int P, int k) {
  if (!shape_ok(Mx, Ny, P) || P % 4 || k < 1 || k > 64) return 0;
  int nqb, ksplit, tps, nt;
  plan(Mx, Ny, RQ, &nqb, &ksplit, &tps, &nt);
  const size_t la = 4 * (size_t)ksplit, lb = (la + MG - 1) / MG;
  return (la + lb) * (size_t)Mx * kpad_knn(k) * (sizeof(float) + sizeof(int));
}

extern "C" int clipk_sim_knn(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const float* bias,
                             long long diag_offset, const float* after_s, const int64_t* after_i, int k, float* scores,
                             int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !Y || !scores || !idx || !workspace) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0 || k <= 0 || diag_offset < -1) return CLIPK_ERR_BAD_ARG;
  if ((after_s == nullptr) != (after_i == nullptr)) return CLIPK_ERR_BAD_ARG;
  if (k > 64 || P % 4 || !shape_ok(Mx, Ny, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(Y)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_knn_workspace(Mx, Ny, P, k)) return CLIPK_ERR_BAD_ARG;
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  TKP p{};
  p.bias = bias; p.diag_offset = diag_offset; p.after_s = after_s; p.after_i = after_i;
  switch (kpad_knn(k)) {
    case 1: return topk_launch<1, true>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st, p);
    case 8: return topk_launch<8, true>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st, p);
    case 16: return topk_launch<16, true>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st, p);
    default: return topk_launch<64, true>(X, Mx, Y, Ny, P, scale, k, scores, idx, ws, st, p);
  }
}

extern "C" size_t clipk_sim_rank_workspace(int Mx, int Ny, int P) {
  if (!shape_ok(Mx, Ny, P)) return 0;
  int nqb, ksplit, tps, nt;
  plan(Mx, Ny, RQ, &nqb, &ksplit, &tps, &nt);
  return (size_t)ksplit * Mx * sizeof(int);
}

extern "C" int clipk_sim_rank(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const int64_t* labels,
                              int64_t label_offset, int64_t* rank, float* pos, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (!X || !Y || !rank || !pos || !workspace) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (P % 4 || !shape_ok(Mx, Ny, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!labels && (label_offset < 0 || label_offset + Mx > Ny)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_rank_workspace(Mx, Ny, P)) return CLIPK_ERR_BAD_ARG;
  RKP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale; p.labels = labels; p.label_offset = label_offset;
  p.part_cnt = static_cast<int*>(workspace); p.pos = pos;
  int nqb, ksplit;
  plan(Mx, Ny, RQ, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sim_rank_kernel<false>, dim3(nqb, ksplit), dim3(256), 0, st, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(sim_rank_finalize, dim3((Mx + 255) / 256), dim3(256), 0, st, (const int*)p.part_cnt, ksplit, Mx,
                     labels, label_offset, Ny, rank);
  return clipk_check_launch();
}

extern "C" int clipk_sim_rank_cls(const float* X, int Mx, const float* Y, int Ny, int P, float scale,
                                  const int64_t* labels, int64_t label_offset, const int64_t* cls, int64_t* rank,
                                  float* pos, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !Y || !cls || !rank || !pos || !workspace) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (P % 4 || !shape_ok(Mx, Ny, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!labels && (label_offset < 0 || label_offset + Mx > Ny)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_rank_workspace(Mx, Ny, P)) return CLIPK_ERR_BAD_ARG;
  RKP p;
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale; p.labels = labels; p.label_offset = label_offset;
  p.part_cnt = static_cast<int*>(workspace); p.pos = pos; p.cls = cls;
  int nqb, ksplit;
  plan(Mx, Ny, RQ, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sim_rank_kernel<true>, dim3(nqb, ksplit), dim3(256), 0, st, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(sim_rank_finalize, dim3((Mx + 255) / 256), dim3(256), 0, st, (const int*)p.part_cnt, ksplit, Mx,
                     labels, label_offset, Ny, rank);
  return clipk_check_launch();
}

// ================================================================================================================
// Prefiltered exact top-k: a bf16 candidate pass, an exact re-rank of the candidates and a per-query certificate
// (include/clipk.h: clipk_split_bf16, clipk_sim_topk_cand, clipk_sim_rerank; the bound is derived there).
//
// Candidate pass tile (sim_cand_kernel): plane_tile.h's PlaneWalk, shared with sinkhorn.hip's bf16x3 LSE pass - 128
// queries x 64 keys per workgroup, 4 waves; wave w owns queries [32 w, +32) against all 64 keys, i.e. two 32x32
// accumulators of v_mfma_f32_32x32x16_bf16 sharing one query fragment.  128 queries per workgroup halve the gallery
// re-reads of the exact kernel's 64 (shape a: 64 instead of 128 passes over the bf16 gallery, most of them L2 / MALL hits
// because the query blocks of one key split run side by side).
// A lane keeps ONE list (its query), fed by 32 keys per tile in ascending index order (accumulator 0 then 1, rows
// ascending), so the sorted-list epilogue and topk_merge_kernel are reused unchanged, with 2 lists per key split.
// bf16 planes have a row pitch of P rounded up to 32 with zero pads (clipk_split_bf16 writes them): the K loop has no
// tail and every staging load is 16 bytes.  X3 (bf16x3): three MFMAs per fragment pair into the same accumulator
// (hi.hi, hi.lo, lo.hi).
// Re-rank (sim_rerank_kernel): one workgroup per query; s_tile over a gathered tile whose 64 key rows are the query's
// candidates and whose 64 query columns are all the query itself.  Each MFMA output element depends only on its row
// and column operands and its accumulator, in the same K order as sim_topk_kernel, so the scores have its bits.
// ================================================================================================================
namespace {

static_assert(PLK == RK, "plan() counts tiles of RK keys");
constexpr int PF_MAX_P = 65536;           // prefilter entries: the norm and bound arithmetic assumes P <= 2^16

int plane_pitch(int P) { return (P + 31) & ~31; }

// rows of X -> bf16 hi (and lo = bf16(x - hi)) planes with zero pads; the row norm, computed in f64 and rounded up to
// f32, raises the running maximum *norm_max (non-negative floats order as their bit patterns); NaN / overflow -> +inf
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* X, int n, int P, int PP, unsigned short* hi,
                                                         unsigned short* lo, float* norm_max) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + w;
  if (row >= n) return;                                                   // per wave; no barriers below
  const float* x = X + (long)row * P;
  unsigned short* hr = hi + (long)row * PP;
  unsigned short* lr = lo ? lo + (long)row * PP : nullptr;
  double ss = 0.0;
  for (int c = 4 * lane; c < PP; c += 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < P) v = *reinterpret_cast<const f32x4*>(x + c);
    u32x2 hv;
    hv[0] = pack_bf16x2(v[0], v[1]); hv[1] = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(hr + c) = hv;
    if (lr) {                                                             // x - hi is exact in f32
      u32x2 lv;
      lv[0] = pack_bf16x2(v[0] - __uint_as_float(hv[0] << 16), v[1] - __uint_as_float(hv[0] & 0xffff0000u));
      lv[1] = pack_bf16x2(v[2] - __uint_as_float(hv[1] << 16), v[3] - __uint_as_float(hv[1] & 0xffff0000u));
      *reinterpret_cast<u32x2*>(lr + c) = lv;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += (double)v[e] * (double)v[e];       // exact squares, P <= 2^16 terms
  }
  if (!norm_max) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) {
    const double nd = sqrt(ss) * (1.0 + 0x1p-30);                         // covers the f64 sum and sqrt roundings
    float nf = INFINITY;
    if (nd <= 3.0e38) {
      nf = (float)nd;
      if ((double)nf < nd) nf = __uint_as_float(__float_as_uint(nf) + 1u);   // round up
    }
    atomicMax(reinterpret_cast<unsigned int*>(norm_max), __float_as_uint(nf));
  }
}

struct CKPm {
  const unsigned short* xh; const unsigned short* xl; int Mx;
  const unsigned short* yh; const unsigned short* yl; int Ny;
  int PP; float scale;
  float* part_s; int* part_i;            // [2 ksplit][Mx][KP]
  int tiles_per_split, ntiles;
};

template <int KP, bool X3>
__global__ __launch_bounds__(256, 2) void sim_cand_kernel(const CKPm p) {
  using Walk = PlaneWalk<X3 ? 2 : 1>;
  __shared__ __attribute__((aligned(16))) unsigned short sm[Walk::LDS_ELEMS];
  const float scale = p.scale;
  const Walk wk(p.xh, p.xl, p.Mx, p.yh, p.yl, p.Ny, p.PP, p.tiles_per_split, p.ntiles, sm);
  const int h = wk.h, ks = wk.ks, qg = wk.qg, Ny = p.Ny;
  float s[KP];
  int ix[KP];
#pragma unroll
  for (int t = 0; t < KP; ++t) { s[t] = -INFINITY; ix[t] = EMPTY; }

  for (int kt = wk.t_beg; kt < wk.t_end; ++kt) {
    const int j0 = kt * PLK;
    f32x16 acc[2];
    wk.product(j0, acc);
    const int kb0 = j0 + 4 * h;                                           // key of acc[kb][r]: kb0 + 32 kb + key_off(r)
    float tmax = -INFINITY;
    if (j0 + PLK <= Ny) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, fmaxf(scale * acc[0][r], scale * acc[1][r]));
    } else {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) if (kb0 + 32 * kb + key_off(r) < Ny) tmax = fmaxf(tmax, scale * acc[kb][r]);
    }
    if (tmax > s[KP - 1]) {                                               // rare once the list is full
      unsigned m = 0;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kb0 + 32 * kb + key_off(r) < Ny && scale * acc[kb][r] > s[KP - 1]) m |= 1u << (kb * 16 + r);
      while (m) {                                                         // ascending bit = ascending key
        const int bi = __builtin_ctz(m);
        m &= m - 1;
        float a = acc[0][0];
#pragma unroll
        for (int bb = 1; bb < 32; ++bb) a = (bi == bb) ? acc[bb >> 4][bb & 15] : a;
        const float v = scale * a;
        if (v > s[KP - 1]) list_insert<KP>(s, ix, v, kb0 + 32 * (bi >> 4) + key_off(bi & 15));
      }
    }
  }

  if (qg < p.Mx) {
    const long o = ((long)(ks * 2 + h) * p.Mx + qg) * KP;
#pragma unroll
    for (int t = 0; t < KP; ++t) { p.part_s[o + t] = s[t]; p.part_i[o + t] = ix[t]; }
  }
}

int kcpad(int kc) { return kc <= 16 ? 16 : kc <= 32 ? 32 : 64; }

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

template <int KP>
int cand_launch(CKPm p, int Mx, int Ny, int kc, bool x3, float* cs, int64_t* ci, char* lists, hipStream_t st) {
  int nqb, ksplit;
  plan(Mx, Ny, PLQ, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  const int la = 2 * ksplit, lb = (la + MG - 1) / MG;
  const size_t per_list = (size_t)Mx * KP;
  float* a_s = reinterpret_cast<float*>(lists);
  int* a_i = reinterpret_cast<int*>(a_s + la * per_list);
  float* b_s = reinterpret_cast<float*>(a_i + la * per_list);
  int* b_i = reinterpret_cast<int*>(b_s + lb * per_list);
  p.part_s = a_s; p.part_i = a_i;
  if (x3) hipLaunchKernelGGL((sim_cand_kernel<KP, true>), dim3(nqb, ksplit), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((sim_cand_kernel<KP, false>), dim3(nqb, ksplit), dim3(256), 0, st, p);
  int rc = clipk_check_launch();
  if (rc) return rc;
  const float* src_s = a_s; const int* src_i = a_i;
  float* dst_s = b_s; int* dst_i = b_i;
  for (int L = la;;) {
    const int groups = (L + MG - 1) / MG;
    if (groups == 1) {
      hipLaunchKernelGGL(topk_merge_kernel<KP>, dim3(Mx, 1), dim3(256), 0, st, src_s, src_i, L, Mx,
                         (float*)nullptr, (int*)nullptr, cs, ci, kc, Ny);
      return clipk_check_launch();
    }
    hipLaunchKernelGGL(topk_merge_kernel<KP>, dim3(Mx, groups), dim3(256), 0, st, src_s, src_i, L, Mx, dst_s, dst_i,
                       (float*)nullptr, (int64_t*)nullptr, kc, Ny);
    if ((rc = clipk_check_launch())) return rc;
    L = groups;
    float* ts = const_cast<float*>(src_s); int* ti = const_cast<int*>(src_i);
    src_s = dst_s; src_i = dst_i; dst_s = ts; dst_i = ti;
  }
}

struct RRP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P; float scale;
  const int64_t* cidx; const float* cs; int kc, k;
  double eps_rel; const float* ynorm;
  float* scores; int64_t* idx; int* cert;
};

__global__ __launch_bounds__(256) void sim_rerank_kernel(const RRP p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (RBK + 4)];
  __shared__ float ex[64];
  __shared__ int ej[64], er[64];
  __shared__ double red[4];
  __shared__ float tks;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q = blockIdx.x, P = p.P, Ny = p.Ny, kc = p.kc, k = p.k;
  const float* xq = p.X + (long)q * P;
  const float* xrows[RBK / 16];
  const float* yrows[RBK / 16];
#pragma unroll
  for (int i = 0; i < RBK / 16; ++i) {
    const int c = (tid + i * 256) / (RBK / 4);                            // key row c of the tile: candidate c
    int64_t j = c < kc ? p.cidx[(long)q * kc + c] : 0;
    j = (j >= 0 && j < Ny) ? j : 0;
    yrows[i] = p.Y + j * P;
    xrows[i] = xq;
  }
  if (tid < 64) {
    const int64_t j = tid < kc ? p.cidx[(long)q * kc + tid] : -1;
    const float a = tid < kc ? p.cs[(long)q * kc + tid] : -INFINITY;
    er[tid] = (a > -INFINITY && j >= 0 && j < Ny);                        // the fillers of a short list carry -inf
    ej[tid] = er[tid] ? (int)j : INT_MAX;
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  s_tile<RBK>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
  if (wn == 0 && li == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) ex[wm * 32 + keyrow32(r, h)] = p.scale * acc[r];
  }
  double ss = 0.0;
  for (int c = tid; c < P; c += 256) ss += (double)xq[c] * (double)xq[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) red[wid] = ss;
  if (tid == 0) tks = -INFINITY;
  __syncthreads();
  if (tid < kc && er[tid]) {
    const float v = ex[tid];
    const int j = ej[tid];
    int rank = 0;
    for (int u = 0; u < kc; ++u) rank += er[u] && (ex[u] > v || (ex[u] == v && ej[u] < j));
    if (rank < k) { p.scores[(long)q * k + rank] = v; p.idx[(long)q * k + rank] = j; }
    if (rank == k - 1) tks = v;
  }
  __syncthreads();
  if (tid == 0) {
    int nreal = 0;
    bool nan = false;
    for (int u = 0; u < kc; ++u) { nreal += er[u]; nan |= er[u] && ex[u] != ex[u]; }
    for (int t = nreal; t < k; ++t) { p.scores[(long)q * k + t] = -INFINITY; p.idx[(long)q * k + t] = 0; }
    const double tk = (double)tks;
    bool ok = !nan && nreal >= k && tk > -INFINITY;
    if (ok && nreal < Ny) {                                               // nreal == Ny: every key is a candidate
      const double xn = sqrt(red[0] + red[1] + red[2] + red[3]) * (1.0 + 0x1p-30);
      const double yn = (double)p.ynorm[0], sc = fabs((double)p.scale), mag = xn * yn;
      const double c = (double)p.cs[(long)q * kc + kc - 1];              // the weakest approximate candidate
      const double eps = (sc * mag * p.eps_rel + (sc * P * (xn + yn + 1.0) + 1.0) * 0x1p-120) * (1.0 + 0x1p-30);
      ok = nreal == kc && mag * (sc > 1.0 ? sc : 1.0) < 0x1p126 && tk > c + eps;
    }
    p.cert[q] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" int clipk_split_bf16(const float* X, int n_rows, int P, void* hi, void* lo, float* norm_max, void* stream) {
  if (!X || !hi || n_rows <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if (P % 4 || P > PF_MAX_P) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(hi) || (lo && !aligned16(lo))) return CLIPK_ERR_BAD_ARG;
  hipLaunchKernelGGL(split_bf16_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, n_rows, P,
                     plane_pitch(P), static_cast<unsigned short*>(hi), static_cast<unsigned short*>(lo), norm_max);
  return clipk_check_launch();
}

extern "C" size_t clipk_sim_topk_cand_workspace(int Mx, int Ny, int P, int kc, int planes) {
  if (!shape_ok(Mx, Ny, P) || P % 4 || P > PF_MAX_P || kc < 1 || kc > 64 || (planes != 1 && planes != 2)) return 0;
  int nqb, ksplit, tps, nt;
  plan(Mx, Ny, PLQ, &nqb, &ksplit, &tps, &nt);
  const size_t la = 2 * (size_t)ksplit, lb = (la + MG - 1) / MG;
  return round256((size_t)planes * Mx * plane_pitch(P) * 2) +
         (la + lb) * (size_t)Mx * kcpad(kc) * (sizeof(float) + sizeof(int));
}

extern "C" int clipk_sim_topk_cand(const float* X, int Mx, const void* Yhi, const void* Ylo, int Ny, int P, float scale,
                                   int kc, float* cand_scores, int64_t* cand_idx, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!X || !Yhi || !cand_scores || !cand_idx || !workspace) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0 || kc < 1 || kc > 64) return CLIPK_ERR_BAD_ARG;
  if (P % 4 || P > PF_MAX_P || !shape_ok(Mx, Ny, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(Yhi) || (Ylo && !aligned16(Ylo)) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  const int planes = Ylo ? 2 : 1;
  if (workspace_bytes < clipk_sim_topk_cand_workspace(Mx, Ny, P, kc, planes)) return CLIPK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int PP = plane_pitch(P);
  unsigned short* xh = static_cast<unsigned short*>(workspace);          // the queries' planes, split once per call
  unsigned short* xl = Ylo ? xh + (size_t)Mx * PP : nullptr;
  char* lists = static_cast<char*>(workspace) + round256((size_t)planes * Mx * PP * 2);
  hipLaunchKernelGGL(split_bf16_kernel, dim3((Mx + 3) / 4), dim3(256), 0, st, X, Mx, P, PP, xh, xl, (float*)nullptr);
  int rc = clipk_check_launch();
  if (rc) return rc;
  CKPm p{};
  p.xh = xh; p.xl = xl; p.Mx = Mx;
  p.yh = static_cast<const unsigned short*>(Yhi); p.yl = static_cast<const unsigned short*>(Ylo); p.Ny = Ny;
  p.PP = PP; p.scale = scale;
  switch (kcpad(kc)) {
    case 16: return cand_launch<16>(p, Mx, Ny, kc, Ylo != nullptr, cand_scores, cand_idx, lists, st);
    case 32: return cand_launch<32>(p, Mx, Ny, kc, Ylo != nullptr, cand_scores, cand_idx, lists, st);
    default: return cand_launch<64>(p, Mx, Ny, kc, Ylo != nullptr, cand_scores, cand_idx, lists, st);
  }
}

extern "C" int clipk_sim_rerank(const float* X, int Mx, const float* Y, int Ny, int P, float scale,
                                const int64_t* cand_idx, const float* cand_scores, int kc, int k, double eps_rel,
                                const float* y_norm_max, float* scores, int64_t* idx, int* certified, void* stream) {
  if (!X || !Y || !cand_idx || !cand_scores || !y_norm_max || !scores || !idx || !certified) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0 || k < 1 || k > kc || kc > 64 || k > Ny) return CLIPK_ERR_BAD_ARG;
  if (!(eps_rel >= 0.0 && eps_rel < 1.0)) return CLIPK_ERR_BAD_ARG;
  if (P % 4 || P > PF_MAX_P || !shape_ok(Mx, Ny, P)) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(Y)) return CLIPK_ERR_BAD_ARG;
  RRP p;
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale;
  p.cidx = cand_idx; p.cs = cand_scores; p.kc = kc; p.k = k; p.eps_rel = eps_rel; p.ynorm = y_norm_max;
  p.scores = scores; p.idx = idx; p.cert = certified;
  hipLaunchKernelGGL(sim_rerank_kernel, dim3(Mx), dim3(256), 0, (hipStream_t)stream, p);
  return clipk_check_launch();
}
