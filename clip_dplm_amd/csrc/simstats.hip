// simstats.hip — embedding-space diagnostics without the similarity matrix (include/clipk.h: clipk_sim_stats).
// One pass over S[i,j] = scale <X_i, Y_j> on the tiled exact-f32 block of sim_tile.h (64 queries per workgroup, 64-key
// tiles, keys on the MFMA rows, one query per lane, 16 keys per lane per tile, key-range splits on grid y: the walk of
// sim_rank_kernel) with a statistics epilogue: per query the positive's score, the best key and the best negative, the
// softmax statistics (running max / sum as simce_lse_tiled_kernel) and the f64 sums of S and S^2 over the negatives;
// globally the histogram of the negatives' scores and of the positives'.  S never reaches HBM.
//
// Sets (include/clipk.h has the definitions): E_i = keys of the query's class other than its label ("mask" rule of the
// class-aware loss; empty without ids), N_i = every other key except the label.  CLS = false is the plain kernel:
// every class line sits under `if constexpr`.
//
// Per tile a lane forms two 16-bit masks over its accumulator rows (d: key in {l_i} u N_i, n: key in N_i).  Interior
// tiles that hold neither the lane's label nor an excluded key take the epilogue with both masks constant.
//
// Histogram: lane-private columns.  hist[slot][32] in LDS, lane (li, h) adds to column li: the 32 lanes of a half wave
// hit 32 different banks whatever their slots are, the two halves collide at most two ways, and no ds_add of one
// wave-instruction shares an address with another lane's except its partner in the other half.  For real embeddings
// the negatives crowd into two or three slots; hist[slot] alone would serialise 64 lanes on one address.  The columns
// are summed once per workgroup and flushed with 64-bit integer global atomics (exact, order-free): <= nbins + 2 per
// workgroup.  The positives are binned by the finalize kernel with the same device function.
//
// f64 sums: a lane adds its 16 masked values of a tile in f32 (squares as an fma chain), converts the two tile
// partials to f64 and adds them to f64 running sums; lane halves, key-waves and splits merge in f64 in a fixed order.
#include "common.h"
#include "sim_tile.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int SQ = 64, SK = 64;          // queries per workgroup, keys per tile
constexpr int SBK = 32;                  // K-step of the tile loop (as the rank / LSE passes)
constexpr int HB_MAX = 256;              // histogram bins (the two outer slots come on top)
constexpr int HCOL = 32;                 // lane-private columns per slot: one LDS bank each

__device__ __forceinline__ int st_key_off(int r) { return (r & 3) + 8 * (r >> 2); }   // keyrow32(r, h) - 4 h

__device__ __forceinline__ int st_label_of(const int64_t* labels, int64_t label_offset, int q, int Ny) {
  const int64_t l = labels ? labels[q] : label_offset + q;
  return (l >= 0 && l < Ny) ? (int)l : -1;
}

// the binning rule of include/clipk.h: subtraction and product in f32, the quotient clamped before the conversion.
// __fsub_rn / __fmul_rn (and __fmul_rn for every S = scale * acc): individually rounded operations the compiler may not
// contract into a fused multiply-add, so the kernel bins the same rounded S that the finalize kernel reads back as pos
__device__ __forceinline__ int st_slot(float s, float lo, float hi, float inv_w, int nbins) {
  float t = __fmul_rn(__fsub_rn(s, lo), inv_w);
  t = fminf(fmaxf(t, 0.f), (float)(nbins - 1));                           // NaN -> 0; int(min(t, n - 1)) = min(int(t), n - 1)
  return s < lo ? 0 : (s >= hi ? nbins + 1 : 1 + (int)t);
}

// (v, i) <- the better of (v, i) and (ov, oi): score descending, equal scores by the lower index; i = -1: empty
__device__ __forceinline__ void st_take(float& v, int& i, float ov, int oi) {
  const bool t = oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i));
  v = t ? ov : v; i = t ? oi : i;
}

__device__ __forceinline__ void st_ml_merge(float& m, float& l, float mo, float lo_) {
  const float mn = fmaxf(m, mo);
  float ln = 0.f;
  if (mn > -INFINITY) ln = l * expf(m - mn) + lo_ * expf(mo - mn);
  m = mn; l = ln;
}

struct SSP {
  const float* X; int Mx;
  const float* Y; int Ny;
  int P; float scale;
  const int64_t* labels; int64_t label_offset;
  const int64_t* cls_x; const int64_t* cls_y;   // CLS instantiation only
  int nbins; float lo, hi, inv_w;
  float* pos;                              // [Mx]
  double* part_d;                          // [ksplit][Mx][2]: sum, sum of squares over N_i
  float* part_f;                           // [ksplit][Mx][4]: best, hard, m, l
  int* part_i;                             // [ksplit][Mx][2]: best_idx, hard_idx
  unsigned long long* hist_neg;            // [nbins + 2]
  int tiles_per_split, ntiles;
};

template <bool CLS>
__global__ __launch_bounds__(256, 2) void sim_stats_kernel(const SSP p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * 64 * (SBK + 4)];
  __shared__ unsigned hist[(HB_MAX + 2) * HCOL];
  __shared__ int labl[SQ];
  __shared__ float posl[SQ];
  __shared__ double mrg_d[2][SQ];
  __shared__ float mrg_f[4][SQ];
  __shared__ int mrg_i[2][SQ];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * SQ, ks = blockIdx.y;
  const int P = p.P, Ny = p.Ny, nbins = p.nbins;
  const float scale = p.scale, lo = p.lo, hi = p.hi, inv_w = p.inv_w;
  const float* xrows[SBK / 16];
#pragma unroll
  for (int i = 0; i < SBK / 16; ++i) {
    int q = q0 + (tid + i * 256) / (SBK / 4); q = q < p.Mx ? q : p.Mx - 1;   // clamped: computed and dropped
    xrows[i] = p.X + (long)q * P;
  }
  for (int e = tid; e < (nbins + 2) * HCOL; e += 256) hist[e] = 0u;
  if (tid < SQ) {
    const int q = q0 + tid;
    labl[tid] = st_label_of(p.labels, p.label_offset, q < p.Mx ? q : p.Mx - 1, Ny);
  }
  __syncthreads();

  // ---- S[q, l_q] from the gathered tile of sim_rank_kernel: the bits clipk_sim_rank returns
  {
    const float* yrows[SBK / 16];
#pragma unroll
    for (int i = 0; i < SBK / 16; ++i) {
      const int l = labl[(tid + i * 256) / (SBK / 4)];
      yrows[i] = p.Y + (long)(l < 0 ? 0 : l) * P;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<SBK>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);
    if (wm == wn) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (keyrow32(r, h) == li) posl[wn * 32 + li] = __fmul_rn(scale, acc[r]);
    }
    __syncthreads();
  }
  const int qg = q0 + wn * 32 + li;                                       // this lane's query
  const int lab = labl[wn * 32 + li];
  const bool rowok = qg < p.Mx && lab >= 0;                               // other rows enter nothing
  int64_t cq = 0;
  if constexpr (CLS) cq = p.cls_x[qg < p.Mx ? qg : p.Mx - 1];
  float bv = -INFINITY, hv = -INFINITY, m_run = -INFINITY, l_run = 0.f;
  int bi = -1, hix = -1;
  double dsum = 0.0, dsq = 0.0;
  unsigned* hcol = hist + li;
  const int t_beg = ks * p.tiles_per_split;
  int t_end = t_beg + p.tiles_per_split; t_end = t_end < p.ntiles ? t_end : p.ntiles;

  for (int kt = t_beg; kt < t_end; ++kt) {
    const int j0 = kt * SK;
    const float* yrows[SBK / 16];
#pragma unroll
    for (int i = 0; i < SBK / 16; ++i) {
      int j = j0 + (tid + i * 256) / (SBK / 4); j = j < Ny ? j : Ny - 1;
      yrows[i] = p.Y + (long)j * P;
    }
    const int kb = j0 + wm * 32 + 4 * h;                                  // key of accumulator row r: kb + st_key_off(r)
    unsigned dm = 0xffffu, lm = 0u;                                       // rows in {l_i} u N_i; the label's row
    if (j0 + SK > Ny) {
#pragma unroll
      for (int r = 0; r < 16; ++r) if (kb + st_key_off(r) >= Ny) dm &= ~(1u << r);
    }
    if (lab >= j0 && lab < j0 + SK) {
#pragma unroll
      for (int r = 0; r < 16; ++r) if (kb + st_key_off(r) == lab) lm |= 1u << r;
    }
    if constexpr (CLS) {                                                  // ids of the lane's 16 key rows, before the K-loop
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + st_key_off(r);
        if (key < Ny && key != lab && p.cls_y[key] == cq) dm &= ~(1u << r);
      }
    }
    if (!rowok) dm = 0u;
    const unsigned nm = dm & ~lm;                                         // rows in N_i
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    s_tile<SBK>(acc, yrows, xrows, smem, P, tid, wm, wn, li, h);

    float sv[16], tmax = -INFINITY, hmax = -INFINITY, ts = 0.f, tq = 0.f;
    if (nm == 0xffffu) {                                                  // interior tile, no label, nothing excluded
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = __fmul_rn(scale, acc[r]);
        sv[r] = s;
        tmax = fmaxf(tmax, s);
        ts += s;
        tq = fmaf(s, s, tq);
        atomicAdd(hcol + st_slot(s, lo, hi, inv_w, nbins) * HCOL, 1u);
      }
      hmax = tmax;
      if (hmax > hv) {                                                    // strictly better: the earlier tile keeps ties
        hv = hmax;
#pragma unroll
        for (int r = 15; r >= 0; --r) if (sv[r] == hmax) hix = kb + st_key_off(r);   // ends at the lowest key
      }
    } else {
      float nv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = __fmul_rn(scale, acc[r]);
        const bool d = (dm >> r) & 1u, n = (nm >> r) & 1u;
        sv[r] = d ? s : -INFINITY;
        nv[r] = n ? s : -INFINITY;
        tmax = fmaxf(tmax, sv[r]);
        hmax = fmaxf(hmax, nv[r]);
        const float z = n ? s : 0.f;
        ts += z;
        tq = fmaf(z, z, tq);
        if (n) atomicAdd(hcol + st_slot(s, lo, hi, inv_w, nbins) * HCOL, 1u);
      }
      if (hmax > hv) {
        hv = hmax;
#pragma unroll
        for (int r = 15; r >= 0; --r) if (((nm >> r) & 1u) && nv[r] == hmax) hix = kb + st_key_off(r);
      }
    }
    if (tmax > bv) {
      bv = tmax;
#pragma unroll
      for (int r = 15; r >= 0; --r) if (((dm >> r) & 1u) && sv[r] == tmax) bi = kb + st_key_off(r);
    }
    if (tmax > -INFINITY) {                                               // the running (max, sum) of simce_lse_tiled_kernel
      const float m_new = fmaxf(m_run, tmax);
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += expf(sv[r] - m_new);             // exp(-inf) = 0 for rows outside the set
      l_run = l_run * expf(m_run - m_new) + a;
      m_run = m_new;
    }
    dsum += (double)ts;
    dsq += (double)tq;
  }

  // ---- the four owners of a query: lane halves, then the two key-waves
  st_take(bv, bi, __shfl_xor(bv, 32, 64), __shfl_xor(bi, 32, 64));
  st_take(hv, hix, __shfl_xor(hv, 32, 64), __shfl_xor(hix, 32, 64));
  st_ml_merge(m_run, l_run, __shfl_xor(m_run, 32, 64), __shfl_xor(l_run, 32, 64));
  dsum += __shfl_xor(dsum, 32, 64);
  dsq += __shfl_xor(dsq, 32, 64);
  const int ql = wn * 32 + li;
  if (wm == 1 && h == 0) {
    mrg_f[0][ql] = bv; mrg_f[1][ql] = hv; mrg_f[2][ql] = m_run; mrg_f[3][ql] = l_run;
    mrg_i[0][ql] = bi; mrg_i[1][ql] = hix;
    mrg_d[0][ql] = dsum; mrg_d[1][ql] = dsq;
  }
  __syncthreads();                                                        // also: every wave's histogram adds are done
  if (wm == 0 && h == 0 && qg < p.Mx) {
    st_take(bv, bi, mrg_f[0][ql], mrg_i[0][ql]);
    st_take(hv, hix, mrg_f[1][ql], mrg_i[1][ql]);
    st_ml_merge(m_run, l_run, mrg_f[2][ql], mrg_f[3][ql]);
    const long o = (long)ks * p.Mx + qg;
    p.part_d[o * 2] = dsum + mrg_d[0][ql]; p.part_d[o * 2 + 1] = dsq + mrg_d[1][ql];
    p.part_f[o * 4] = bv; p.part_f[o * 4 + 1] = hv; p.part_f[o * 4 + 2] = m_run; p.part_f[o * 4 + 3] = l_run;
    p.part_i[o * 2] = bi; p.part_i[o * 2 + 1] = hix;
    if (ks == 0) p.pos[qg] = lab >= 0 ? posl[ql] : __builtin_nanf("");
  }
  // ---- histogram columns -> one count per slot -> global (the column index is rotated: 32 threads, 32 banks)
  for (int slot = tid; slot < nbins + 2; slot += 256) {
    unsigned long long c = 0;
#pragma unroll 8
    for (int k = 0; k < HCOL; ++k) c += hist[slot * HCOL + ((k + tid) & (HCOL - 1))];
    if (c) atomicAdd(p.hist_neg + slot, c);
  }
}

struct SSF {
  const double* part_d; const float* part_f; const int* part_i;
  int ksplit, Mx, Ny;
  const int64_t* labels; int64_t label_offset;
  int nbins; float lo, hi, inv_w;
  const float* pos;
  float* best; int64_t* best_idx; float* hard; int64_t* hard_idx; float* lse;
  double* neg_sum; double* neg_sumsq;
  unsigned long long* hist_pos;
};

// one thread per query: the splits' partials in ascending split order (a split's keys precede the next one's, but
// st_take does not rely on it), then the positive's slot
__global__ __launch_bounds__(256) void sim_stats_finalize(const SSF f) {
  __shared__ unsigned hp[HB_MAX + 2];
  const int tid = threadIdx.x, q = blockIdx.x * 256 + tid;
  for (int e = tid; e < f.nbins + 2; e += 256) hp[e] = 0u;
  __syncthreads();
  if (q < f.Mx) {
    float bv = -INFINITY, hv = -INFINITY, m = -INFINITY, l = 0.f;
    int bi = -1, hix = -1;
    double ds = 0.0, dq = 0.0;
    for (int s = 0; s < f.ksplit; ++s) m = fmaxf(m, f.part_f[((long)s * f.Mx + q) * 4 + 2]);
    for (int s = 0; s < f.ksplit; ++s) {
      const long o = (long)s * f.Mx + q;
      st_take(bv, bi, f.part_f[o * 4], f.part_i[o * 2]);
      st_take(hv, hix, f.part_f[o * 4 + 1], f.part_i[o * 2 + 1]);
      const float ms = f.part_f[o * 4 + 2], ls = f.part_f[o * 4 + 3];
      if (ms > -INFINITY) l += ls * expf(ms - m);
      ds += f.part_d[o * 2]; dq += f.part_d[o * 2 + 1];
    }
    f.best[q] = bv; f.best_idx[q] = bi; f.hard[q] = hv; f.hard_idx[q] = hix;
    f.lse[q] = m + logf(l);
    f.neg_sum[q] = ds; f.neg_sumsq[q] = dq;
    if (st_label_of(f.labels, f.label_offset, q, f.Ny) >= 0)
      atomicAdd(hp + st_slot(f.pos[q], f.lo, f.hi, f.inv_w, f.nbins), 1u);
  }
  __syncthreads();
  for (int e = tid; e < f.nbins + 2; e += 256)
    if (hp[e]) atomicAdd(f.hist_pos + e, (unsigned long long)hp[e]);
}

__global__ void sim_stats_zero(unsigned long long* a, unsigned long long* b, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) { a[e] = 0ull; b[e] = 0ull; }
}

// the plan of retrieval.hip (one workgroup per 64-query block and key split, >= 2 workgroups per CU, option
// retrieval_splits), with at most 2^24 tiles per split: a histogram column then stays below 2^31 counts
void st_plan(int Mx, int Ny, int* nqb, int* ksplit, int* tps, int* ntiles) {
  *nqb = (Mx + SQ - 1) / SQ;
  *ntiles = (Ny + SK - 1) / SK;
  const int opt = clipk_opt_get(OPT_RETRIEVAL_SPLITS);
  int ks = opt > 0 ? opt : (512 + *nqb - 1) / *nqb;
  if (ks > 65535) ks = 65535;
  if (ks > *ntiles) ks = *ntiles;
  if (ks < 1) ks = 1;
  *tps = (*ntiles + ks - 1) / ks;
  if (*tps > (1 << 24)) *tps = 1 << 24;
  *ksplit = (*ntiles + *tps - 1) / *tps;
}

bool st_shape_ok(int Mx, int Ny, int P, int nbins) {
  return Mx > 0 && Ny > 0 && P > 0 && Ny <= INT_MAX - SK && nbins >= 1 && nbins <= HB_MAX;
}

}  // namespace

extern "C" size_t clipk_sim_stats_workspace(int Mx, int Ny, int P, int nbins) {
  if (!st_shape_ok(Mx, Ny, P, nbins) || P % 4) return 0;
  int nqb, ksplit, tps, nt;
  st_plan(Mx, Ny, &nqb, &ksplit, &tps, &nt);
  return (size_t)ksplit * Mx * (2 * sizeof(double) + 4 * sizeof(float) + 2 * sizeof(int));
}

extern "C" int clipk_sim_stats(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const int64_t* labels,
                               int64_t label_offset, const int64_t* cls_x, const int64_t* cls_y, int nbins, float lo,
                               float hi, float* pos, float* best, int64_t* best_idx, float* hard, int64_t* hard_idx,
                               float* lse, double* neg_sum, double* neg_sumsq, int64_t* hist_neg, int64_t* hist_pos,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !Y || !pos || !best || !best_idx || !hard || !hard_idx || !lse || !neg_sum || !neg_sumsq || !hist_neg ||
      !hist_pos || !workspace)
    return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0) return CLIPK_ERR_BAD_ARG;
  if ((cls_x == nullptr) != (cls_y == nullptr)) return CLIPK_ERR_BAD_ARG;
  if (nbins < 1 || nbins > HB_MAX || !(lo < hi) || !isfinite(lo) || !isfinite(hi)) return CLIPK_ERR_BAD_ARG;
  if (P % 4 || !st_shape_ok(Mx, Ny, P, nbins)) return CLIPK_ERR_UNSUPPORTED;
  if (!labels && (label_offset < 0 || label_offset + Mx > Ny)) return CLIPK_ERR_BAD_ARG;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(workspace)) return CLIPK_ERR_BAD_ARG;
  if (workspace_bytes < clipk_sim_stats_workspace(Mx, Ny, P, nbins)) return CLIPK_ERR_BAD_ARG;
  const float inv_w = (float)((double)nbins / ((double)hi - (double)lo));   // rounded once
  if (!isfinite(inv_w)) return CLIPK_ERR_BAD_ARG;
  SSP p{};
  p.X = X; p.Mx = Mx; p.Y = Y; p.Ny = Ny; p.P = P; p.scale = scale; p.labels = labels; p.label_offset = label_offset;
  p.cls_x = cls_x; p.cls_y = cls_y; p.nbins = nbins; p.lo = lo; p.hi = hi; p.inv_w = inv_w; p.pos = pos;
  int nqb, ksplit;
  st_plan(Mx, Ny, &nqb, &ksplit, &p.tiles_per_split, &p.ntiles);
  const size_t rows = (size_t)ksplit * Mx;
  p.part_d = static_cast<double*>(workspace);
  p.part_f = reinterpret_cast<float*>(p.part_d + 2 * rows);
  p.part_i = reinterpret_cast<int*>(p.part_f + 4 * rows);
  p.hist_neg = reinterpret_cast<unsigned long long*>(hist_neg);
  unsigned long long* hpos = reinterpret_cast<unsigned long long*>(hist_pos);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sim_stats_zero, dim3((nbins + 2 + 255) / 256), dim3(256), 0, st, p.hist_neg, hpos, nbins + 2);
  int rc = clipk_check_launch();
  if (rc) return rc;
  if (cls_x) hipLaunchKernelGGL(sim_stats_kernel<true>, dim3(nqb, ksplit), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(sim_stats_kernel<false>, dim3(nqb, ksplit), dim3(256), 0, st, p);
  if ((rc = clipk_check_launch())) return rc;
  SSF f{};
  f.part_d = p.part_d; f.part_f = p.part_f; f.part_i = p.part_i; f.ksplit = ksplit; f.Mx = Mx; f.Ny = Ny;
  f.labels = labels; f.label_offset = label_offset; f.nbins = nbins; f.lo = lo; f.hi = hi; f.inv_w = inv_w;
  f.pos = pos; f.best = best; f.best_idx = best_idx; f.hard = hard; f.hard_idx = hard_idx; f.lse = lse;
  f.neg_sum = neg_sum; f.neg_sumsq = neg_sumsq; f.hist_pos = hpos;
  hipLaunchKernelGGL(sim_stats_finalize, dim3((Mx + 255) / 256), dim3(256), 0, st, f);
  return clipk_check_launch();
}
