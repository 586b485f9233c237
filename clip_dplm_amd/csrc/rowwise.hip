// rowwise.hip — HBM-bound row kernels: LayerNorm fwd/bwd (+fused activation), L2-normalise fwd/bwd.
// One wave (64 lanes) per row, whole row held in registers as 4-element chunks (16-byte f32 loads,
// 8-byte bf16 loads), f32 statistics with wave-shuffle reductions — no LDS, no re-reads; beyond 2048 columns the
// LayerNorm forward and its all-f32 backward give a row to a whole workgroup (RowGeom below).
// Reference ops: nn.LayerNorm at old/clip.py:12,28,32, the LayerNorms inside nn.TransformerEncoderLayer
// (rna_clip_codes.ipynb:1915-1916) and EsmLayer (modeling_esm.py:429-438,552-553); F.normalize at
// old/clip.py:63-64.
#include "common.h"

namespace {

template <bool BF16>
__device__ __forceinline__ f32x4 load4(const void* base, long off) {
  if (BF16) {
    const u32x2 r = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(base) + off);
    return f32x4{bf16_to_f32((unsigned short)(r[0] & 0xffffu)), bf16_to_f32((unsigned short)(r[0] >> 16)),
                 bf16_to_f32((unsigned short)(r[1] & 0xffffu)), bf16_to_f32((unsigned short)(r[1] >> 16))};
  } else {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
  }
}
__device__ __forceinline__ void store4_bf16(void* base, long off, f32x4 v) {
  u32x2 o;
  o[0] = pack_bf16x2(v[0], v[1]);
  o[1] = pack_bf16x2(v[2], v[3]);
  *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(base) + off) = o;
}

__device__ __forceinline__ float sum4(float a, float b, float c, float d) { return (a + b) + (c + d); }

// ---- row geometry: NW waves share a row ------------------------------------------------------------
// NW = 1: a wave per row, four rows per block, lane l holds the chunks l + 64 v.  NW = 4 (wide rows, cols > 2048: the
// 2560-wide hidden LayerNorms of the notebook's projection heads, rna_clip_codes.ipynb:1887-1903): a WORKGROUP per row,
// the four waves take interleaved 256-float segments (chunk = lane + 64 (4 v + wave)) and row sums meet in LDS.  The
// one-wave form needs 20 float4 per lane and array there (560 registers in the backward: it lived in scratch, 48 us
// for 32 rows).  A row's arithmetic depends on NW and the width only, never on the batch.
template <int NW>
struct RowGeom {
  static_assert(NW == 1 || NW == 4, "a wave or a 256-thread workgroup per row");
  // ---- the geometry itself, stateless (lane: of its wave, wid: the wave of its block)
  __device__ __forceinline__ static int chunk(int lane, int wid, int v) {
    return NW == 1 ? lane + 64 * v : lane + 64 * (NW * v + wid);
  }
  // the grid-stride walk over rows: a kernel's waves (NW = 1) or blocks (NW = 4).  block_threads: blockDim.x, read in the
  // kernel itself - there the compiler knows that no workgroup of the grid is a partial one; read in a device function it
  // costs a compare and a select on the block index per use
  __device__ __forceinline__ static int first_row(unsigned block_threads) {
    return NW == 1 ? (blockIdx.x * block_threads + threadIdx.x) >> 6 : blockIdx.x;
  }
  __device__ __forceinline__ static int row_step(unsigned block_threads) {
    return NW == 1 ? (gridDim.x * block_threads) >> 6 : gridDim.x;
  }
  // The mean of a row quantity from every lane's partial sum: wave shuffles, and for NW = 4 one float per wave in LDS
  // slot 0 or 1, added as (w0 + w1) + (w2 + w3).  One barrier: a caller alternates the slots, so every wave has read a
  // slot's last sums before anyone passes the barrier behind which it is written again.
  __device__ __forceinline__ static float* red(int slot) {
    __shared__ float r[2][4];
    return r[slot];
  }
  __device__ __forceinline__ static float row_mean(int lane, int wid, float s, float inv_n, int slot) {
    s = wave_sum(s);
    if constexpr (NW == 4) {
      float* r = red(slot);
      if (lane == 0) r[wid] = s;
      __syncthreads();
      s = sum4(r[0], r[1], r[2], r[3]);
    }
    return s * inv_n;
  }
  // Two at once, both slots every row: a second barrier, "the previous row's sums have been read by every wave"
  __device__ __forceinline__ static void row_means(int lane, int wid, float& a, float& b, float inv_n) {
    if constexpr (NW == 4) {
      a = wave_sum(a); b = wave_sum(b);
      float *r0 = red(0), *r1 = red(1);
      __syncthreads();
      if (lane == 0) { r0[wid] = a; r1[wid] = b; }
      __syncthreads();
      a = sum4(r0[0], r0[1], r0[2], r0[3]) * inv_n;
      b = sum4(r1[0], r1[1], r1[2], r1[3]) * inv_n;
    } else {
      a = wave_sum(a) * inv_n;
      b = wave_sum(b) * inv_n;
    }
  }

  // ---- one thread's view of it, for the kernels that hand it to the helpers below.  (ln_bwd_kernel uses the static
  // functions with locals of its own: with an object its NW = 1 forms order their address arithmetic differently from the
  // parent's, profiles/ln_fold/README.md.)
  const int lane, wid;
  const unsigned block_threads;
  const int row0, step;
  __device__ __forceinline__ explicit RowGeom(unsigned block_dim_x)
      : lane(threadIdx.x & 63), wid(threadIdx.x >> 6), block_threads(block_dim_x),
        row0(first_row(block_dim_x)), step(row_step(block_dim_x)) {}
  __device__ __forceinline__ int chunk(int v) const { return chunk(lane, wid, v); }
  __device__ __forceinline__ bool row_leader() const { return NW == 1 ? lane == 0 : threadIdx.x == 0; }
  __device__ __forceinline__ float row_mean(float s, float inv_n, int slot) const { return row_mean(lane, wid, s, inv_n, slot); }
  // One row sum kept as NS segment sums.  NS = 4 is a lone wave walking a wide row (NW = 1): its chunk v is the NW = 4
  // geometry's chunk v / 4 of wave v % 4, so segment v % 4 adds what that wave adds, in its order, and the four
  // segment totals are added as the one-sum row_mean adds the four waves' - the bits of the NW = 4 mean.
  template <int NS>
  __device__ __forceinline__ float row_mean(const float (&s)[NS], float inv_n, int slot) const {
    static_assert(NS == 1 || (NS == 4 && NW == 1), "segments stand in for the waves of the NW = 4 form");
    if constexpr (NS == 4) return sum4(wave_sum(s[0]), wave_sum(s[1]), wave_sum(s[2]), wave_sum(s[3])) * inv_n;
    else return row_mean(s[0], inv_n, slot);
  }
};

// the waves that share a row of VPL-wide chunk arrays in clipk_layernorm_fwd: what launches its kernel, and what
// ln_pool_fwd_kernel sums its segments by so that mean / rstd are that entry's bits
constexpr int ln_fwd_row_waves(int vpl) { return vpl == 20 ? 4 : 1; }

// gamma and (want_beta) beta chunks of this lane, zero beyond the row's end
template <int V, int NW>
__device__ __forceinline__ void ln_load_params(const RowGeom<NW> t, int nch, const float* gamma, const float* beta,
                                               bool want_beta, f32x4 (&g)[V], f32x4 (&b)[V]) {
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = t.chunk(v);
    g[v] = f32x4{0.f, 0.f, 0.f, 0.f}; b[v] = g[v];
    if (c < nch) {
      g[v] = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
      if (want_beta) b[v] = *reinterpret_cast<const f32x4*>(beta + 4 * c);
    }
  }
}

// A row into registers (zeros beyond its end) with its two-pass mean and rstd, the sums in NS segments (RowGeom::row_mean)
template <bool XBF16, int NS, int V, int NW>
__device__ __forceinline__ void ln_load_row_stats(const RowGeom<NW> t, int nch, const void* xp, long rowoff, float inv_n,
                                                  float eps, f32x4 (&x)[V], float& mean, float& rstd) {
  float s[NS] = {}, q[NS] = {};
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = t.chunk(v);
    f32x4 xv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < nch) xv = load4<XBF16>(xp, rowoff + 4 * c);
    s[NS == 1 ? 0 : v % NS] += (xv[0] + xv[1]) + (xv[2] + xv[3]);
    x[v] = xv;
  }
  mean = t.row_mean(s, inv_n, 0);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    if (t.chunk(v) < nch) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = x[v][e] - mean; q[NS == 1 ? 0 : v % NS] += d * d; }
    }
  }
  const float var = t.row_mean(q, inv_n, 1);   // (slot 1: every wave has read slot 0 before the next row's barrier)
  rstd = rsqrtf(var + eps);
}

// This block's dgamma / dbeta partial row part[blockIdx.x][2][cols], NW = 4: every wave writes its own columns
template <int V>
__device__ __forceinline__ void ln_partials_direct(int lane, int wid, int cols, const f32x4 (&dg)[V], const f32x4 (&db)[V],
                                                   float* part) {
  const int nch = cols >> 2;
  float* out = part + (long)blockIdx.x * 2 * cols;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = RowGeom<4>::chunk(lane, wid, v);
    if (c < nch) {
      *reinterpret_cast<f32x4*>(out + 4 * c) = dg[v];
      *reinterpret_cast<f32x4*>(out + cols + 4 * c) = db[v];
    }
  }
}

// ... NW = 1: the four waves hold partials of the same columns, combined through dynamic LDS [4][2][cols]
template <int V>
__device__ __forceinline__ void ln_partials_through_lds(const RowGeom<1> t, int cols, const f32x4 (&dg)[V],
                                                        const f32x4 (&db)[V], float* part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm = reinterpret_cast<float*>(smem);          // [4][2][cols]
  const int nch = cols >> 2;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = t.chunk(v);
    if (c < nch) {
      *reinterpret_cast<f32x4*>(sm + (t.wid * 2 + 0) * cols + 4 * c) = dg[v];
      *reinterpret_cast<f32x4*>(sm + (t.wid * 2 + 1) * cols + 4 * c) = db[v];
    }
  }
  __syncthreads();
  const int nw = t.block_threads >> 6;
  for (int i = threadIdx.x; i < 2 * cols; i += t.block_threads) {
    float a = 0.f;
    for (int w = 0; w < nw; ++w) a += sm[w * 2 * cols + i];
    part[(long)blockIdx.x * 2 * cols + i] = a;
  }
}

struct LnFwd {
  const void* x; long ldx;
  const float* gamma; const float* beta; float eps; int act;
  float* y_f32; void* y_bf16; long ldy;
  float* mean; float* rstd; int rows, cols;
};

// f32 or bf16 in, f32 and / or bf16 out
template <int V, int NW, bool XBF16>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const LnFwd p) {
  const RowGeom<NW> t(blockDim.x);
  const int nch = p.cols >> 2;
  f32x4 g[V], b[V];
  ln_load_params(t, nch, p.gamma, p.beta, true, g, b);
  const float inv_n = 1.0f / (float)p.cols;
  for (int row = t.row0; row < p.rows; row += t.step) {
    f32x4 x[V];
    float mean, rstd;
    if constexpr (NW == 1 && !XBF16) {
      // ln_load_row_stats<false, 1> spelled out: behind the call (the row array passed by reference) the three f32
      // instantiations allocate 66 / 92 / 140 registers instead of 64 / 90 / 138, and 66 is 7 waves per SIMD instead
      // of 8 at the 480-wide rows (profiles/ln_fold/README.md).  Same operations in the same order.
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c = t.chunk(v);
        x[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nch) x[v] = load4<XBF16>(p.x, (long)row * p.ldx + 4 * c);
        s += (x[v][0] + x[v][1]) + (x[v][2] + x[v][3]);
      }
      mean = wave_sum(s) * inv_n;
      float q = 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c = t.chunk(v);
        if (c < nch) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float d = x[v][e] - mean; q += d * d; }
        }
      }
      const float var = wave_sum(q) * inv_n;
      rstd = rsqrtf(var + p.eps);
    } else {
      ln_load_row_stats<XBF16, 1>(t, nch, p.x, (long)row * p.ldx, inv_n, p.eps, x, mean, rstd);
    }
    if (t.row_leader()) {
      if (p.mean) p.mean[row] = mean;
      if (p.rstd) p.rstd[row] = rstd;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c = t.chunk(v);
      if (c < nch) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = act_apply((x[v][e] - mean) * rstd * g[v][e] + b[v][e], p.act);
        if (p.y_f32) *reinterpret_cast<f32x4*>(p.y_f32 + (long)row * p.ldy + 4 * c) = y;
        if (p.y_bf16) store4_bf16(p.y_bf16, (long)row * p.ldy + 4 * c, y);
      }
    }
  }
}

// LayerNorm + masked mean over the L rows of each sample in one pass (the encoders' final LayerNorm followed by the
// pooling of configuration_hybrid_clip.py:109 use_mean_pooling / tf_clip_codes (1).ipynb:1188): the normalised rows
// are never written (2 x rows x cols x 4 B less per tower and step: one write here, one read by the pooling kernel).
// One workgroup per sample; wave w takes rows w, w + 4, ...; the four partial sums are combined in wave order, so a
// sample's pooled row does not depend on where it sits in the batch.  mean / rstd per row are kept for the backward.
struct LnPool {
  const void* x; long ldx;        // f32 or bf16 (XBF16)
  const float* gamma; const float* beta; float eps;
  const unsigned char* mask;      // [B * L], 1 = valid, or null
  float* pooled; float* mean; float* rstd; float* wrow;   // wrow [B * L]: the row's weight in its mean, 1 / #valid or 0
  int L, cols;
};

template <int VPL, bool XBF16>
__global__ __launch_bounds__(256) void ln_pool_fwd_kernel(const LnPool p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm = reinterpret_cast<float*>(smem);                    // [4][cols] partial sums, then [4] counts
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;     // a wave per row, whatever the width
  const int b = blockIdx.x;
  const int nch = p.cols >> 2;
  f32x4 g[VPL], be[VPL], acc[VPL];
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = lane + 64 * v;
    g[v] = f32x4{0.f, 0.f, 0.f, 0.f}; be[v] = g[v]; acc[v] = g[v];
    if (c < nch) {
      g[v] = *reinterpret_cast<const f32x4*>(p.gamma + 4 * c);
      be[v] = *reinterpret_cast<const f32x4*>(p.beta + 4 * c);
    }
  }
  const float inv_n = 1.0f / (float)p.cols;
  int cnt = 0;
  for (int l = wid; l < p.L; l += 4) {
    const long row = (long)b * p.L + l;
    f32x4 x[VPL];
    float mean, rstd;
    constexpr int NS = ln_fwd_row_waves(VPL);
    if constexpr (NS == 1) {
      // ln_load_row_stats<XBF16, 1> spelled out: behind the call the VPL 2 / 4 / 8 forms allocate 60 / 94 / 408 registers
      // instead of 58 / 92 / 404; with it, the preamble above and no RowGeom object they are the parent's instruction
      // stream (profiles/ln_fold/README.md).  Same operations in the same order.
      float s[NS] = {}, q[NS] = {};
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        const int c = lane + 64 * v;
        x[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nch) x[v] = load4<XBF16>(p.x, row * p.ldx + 4 * c);
        s[v % NS] += (x[v][0] + x[v][1]) + (x[v][2] + x[v][3]);
      }
      mean = wave_sum(s[0]) * inv_n;
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        const int c = lane + 64 * v;
        if (c < nch) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float d = x[v][e] - mean; q[v % NS] += d * d; }
        }
      }
      rstd = rsqrtf(wave_sum(q[0]) * inv_n + p.eps);
    } else {     // beyond 2048 columns: the four segment sums of the forward's NW = 4 form
      ln_load_row_stats<XBF16, NS>(RowGeom<1>(blockDim.x), nch, p.x, row * p.ldx, inv_n, p.eps, x, mean, rstd);
    }
    if (lane == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
    const bool ok = !p.mask || p.mask[row];                      // wave-uniform
    if (ok) {
      ++cnt;
#pragma unroll
      for (int v = 0; v < VPL; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[v][e] += (x[v][e] - mean) * rstd * g[v][e] + be[v][e];
    }
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = lane + 64 * v;
    if (c < nch) *reinterpret_cast<f32x4*>(sm + wid * p.cols + 4 * c) = acc[v];
  }
  if (lane == 0) sm[4 * p.cols + wid] = (float)cnt;
  __syncthreads();
  const float n = (sm[4 * p.cols] + sm[4 * p.cols + 1]) + (sm[4 * p.cols + 2] + sm[4 * p.cols + 3]);
  const float inv = n > 0.f ? 1.0f / n : 0.f;
  for (int l = threadIdx.x; l < p.L; l += blockDim.x) {
    const long row = (long)b * p.L + l;
    p.wrow[row] = (!p.mask || p.mask[row]) ? inv : 0.f;          // what the backward multiplies the pooled gradient by
  }
  for (int i = threadIdx.x; i < p.cols; i += blockDim.x) {
    const float a = ((sm[i] + sm[p.cols + i]) + sm[2 * p.cols + i]) + sm[3 * p.cols + i];
    p.pooled[(long)b * p.cols + i] = a * inv;
  }
}

struct LnBwd {
  const void* dy; long lddy;
  const void* x; long ldx;
  const float* gamma; const float* beta; const float* mean; const float* rstd; int act;
  const void* dx_add; float* dx_f32; void* dx_bf16; long lddx;
  float* part;   // [nblocks][2][cols]
  int rows, cols;
  // dropout mask on the bf16 output only: it is the gradient of a Linear's dropped-out output (d(W x) = keep / (1-p) *
  // d(residual sum)), the f32 output stays the residual-path gradient.  Index = row * cols + col.  thr 0 = off.
  unsigned drop_thr, drop_seed; float drop_scale;
  int add_bf16;     // dx_add holds bf16 instead of f32
  // POOL instantiation (LayerNorm followed by a masked mean over the L rows of each sample): dy is the gradient of the
  // POOLED row, f32 [rows / pool_L][cols]; row r receives dy[r / pool_L] * wrow[r] (1 / #valid rows of its sample, or 0:
  // written by ln_pool_fwd_kernel next to mean / rstd, so that the row's scalars are three independent loads)
  const float* wrow; int pool_L;
  const unsigned* drop_epoch;   // common.h drop_seed_eff (last member: the aggregate initialisers below leave it nullptr)
};

// NW = 4 (launch_ln_bwd: f32 dy / x beyond 2048 columns): two barriers per row, none for the partial row.
// The kernel keeps lane / wid / the row walk as locals over RowGeom's static functions, and its preamble and NW = 1 tail are
// ln_load_params and ln_partials_through_lds spelled out: so built, every NW = 1 instantiation is the parent's instruction
// stream.  With a RowGeom object they order their address arithmetic differently; with the two helper calls (four arrays
// passed by reference) the VPL 8 forms allocate up to 275 registers instead of 271 and the VPL 20 forms spill 8 to 24 B more
// per lane (profiles/ln_fold/README.md).
template <int V, int NW, bool DYBF16, bool XBF16, bool ADD16 = false, bool POOL = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwd p) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  using G = RowGeom<NW>;
  const int row0 = G::first_row(blockDim.x), row_step = G::row_step(blockDim.x);
  const int nch = p.cols >> 2;
  f32x4 g[V], b[V], dg[V], db[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = G::chunk(lane, wid, v);
    g[v] = f32x4{0.f, 0.f, 0.f, 0.f}; b[v] = g[v]; dg[v] = g[v]; db[v] = g[v];
    if (c < nch) {
      g[v] = *reinterpret_cast<const f32x4*>(p.gamma + 4 * c);
      if (p.act != CLIPK_ACT_NONE) b[v] = *reinterpret_cast<const f32x4*>(p.beta + 4 * c);
    }
  }
  const float inv_n = 1.0f / (float)p.cols;
  for (int row = row0; row < p.rows; row += row_step) {
    const float mean = p.mean[row], rstd = p.rstd[row];
    f32x4 xh[V], gy[V], addv[V];
    float s1 = 0.f, s2 = 0.f;
    long dyrow = row;
    float pw = 1.f;
    if constexpr (POOL) {
      dyrow = row / p.pool_L;
      pw = p.wrow[row];
    }
    // the residual-path gradient is only needed after the row reductions: issue its load with the others, so the
    // row costs one memory round trip instead of two
    u32x2 addp[V];                              // ADD16: the residual-path gradient stays packed bf16 until it is added
#pragma unroll                                  // (2 instead of 4 registers per chunk: 100 -> 96 VGPRs at VPL 2 = 5 waves / SIMD)
    for (int v = 0; v < V; ++v) {
      const int c = G::chunk(lane, wid, v);
      addv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      addp[v] = u32x2{0u, 0u};
      if constexpr (!POOL) {                    // (the pooled form has no residual-path gradient: 16 registers at VPL 4,
        if (p.dx_add && c < nch) {              //  the difference between 2 and 3 waves per SIMD)
          if constexpr (ADD16)
            addp[v] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(p.dx_add) + (long)row * p.lddx + 4 * c);
          else
            addv[v] = load4<false>(p.dx_add, (long)row * p.lddx + 4 * c);
        }
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c = G::chunk(lane, wid, v);
      xh[v] = f32x4{0.f, 0.f, 0.f, 0.f}; gy[v] = xh[v];
      if (c < nch) {
        const f32x4 xv = load4<XBF16>(p.x, (long)row * p.ldx + 4 * c);
        f32x4 dyv = load4<DYBF16>(p.dy, dyrow * p.lddy + 4 * c);
        if constexpr (POOL) dyv = dyv * pw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xhat = (xv[e] - mean) * rstd;
          if (p.act != CLIPK_ACT_NONE) dyv[e] *= act_grad(xhat * g[v][e] + b[v][e], p.act);
          xh[v][e] = xhat;
          dg[v][e] += dyv[e] * xhat;
          db[v][e] += dyv[e];
          const float gg = dyv[e] * g[v][e];
          gy[v][e] = gg;
          s1 += gg; s2 += gg * xhat;
        }
      }
    }
    float c1 = s1, c2 = s2;
    G::row_means(lane, wid, c1, c2, inv_n);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c = G::chunk(lane, wid, v);
      if (c < nch) {
        f32x4 dx;
#pragma unroll
        for (int e = 0; e < 4; ++e) dx[e] = rstd * (gy[v][e] - c1 - xh[v][e] * c2);
        if constexpr (!POOL) {
          if constexpr (ADD16)
            dx += f32x4{bf16_to_f32((unsigned short)(addp[v][0] & 0xffffu)), bf16_to_f32((unsigned short)(addp[v][0] >> 16)),
                        bf16_to_f32((unsigned short)(addp[v][1] & 0xffffu)), bf16_to_f32((unsigned short)(addp[v][1] >> 16))};
          else
            dx += addv[v];
        }
        if (p.dx_f32) *reinterpret_cast<f32x4*>(p.dx_f32 + (long)row * p.lddx + 4 * c) = dx;
        if (p.dx_bf16) {
          if (p.drop_thr) {
            const unsigned long long base = (unsigned long long)row * (unsigned)p.cols + 4u * c;
            const unsigned dseed = drop_seed_eff(p.drop_seed, p.drop_epoch);
#pragma unroll
            for (int e = 0; e < 4; ++e) dx[e] *= drop_mul(dseed, base + e, p.drop_thr, p.drop_scale);
          }
          store4_bf16(p.dx_bf16, (long)row * p.lddx + 4 * c, dx);
        }
      }
    }
  }
  if constexpr (NW == 4) {
    ln_partials_direct(lane, wid, p.cols, dg, db, p.part);
  } else {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sm = reinterpret_cast<float*>(smem);          // [4][2][cols]
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c = G::chunk(lane, wid, v);
      if (c < nch) {
        *reinterpret_cast<f32x4*>(sm + (wid * 2 + 0) * p.cols + 4 * c) = dg[v];
        *reinterpret_cast<f32x4*>(sm + (wid * 2 + 1) * p.cols + 4 * c) = db[v];
      }
    }
    __syncthreads();
    const int nw = blockDim.x >> 6;
    for (int i = threadIdx.x; i < 2 * p.cols; i += blockDim.x) {
      float a = 0.f;
      for (int w = 0; w < nw; ++w) a += sm[w * 2 * p.cols + i];
      p.part[(long)blockIdx.x * 2 * p.cols + i] = a;
    }
  }
}

// -------------------------------------------------------------------------------------------------
// Backward OF the LayerNorm(+activation) backward (second order).  The ICNN transport map is T(x) = dPsi/dx
// (2_icnn_core.py:181-211, create_graph=True) and its training loss is a function of T, so autograd differentiates
// the first backward  da = r (u - mean u - xh mean(u xh)),  u = dy * act'(n) * gamma,  n = xh gamma + beta,
// xh = (a - mean a) r,  r = rstd(a)  with respect to (dy, a, gamma, beta).  With g the cotangent of da, per row:
//   w  = r (g - mean g - xh mean(g xh))                     (the same projection applied to g)
//   d_dy = w gamma act'(n)
//   q  = w gamma dy act''(n)                                (cotangent of n through act')
//   tt = q gamma - r (u mean(g xh) + g mean(u xh))          (cotangent of xh: through n, and explicit in da)
//   d_a = r (tt - mean tt - xh (mean(tt xh) + mean(g da)))  (through xh and through r)
//   d_gamma += w dy act'(n) + q xh,   d_beta += q           (column sums over the rows)
// One wave per row, the row in registers, two rounds of shuffle reductions; dgamma / dbeta as per-block partial rows
// + the deterministic column reduce of the first-order kernel.
// -------------------------------------------------------------------------------------------------
struct LnBwd2 {
  const float* g; const float* dy; const float* a; long ld;
  const float* gamma; const float* beta; const float* mean; const float* rstd; int act;
  float* d_dy; float* d_a; float* part; int rows, cols;
};

template <int VPL>
__global__ __launch_bounds__(256) void ln_bwd2_kernel(const LnBwd2 p) {
  const RowGeom<1> t(blockDim.x);
  const int nch = p.cols >> 2;
  f32x4 gm[VPL], bt[VPL], dgm[VPL], dbt[VPL];
  ln_load_params(t, nch, p.gamma, p.beta, p.act != CLIPK_ACT_NONE, gm, bt);
#pragma unroll
  for (int v = 0; v < VPL; ++v) { dgm[v] = f32x4{0.f, 0.f, 0.f, 0.f}; dbt[v] = dgm[v]; }
  const float inv_n = 1.0f / (float)p.cols;
  for (int row = t.row0; row < p.rows; row += t.step) {
    const float mean = p.mean[row], r = p.rstd[row];
    f32x4 xh[VPL], gv[VPL], u[VPL], k1[VPL], k2[VPL];      // u = dy act'(n), k1 = act'(n), k2 = gamma dy act''(n)
    float su = 0.f, sux = 0.f, sg = 0.f, sgx = 0.f, sgu = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int c = t.chunk(v);
      xh[v] = f32x4{0.f, 0.f, 0.f, 0.f}; gv[v] = xh[v]; u[v] = xh[v]; k1[v] = xh[v]; k2[v] = xh[v];
      if (c < nch) {
        const long o = (long)row * p.ld + 4 * c;
        const f32x4 av = *reinterpret_cast<const f32x4*>(p.a + o);
        const f32x4 dyv = *reinterpret_cast<const f32x4*>(p.dy + o);
        gv[v] = *reinterpret_cast<const f32x4*>(p.g + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = (av[e] - mean) * r;
          float a1 = 1.f, a2 = 0.f;
          if (p.act != CLIPK_ACT_NONE) {
            const float n = x * gm[v][e] + bt[v][e];
            a1 = act_grad(n, p.act);
            a2 = act_grad2(n, p.act);
          }
          xh[v][e] = x;
          k1[v][e] = a1;
          k2[v][e] = gm[v][e] * dyv[e] * a2;
          const float ud = dyv[e] * a1;                     // dy act'(n): d_gamma's first term pairs it with w
          u[v][e] = ud;
          const float ug = ud * gm[v][e];                   // the first backward's u
          su += ug; sux += ug * x; sg += gv[v][e]; sgx += gv[v][e] * x; sgu += gv[v][e] * ug;
        }
      }
    }
    const float mu = wave_sum(su) * inv_n, cux = wave_sum(sux) * inv_n, mg = wave_sum(sg) * inv_n,
                dgx = wave_sum(sgx) * inv_n, mgu = wave_sum(sgu) * inv_n;
    const float e_gda = r * (mgu - mg * mu - dgx * cux);   // mean(g da)
    f32x4 tt[VPL], w[VPL];
    float st = 0.f, stx = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int c = t.chunk(v);
      tt[v] = f32x4{0.f, 0.f, 0.f, 0.f}; w[v] = tt[v];
      if (c < nch) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = xh[v][e];
          const float ww = r * (gv[v][e] - mg - x * dgx);
          w[v][e] = ww;
          const float q = ww * k2[v][e];                   // w gamma dy act''(n)
          const float ug = u[v][e] * gm[v][e];              // u with gamma
          const float tv = q * gm[v][e] - r * (ug * dgx + gv[v][e] * cux);
          tt[v][e] = tv;
          st += tv; stx += tv * x;
          dgm[v][e] += ww * u[v][e] + q * x;
          dbt[v][e] += q;
        }
      }
    }
    const float mt = wave_sum(st) * inv_n, mtx = wave_sum(stx) * inv_n;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int c = t.chunk(v);
      if (c < nch) {
        const long o = (long)row * p.ld + 4 * c;
        f32x4 ddy, da;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ddy[e] = w[v][e] * gm[v][e] * k1[v][e];
          da[e] = r * (tt[v][e] - mt - xh[v][e] * (mtx + e_gda));
        }
        if (p.d_dy) *reinterpret_cast<f32x4*>(p.d_dy + o) = ddy;
        if (p.d_a) *reinterpret_cast<f32x4*>(p.d_a + o) = da;
      }
    }
  }
  ln_partials_through_lds(t, p.cols, dgm, dbt, p.part);
}

// part: [nparts][ncols] with ncols = 2*cols ([dgamma | dbeta]).  Block = 16 columns x 16 row groups: a thread sums
// every 16th partial row with 8 independent loads in flight (the old 64 x 4 shape ran 15 blocks of 256-deep
// dependent chains: 33 us for a 4 MB input), LDS combines the 16 groups in a fixed order (deterministic).
__device__ __forceinline__ void colreduce_block(const float* part, int nparts, int ncols, float* out0, float* out1,
                                                int cols, int accumulate) {
  __shared__ float sm[16][17];
  const int c = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + c;
  float a = 0.f;
  if (i < ncols) {
    int s = rg;
    for (; s + 7 * 16 < nparts; s += 8 * 16) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(long)(s + 16 * u) * ncols + i];
      a += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; s < nparts; s += 16) a += part[(long)s * ncols + i];
  }
  sm[rg][c] = a;
  __syncthreads();
  if (rg == 0 && i < ncols) {
    a = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) a += sm[r][c];
    float* o = (i < cols) ? (out0 ? out0 + i : nullptr) : (out1 ? out1 + (i - cols) : nullptr);
    if (o) *o = accumulate ? (*o + a) : a;
  }
}

__global__ __launch_bounds__(256) void colreduce_kernel(const float* part, int nparts, int ncols, float* out0,
                                                        float* out1, int cols, int accumulate) {
  colreduce_block(part, nparts, ncols, out0, out1, cols, accumulate);
}

// Several column reduces in ONE launch (blockIdx.y = problem): the dgamma / dbeta partial rows of every LayerNorm whose
// backward ran in this pass, reduced when the pass is over (functional.LayerNormFn defers them: one launch instead of one
// per LayerNorm - 20 per step of the sliced notebook model, each a 4-us launch on the critical chain).  desc: 6 int64 per
// problem {part, nparts, cols, out0 (dgamma), out1 (dbeta), accumulate}.
__global__ __launch_bounds__(256) void colreduce_batched_kernel(const long long* desc) {
  const long long* d = desc + 6 * (long)blockIdx.y;
  const int cols = (int)d[2];
  if ((int)blockIdx.x * 16 >= 2 * cols) return;              // (block-uniform)
  colreduce_block(reinterpret_cast<const float*>(d[0]), (int)d[1], 2 * cols, reinterpret_cast<float*>(d[3]),
                  reinterpret_cast<float*>(d[4]), cols, (int)d[5]);
}

// ---- L2 normalise -------------------------------------------------------------------------------
template <int VPL>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* x, float* y, float* norm, int rows, int cols,
                                                         float eps) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const int nch = cols >> 2;
  f32x4 xv[VPL];
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = lane + 64 * v;
    xv[v] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < nch) xv[v] = *reinterpret_cast<const f32x4*>(x + (long)row * cols + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += xv[v][e] * xv[v][e];
  }
  const float n = sqrtf(wave_sum(s));
  const float inv = 1.0f / fmaxf(n, eps);
  if (lane == 0 && norm) norm[row] = n;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = lane + 64 * v;
    if (c < nch) *reinterpret_cast<f32x4*>(y + (long)row * cols + 4 * c) = xv[v] * inv;
  }
}

template <int VPL>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* dy, const float* y, const float* norm, float* dx,
                                                         int rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const int nch = cols >> 2;
  f32x4 yv[VPL], dv[VPL];
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = lane + 64 * v;
    yv[v] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[v] = yv[v];
    if (c < nch) {
      yv[v] = *reinterpret_cast<const f32x4*>(y + (long)row * cols + 4 * c);
      dv[v] = *reinterpret_cast<const f32x4*>(dy + (long)row * cols + 4 * c);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s += yv[v][e] * dv[v][e];
  }
  const float dot = wave_sum(s);
  const float n = norm[row];
  // y = x / max(n, eps): for n >= eps, dx = (dy - y*(y.dy)) / n ; below eps the clamp is constant: dx = dy/eps
  const bool clamped = n < eps;
  const float inv = 1.0f / fmaxf(n, eps);
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = lane + 64 * v;
    if (c < nch) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = clamped ? dv[v][e] * inv : (dv[v][e] - yv[v][e] * dot) * inv;
      *reinterpret_cast<f32x4*>(dx + (long)row * cols + 4 * c) = o;
    }
  }
}

// one wave per row, 4 waves per block.  These kernels are pure HBM streams: they need ~72 KiB in flight per CU
// (MI355X_MICROARCH.md) and a 480-wide f32 row is 1.9 KiB, i.e. >= 32 resident waves per CU.  The backward also
// writes one [2][cols] partial row per block for dgamma / dbeta, hence its smaller cap.
int ln_blocks_cap(int rows, int cap) {
  int b = (rows + 3) / 4;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return b;
}
// backward: as many blocks as are resident at once (96 VGPRs at VPL 2 = 5 waves per SIMD, ~160 at VPL 4 = 3), never a
// second round
int ln_blocks(int rows, int cols) { return ln_blocks_cap(rows, cols <= 512 ? 1280 : (cols <= 1024 ? 768 : 512)); }
int ln_blocks_fwd(int rows) { return ln_blocks_cap(rows, 2048); }
size_t ln_partials_lds(int cols) { return (size_t)4 * 2 * cols * sizeof(float); }   // ln_partials_through_lds

template <class P>
void ln_launch(void (*kernel)(const P), int blocks, size_t lds, hipStream_t st, const P& p) {
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, st, p);
}

// VPL 20 is the width of the workgroup-per-row form: five chunks in each of four waves, one block per row up to 2048
template <int V, bool XBF16>
void launch_ln_fwd(const LnFwd& p, hipStream_t st) {
  constexpr int NW = ln_fwd_row_waves(V);
  const int blocks = NW == 1 ? ln_blocks_fwd(p.rows) : (p.rows < 2048 ? p.rows : 2048);
  ln_launch(ln_fwd_kernel<V / NW, NW, XBF16>, blocks, 0, st, p);
}

// ... and of the backward where dy and x are both f32 (with ln_blocks' grid: `blocks` partial rows either way); a bf16
// stream or the pooled form keeps a wave per row at VPL 20
template <int V, bool DYBF16, bool XBF16, bool ADD16 = false, bool POOL = false>
void launch_ln_bwd(const LnBwd& p, int blocks, hipStream_t st) {
  if constexpr (V == 20 && !DYBF16 && !XBF16 && !POOL)
    ln_launch(ln_bwd_kernel<5, 4, false, false>, blocks, 0, st, p);
  else
    ln_launch(ln_bwd_kernel<V, 1, DYBF16, XBF16, ADD16, POOL>, blocks, ln_partials_lds(p.cols), st, p);
}

template <int V>
int launch_ln_bwd2(const LnBwd2& p, int blocks, hipStream_t st) {
  if constexpr (V > 8) return CLIPK_ERR_UNSUPPORTED;        // (eleven chunk arrays per lane: no form beyond 2048 columns)
  else {
    ln_launch(ln_bwd2_kernel<V>, blocks, ln_partials_lds(p.cols), st, p);
    return CLIPK_OK;
  }
}

int launch_colreduce(const void* part, int nparts, int cols, float* dgamma, float* dbeta, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(colreduce_kernel, dim3((2 * cols + 15) / 16), dim3(256), 0, st, (const float*)part, nparts, 2 * cols,
                     dgamma, dbeta, cols, accumulate);
  return clipk_check_launch();
}

}  // namespace

#define LN_DISPATCH_VPL(cols, CALL)                      \
  do {                                                   \
    const int nch_ = (cols) >> 2;                        \
    if (nch_ <= 64 * 2) { CALL(2); }                     \
    else if (nch_ <= 64 * 4) { CALL(4); }                \
    else if (nch_ <= 64 * 8) { CALL(8); }                \
    else if (nch_ <= 64 * 20) { CALL(20); }              \
    else return CLIPK_ERR_UNSUPPORTED;                   \
  } while (0)

extern "C" int clipk_layernorm_fwd(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta,
                                   float eps, int act, float* y_f32, void* y_bf16, int64_t ldy,
                                   float* mean, float* rstd, int rows, int cols, void* stream) {
  if (!x || !gamma || !beta || rows <= 0 || cols <= 0 || (!y_f32 && !y_bf16)) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || (ldx & 3) || (ldy & 3)) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(gamma) || !aligned16(beta)) return CLIPK_ERR_BAD_ARG;
  LnFwd p{x, (long)ldx, gamma, beta, eps, act, y_f32, y_bf16, (long)ldy, mean, rstd, rows, cols};
  hipStream_t st = (hipStream_t)stream;
#define CALL(V)                                                    \
  if (x_dtype == CLIPK_BF16) launch_ln_fwd<V, true>(p, st);        \
  else launch_ln_fwd<V, false>(p, st)
  LN_DISPATCH_VPL(cols, CALL);
#undef CALL
  return clipk_check_launch();
}

extern "C" size_t clipk_layernorm_bwd_workspace(int rows, int cols) {
  return (size_t)ln_blocks(rows, cols) * 2 * cols * sizeof(float);
}

extern "C" int clipk_layernorm_bwd(const void* dy, int dy_dtype, int64_t lddy, const void* x, int x_dtype, int64_t ldx,
                                   const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                                   const void* dx_add, int dx_add_dtype, float* dx_f32, void* dx_bf16, int64_t lddx,
                                   float* dgamma, float* dbeta, int accumulate,
                                   int rows, int cols, float drop_p, uint32_t drop_seed,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!dy || !x || !gamma || !mean || !rstd || rows <= 0 || cols <= 0 || !workspace) return CLIPK_ERR_BAD_ARG;
  if (act != CLIPK_ACT_NONE && !beta) return CLIPK_ERR_BAD_ARG;
  if (!(drop_p >= 0.f) || drop_p >= 1.f) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || (ldx & 3) || (lddy & 3) || (lddx & 3)) return CLIPK_ERR_UNSUPPORTED;
  if (dx_add && dx_add_dtype == CLIPK_BF16 && !(dy_dtype == CLIPK_BF16 && x_dtype == CLIPK_F32)) return CLIPK_ERR_UNSUPPORTED;
  const int blocks = ln_blocks(rows, cols);
  if (workspace_bytes < (size_t)blocks * 2 * cols * sizeof(float)) return CLIPK_ERR_BAD_ARG;
  const DropParams drop = drop_params(drop_p);
  LnBwd p{dy, (long)lddy, x, (long)ldx, gamma, beta, mean, rstd, act, dx_add, dx_f32, dx_bf16, (long)lddx,
          (float*)workspace, rows, cols, drop.thr, drop_seed, drop.scale, (dx_add && dx_add_dtype == CLIPK_BF16) ? 1 : 0,
          nullptr, 1};
  p.drop_epoch = clipk_drop_epoch();
  hipStream_t st = (hipStream_t)stream;
#define CALL(V)                                                                                                   \
  do {                                                                                                            \
    if (p.add_bf16)                             /* bf16 gradient stream: bf16 dy, f32 x (checked above) */       \
      launch_ln_bwd<V, true, false, true>(p, blocks, st);                                                         \
    else if (dy_dtype == CLIPK_BF16 && x_dtype == CLIPK_BF16)                                                     \
      launch_ln_bwd<V, true, true>(p, blocks, st);                                                                \
    else if (dy_dtype == CLIPK_BF16)                                                                              \
      launch_ln_bwd<V, true, false>(p, blocks, st);                                                               \
    else if (x_dtype == CLIPK_BF16)                                                                               \
      launch_ln_bwd<V, false, true>(p, blocks, st);                                                               \
    else                                                                                                          \
      launch_ln_bwd<V, false, false>(p, blocks, st);                                                              \
  } while (0)
  LN_DISPATCH_VPL(cols, CALL);
#undef CALL
  const int rc = clipk_check_launch();
  if (rc || !(dgamma || dbeta)) return rc;
  return launch_colreduce(workspace, blocks, cols, dgamma, dbeta, accumulate, st);
}

// out[c] (+)= sum over rows of x[r][c]: the bias gradient of an exact-f32 Linear (db = dY.sum(0)), fixed summation order
extern "C" int clipk_colsum_f32(const float* x, int rows, int cols, float* out, int accumulate, void* stream) {
  if (!x || !out || rows <= 0 || cols <= 0) return CLIPK_ERR_BAD_ARG;
  hipLaunchKernelGGL(colreduce_kernel, dim3((cols + 15) / 16), dim3(256), 0, (hipStream_t)stream, x, rows, cols, out,
                     (float*)nullptr, cols, accumulate);
  return clipk_check_launch();
}

// The deferred form of clipk_layernorm_bwd's parameter gradients: call it with dgamma = dbeta = NULL and a workspace of your
// own per LayerNorm (it keeps the [blocks][2][cols] partial rows, blocks = workspace bytes / (2 cols 4)), then reduce all of
// them here in one launch.  desc_dev: n x 6 int64 in device memory {partial rows, blocks, cols, dgamma, dbeta, accumulate}.
extern "C" int clipk_colreduce_batched(const int64_t* desc_dev, int n, int max_cols, void* stream) {
  if (!desc_dev || n <= 0 || max_cols <= 0 || n > 65535) return CLIPK_ERR_BAD_ARG;
  hipLaunchKernelGGL(colreduce_batched_kernel, dim3((2 * max_cols + 15) / 16, n), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(desc_dev));
  return clipk_check_launch();
}

// Second-order LayerNorm(+activation) backward (see ln_bwd2_kernel): f32 only, [rows, cols] row-major with one leading
// dimension.  workspace: clipk_layernorm_bwd_workspace(rows, cols) bytes.  d_gamma / d_beta are overwritten
// (accumulate = 0) or added to (accumulate = 1); either both or neither.
extern "C" int clipk_layernorm_bwd2(const float* g, const float* dy, const float* a, int64_t ld, const float* gamma,
                                    const float* beta, const float* mean, const float* rstd, int act, float* d_dy,
                                    float* d_a, float* d_gamma, float* d_beta, int accumulate, int rows, int cols,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!g || !dy || !a || !gamma || !mean || !rstd || rows <= 0 || cols <= 0 || !workspace) return CLIPK_ERR_BAD_ARG;
  if (act != CLIPK_ACT_NONE && !beta) return CLIPK_ERR_BAD_ARG;
  if (act != CLIPK_ACT_NONE && act != CLIPK_ACT_CELU && act != CLIPK_ACT_SOFTPLUS) return CLIPK_ERR_UNSUPPORTED;
  if ((d_gamma == nullptr) != (d_beta == nullptr)) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || (ld & 3)) return CLIPK_ERR_UNSUPPORTED;
  const int blocks = ln_blocks_cap(rows, 512);
  if (workspace_bytes < (size_t)blocks * 2 * cols * sizeof(float)) return CLIPK_ERR_BAD_ARG;
  LnBwd2 p{g, dy, a, (long)ld, gamma, beta, mean, rstd, act, d_dy, d_a, (float*)workspace, rows, cols};
  hipStream_t st = (hipStream_t)stream;
#define CALL(V) \
  if (const int rc = launch_ln_bwd2<V>(p, blocks, st)) return rc
  LN_DISPATCH_VPL(cols, CALL);
#undef CALL
  if (d_gamma) return launch_colreduce(workspace, blocks, cols, d_gamma, d_beta, accumulate, st);
  return clipk_check_launch();
}

extern "C" int clipk_layernorm_meanpool_fwd(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta, float eps,
                                           const uint8_t* mask, int B, int L, int cols, float* pooled, float* mean,
                                           float* rstd, float* row_weight, void* stream) {
  if (!x || !gamma || !beta || !pooled || !mean || !rstd || !row_weight || B <= 0 || L <= 0 || cols <= 0) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || (ldx & 3)) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta)) return CLIPK_ERR_BAD_ARG;
  LnPool p{x, (long)ldx, gamma, beta, eps, mask, pooled, mean, rstd, row_weight, L, cols};
  const size_t lds = ((size_t)4 * cols + 4) * sizeof(float);
  if (lds > 65536) return CLIPK_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
#define CALL(V)                                                                      \
  if (x_dtype == CLIPK_BF16) ln_launch(ln_pool_fwd_kernel<V, true>, B, lds, st, p);  \
  else ln_launch(ln_pool_fwd_kernel<V, false>, B, lds, st, p)
  LN_DISPATCH_VPL(cols, CALL);
#undef CALL
  return clipk_check_launch();
}

extern "C" int clipk_layernorm_meanpool_bwd(const float* dpooled, const float* row_weight, int B, int L,
                                           const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* mean,
                                           const float* rstd, float* dx_f32, void* dx_bf16, int64_t lddx, float* dgamma,
                                           float* dbeta, int accumulate, int cols, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  if (!dpooled || !row_weight || !x || !gamma || !mean || !rstd || B <= 0 || L <= 0 || cols <= 0 || !workspace)
    return CLIPK_ERR_BAD_ARG;
  if (!dx_f32 && !dx_bf16) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || (ldx & 3) || (lddx & 3)) return CLIPK_ERR_UNSUPPORTED;
  const long rows_l = (long)B * L;
  if (rows_l > 0x7fffffffL) return CLIPK_ERR_UNSUPPORTED;
  const int rows = (int)rows_l;
  const int blocks = ln_blocks(rows, cols);
  if (workspace_bytes < (size_t)blocks * 2 * cols * sizeof(float)) return CLIPK_ERR_BAD_ARG;
  LnBwd p{dpooled, (long)cols, x, (long)ldx, gamma, nullptr, mean, rstd, CLIPK_ACT_NONE, nullptr, dx_f32, dx_bf16,
          (long)lddx, (float*)workspace, rows, cols, 0u, 0u, 1.0f, 0, row_weight, L};
  hipStream_t st = (hipStream_t)stream;
#define CALL(V)                                                                          \
  if (x_dtype == CLIPK_BF16) launch_ln_bwd<V, false, true, false, true>(p, blocks, st);  \
  else launch_ln_bwd<V, false, false, false, true>(p, blocks, st)
  LN_DISPATCH_VPL(cols, CALL);
#undef CALL
  const int rc = clipk_check_launch();
  if (rc || !(dgamma || dbeta)) return rc;
  return launch_colreduce(workspace, blocks, cols, dgamma, dbeta, accumulate, st);
}

extern "C" int clipk_l2norm_fwd(const float* x, float* y, float* norm, int rows, int cols, float eps, void* stream) {
  if (!x || !y || rows <= 0 || cols <= 0) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || cols > 64 * 4 * 8) return CLIPK_ERR_UNSUPPORTED;
  const int blocks = (rows + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  if (cols <= 512) hipLaunchKernelGGL((l2norm_fwd_kernel<2>), dim3(blocks), dim3(256), 0, st, x, y, norm, rows, cols, eps);
  else hipLaunchKernelGGL((l2norm_fwd_kernel<8>), dim3(blocks), dim3(256), 0, st, x, y, norm, rows, cols, eps);
  return clipk_check_launch();
}

extern "C" int clipk_l2norm_bwd(const float* dy, const float* y, const float* norm, float* dx,
                                int rows, int cols, float eps, void* stream) {
  if (!dy || !y || !norm || !dx || rows <= 0 || cols <= 0) return CLIPK_ERR_BAD_ARG;
  if ((cols & 3) || cols > 64 * 4 * 8) return CLIPK_ERR_UNSUPPORTED;
  const int blocks = (rows + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  if (cols <= 512) hipLaunchKernelGGL((l2norm_bwd_kernel<2>), dim3(blocks), dim3(256), 0, st, dy, y, norm, dx, rows, cols, eps);
  else hipLaunchKernelGGL((l2norm_bwd_kernel<8>), dim3(blocks), dim3(256), 0, st, dy, y, norm, dx, rows, cols, eps);
  return clipk_check_launch();
}
