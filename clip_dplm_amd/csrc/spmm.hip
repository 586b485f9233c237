// spmm.hip — clipk_csr_spmm_f64: a CSR matrix with an optional symmetric diagonal scaling applied to a block of f64
// vectors, with a two-term epilogue (include/clipk.h has the contract and the arithmetic, which a numpy restatement
// reproduces bit for bit):
//   Y[i, :] = alpha * s_i * sum_{e in row i} (w_e * s_{col_e}) * X[col_e, :]  +  beta * B[i, :]  +  gamma * C[i, :]
// It is the operator of diffusion.diffusion_map (T = S W S, never materialised), one Chebyshev three-term step, or a
// Lanczos step, a few hundred times per solve.
//
// Shape of the work.  The kernel is a row gather: per entry 4 + 8 (+ 8 with s) bytes of the matrix and one m * 8-byte row
// of X from wherever it sits (L2 / Infinity Cache for the clouds this is for: 2^20 rows of 32 columns are 268 MB).  A group
// of G lanes owns one (row, chunk) item, a lane V = 1 or 2 adjacent columns (V = 2 - 16-byte loads - when m is even and
// every operand is 16-byte aligned; G = the power of two >= m / V), so a wave holds 64 / G items and keeps four gathered
// rows per item in flight.  Results do not depend on V or G.
//
// Row-length skew.  Rows of a symmetrised kNN graph have k + in-degree entries and hubs exist; a group would run as long
// as its longest row.  A row's entries are therefore cut into chunks of CLIPK_SPMM_CHUNK: chunk 0 is summed by the row's
// own group, every further chunk by a group of a first launch that leaves its partial sum in the workspace, and the row's
// group adds the partials in chunk order.  No scan and no host read is needed to find the further chunks: the starts of
// two of them are more than CHUNK entries apart (in one row exactly CHUNK; in two rows the later one lies at least CHUNK
// beyond its own row's start), so each aligned block [j CHUNK, (j + 1) CHUNK) of the entry array holds at most one start,
// and it belongs to the row that holds entry j CHUNK.  Slot j finds that row by bisection of indptr and owns partial j.
//
// CHUNK = 64 and four rows in flight are measured choices (profiles/diffusion/): a group walks its chunk as a chain of
// CHUNK / 4 dependent round trips (index, then s[col] and the row), and that chain of the longest item is the floor of a
// launch.  At 65536 rows (hub rows of 1292 entries) chunks of 256 took 1.76x the time of chunks of 64 at m = 32; at 2^20
// rows, where the gathered bytes decide, the chunk size moves the time by 2 - 7 %.  Eight rows in flight lose at m = 32.
#include "common.h"

namespace {

constexpr int CHUNK = CLIPK_SPMM_CHUNK;
constexpr int U = 4;                                  // gathered rows in flight per item
constexpr int THREADS = 256;
typedef double f64x2 __attribute__((ext_vector_type(2)));

// one rounding each (the __dmul_rn / __dadd_rn of the contract), never contracted into an fma: the header's own
// __dmul_rn is compiled with contraction allowed and fused with the add that follows it (seen in the ISA), so the
// products and sums are written here, under the pragma, for the whole file
#pragma clang fp contract(off)
__device__ __forceinline__ double dmul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double dadd(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

struct SpmmArgs {
  const int64_t* indptr;
  const int32_t* indices;
  const double* w;
  const double* s;
  const double* X;
  const double* B;
  const double* C;
  double* Y;
  double* part;        // [slots][m]
  int N, m, gshift;    // G = 1 << gshift
  long nnz;
  double alpha, beta, gamma;
};

template <int V>
__device__ __forceinline__ void load_cols(const double* p, double (&v)[V]) {
  if constexpr (V == 2) {
    const f64x2 t = *reinterpret_cast<const f64x2*>(p);
    v[0] = t[0]; v[1] = t[1];
  } else {
    v[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void store_cols(double* p, const double (&v)[V]) {
  if constexpr (V == 2) *reinterpret_cast<f64x2*>(p) = f64x2{v[0], v[1]};
  else p[0] = v[0];
}

__device__ __forceinline__ long clamp_e(long e, long nnz) { return e < 0 ? 0 : (e > nnz ? nnz : e); }

// acc[v] = the chunk's sum over e0 <= e < e1 in ascending e of fl(coef_e * X[col_e, c + v]), from +0
template <int V>
__device__ __forceinline__ void chunk_sum(const SpmmArgs& a, long e0, long e1, int c, double (&acc)[V]) {
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.0;
  long e = e0;
  for (; e + U <= e1; e += U) {                       // U gathered rows in flight, added in order
    int j[U];
    bool ok[U];
    double cf[U], x[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      j[u] = a.indices[e + u];
      ok[u] = (unsigned)j[u] < (unsigned)a.N;
      if (!ok[u]) j[u] = 0;
      cf[u] = a.w[e + u];
    }
    if (a.s) {
#pragma unroll
      for (int u = 0; u < U; ++u) cf[u] = dmul(cf[u], a.s[j[u]]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) load_cols<V>(a.X + (long)j[u] * a.m + c, x[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (ok[u]) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = dadd(acc[v], dmul(cf[u], x[u][v]));
      }
    }
  }
  for (; e < e1; ++e) {
    const int j = a.indices[e];
    if ((unsigned)j >= (unsigned)a.N) continue;
    double cf = a.w[e], x[V];
    if (a.s) cf = dmul(cf, a.s[j]);
    load_cols<V>(a.X + (long)j * a.m + c, x);
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = dadd(acc[v], dmul(cf, x[v]));
  }
}

// slot j: the one chunk q >= 1 of some row that starts inside [j CHUNK, (j + 1) CHUNK), if there is one
template <int V>
__global__ __launch_bounds__(THREADS) void spmm_chunks_kernel(SpmmArgs a, long slots) {
  const long slot = ((long)blockIdx.x * THREADS + threadIdx.x) >> a.gshift;
  const int c = (threadIdx.x & ((1 << a.gshift) - 1)) * V;
  if (slot >= slots || c >= a.m) return;
  const long E = slot * CHUNK;
  int lo = 0, hi = a.N - 1;                            // the largest r with indptr[r] <= E: the row that holds entry E
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (a.indptr[mid] <= E) lo = mid; else hi = mid - 1;
  }
  const long r0 = clamp_e(a.indptr[lo], a.nnz), r1 = clamp_e(a.indptr[lo + 1], a.nnz);
  const long off = E - r0;
  if (off <= 0) return;                                // E is the row's first entry: chunk 0, the row kernel's
  const long start = r0 + (off + CHUNK - 1) / CHUNK * CHUNK;
  if (start >= r1) return;
  double acc[V];
  chunk_sum<V>(a, start, start + CHUNK < r1 ? start + CHUNK : r1, c, acc);
  store_cols<V>(a.part + slot * a.m + c, acc);
}

template <int V>
__global__ __launch_bounds__(THREADS) void spmm_rows_kernel(SpmmArgs a) {
  const long row = ((long)blockIdx.x * THREADS + threadIdx.x) >> a.gshift;
  const int c = (threadIdx.x & ((1 << a.gshift) - 1)) * V;
  if (row >= a.N || c >= a.m) return;
  const long r0 = clamp_e(a.indptr[row], a.nnz), r1 = clamp_e(a.indptr[row + 1], a.nnz);
  double t[V];
  chunk_sum<V>(a, r0, r0 + CHUNK < r1 ? r0 + CHUNK : r1, c, t);
  for (long start = r0 + CHUNK; start < r1; start += CHUNK) {      // partials in chunk order
    double p[V];
    load_cols<V>(a.part + start / CHUNK * a.m + c, p);
#pragma unroll
    for (int v = 0; v < V; ++v) t[v] = dadd(t[v], p[v]);
  }
  const long o = row * a.m + c;
  double y[V], b[V], cc[V];
  const double si = a.s ? a.s[row] : 1.0;
  if (a.B) load_cols<V>(a.B + o, b);
  if (a.C) load_cols<V>(a.C + o, cc);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    y[v] = dmul(a.alpha, a.s ? dmul(si, t[v]) : t[v]);
    if (a.B) y[v] = dadd(y[v], dmul(a.beta, b[v]));
    if (a.C) y[v] = dadd(y[v], dmul(a.gamma, cc[v]));
  }
  store_cols<V>(a.Y + o, y);
}

inline long spmm_slots(long nnz) { return nnz > CHUNK ? (nnz + CHUNK - 1) / CHUNK : 0; }

inline bool overlap(const double* p, const double* q, long n) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q, len = (uintptr_t)n * sizeof(double);
  return a < b + len && b < a + len;
}

}  // namespace

extern "C" size_t clipk_csr_spmm_workspace(long long nnz, int m) {
  if (nnz < 0 || m < 1 || m > CLIPK_SPMM_MAX_M) return 0;
  return (size_t)spmm_slots(nnz) * m * sizeof(double);
}

extern "C" int clipk_csr_spmm_f64(const int64_t* indptr, const int32_t* indices, const double* w, const double* s, int N,
                                  long long nnz, int m, const double* X, double alpha, const double* B, double beta,
                                  const double* C, double gamma, double* Y, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (!indptr || !X || !Y || N <= 0 || nnz < 0 || m < 1) return CLIPK_ERR_BAD_ARG;
  if (nnz > 0 && (!indices || !w)) return CLIPK_ERR_BAD_ARG;
  if (m > CLIPK_SPMM_MAX_M) return CLIPK_ERR_UNSUPPORTED;
  if (overlap(X, Y, (long)N * m)) return CLIPK_ERR_BAD_ARG;
  const long slots = spmm_slots(nnz);
  if (slots && (!workspace || workspace_bytes < (size_t)slots * m * sizeof(double))) return CLIPK_ERR_BAD_ARG;
  const bool v2 = m % 2 == 0 && aligned16(X) && aligned16(Y) && (!B || aligned16(B)) && (!C || aligned16(C)) &&
                  (!slots || aligned16(workspace));
  const int cols = v2 ? m / 2 : m;
  int gshift = 0;
  while ((1 << gshift) < cols) ++gshift;
  SpmmArgs a{indptr, indices, w, s, X, B, C, Y, (double*)workspace, N, m, gshift, (long)nnz, alpha, beta, gamma};
  const int per_block = THREADS >> gshift;
  if (slots) {
    const long blocks = (slots + per_block - 1) / per_block;
    if (blocks > INT32_MAX) return CLIPK_ERR_UNSUPPORTED;
    if (v2) hipLaunchKernelGGL(spmm_chunks_kernel<2>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a, slots);
    else hipLaunchKernelGGL(spmm_chunks_kernel<1>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a, slots);
  }
  const long blocks = ((long)N + per_block - 1) / per_block;
  if (v2) hipLaunchKernelGGL(spmm_rows_kernel<2>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(spmm_rows_kernel<1>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  return clipk_check_launch();
}
