// graph_labels.hip — clipk_knn_label_pairs: the edges of a kNN graph counted by (label of the row, label of the
// neighbour), the G x G table behind PAGA's cluster graph and a kNN label-transfer confusion matrix (include/clipk.h has
// the contract):
//   counts[a, b] += #{(i, t) : row_labels[i] = a, 0 <= idx[i, t] < Ny, key_labels[idx[i, t]] = b}      a, b in [0, G)
//
// Shape of the work.  A histogram over M k entries: 8 bytes of index per entry streamed once, a 4-byte gather of the
// neighbour's label (the label vector is 4 Ny bytes and stays in cache) and the row's own label, which the lanes of
// a wave share.  What decides the time besides the stream is where the adds go: most neighbours of a row carry its own
// label, so the G diagonal words take most of the adds, and one global word takes only some 88 atomics per microsecond.
//
// Both kernels walk the flat entry array e = i k + t with consecutive lanes on consecutive entries (coalesced 8-byte
// loads), a workgroup over the entries of a contiguous range of rows, U strides of the workgroup in flight.  A lane
// carries the row of its entry along (THREADS / k rows and THREADS % k columns further each stride): no division in
// the loop.
//
// G <= 128 (lds kernel).  The workgroup keeps the whole table as int32 bins in LDS (4 G^2 bytes, 64 KB at G = 128: two
// workgroups of 512 threads per CU), adds with LDS atomics and, at the end, adds its non-zero bins to counts with
// 64-bit global atomics: G^2 global atomics per workgroup at the most, whatever M k.  Before the LDS add a wave merges
// the lanes that hold the key of its first valid lane - with clustered labels that is most of them - into one add of
// their number; the other lanes add 1 each.
// BOUND: a workgroup's range holds at most 2^31 - 1 entries (its rows are capped at floor((2^31 - 1) / k)), so no int32
// bin can pass 2^31 - 1 before it is flushed.
//
// G > 128 (wave kernel).  No table.  A wave takes the key of its first lane that still has one, ballots the lanes that
// hold it, one lane adds their number to counts with one 64-bit global atomic, and the round repeats with the lanes
// that are left: one atomic per distinct key of the wave, a few rounds with clustered labels and up to 64 with random
// ones.  The key of each stride's FIRST round is not added at once but carried (key, number) into the next stride and
// added when another key takes its place: a run of strides with one dominant key - the diagonal of the cluster the
// rows belong to - costs the diagonal word one atomic, not one per stride.
//
// Every add is an integer add, so the table is exact and independent of the grid, of the order of the atomics and of the
// kernel that ran.  No value is written except by atomics (LDS and global) and the zeroing of the LDS bins.
#include "common.h"

namespace {

constexpr int U = 4;                                   // strides of the workgroup in flight
constexpr int LDS_THREADS = 512, WAVE_THREADS = 256;
constexpr int LDS_MAX_G = 128;                         // 4 G^2 <= 64 KB

struct PairArgs {
  const int64_t* idx;
  const int32_t* row_labels;
  const int32_t* key_labels;
  long long* counts;
  long M, Ny, rows_per;                                // rows_per: rows of one workgroup
  int k, G;
};

__device__ __forceinline__ void add64(long long* p, long long n) {
  (void)__hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// U strides of the workgroup from entry `base` on: the indices and the row labels first, then the gathers, then the adds.
// FULL: all U strides lie inside the workgroup's range and every load is unconditional, so the compiler issues them back
// to back; the last, partial group predicates each entry.  An entry that counts nowhere gathers key_labels[0] and drops it.
template <int THREADS, bool FULL, typename Sink>
__device__ __forceinline__ void strides(const PairArgs& p, long base, long e1, long& row, int& t, int dr, int dt,
                                        Sink&& sink) {
  long j[U];
  int a[U], b[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long e = base + (long)u * THREADS + threadIdx.x;
    const bool in = FULL || e < e1;                    // then row < r1 <= M
    j[u] = in ? p.idx[e] : -1;
    a[u] = in ? p.row_labels[row] : -1;
    row += dr;
    t += dt;
    if (t >= p.k) { t -= p.k; ++row; }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = (unsigned)a[u] < (unsigned)p.G && (unsigned long)j[u] < (unsigned long)p.Ny;
    if (!ok) a[u] = -1;
    b[u] = p.key_labels[ok ? j[u] : 0];                // Ny >= 1
  }
#pragma unroll
  for (int u = 0; u < U; ++u) sink(a[u] >= 0 && (unsigned)b[u] < (unsigned)p.G ? a[u] * p.G + b[u] : -1);
}

// The walk of one workgroup: sink(key) is called by every lane of every wave, the same number of times in all of them,
// with key = a G + b of the lane's entry or -1 (no entry left, or one that counts nowhere).
template <int THREADS, typename Sink>
__device__ __forceinline__ void walk(const PairArgs& p, Sink&& sink) {
  const long r0 = (long)blockIdx.x * p.rows_per;
  const long r1 = r0 + p.rows_per < p.M ? r0 + p.rows_per : p.M;
  const long e1 = r1 * p.k;
  const int tid = threadIdx.x;
  long row = r0 + tid / p.k;                           // the row and the column of entry base + tid
  int t = tid % p.k;
  const int dr = THREADS / p.k, dt = THREADS % p.k;
  long base = r0 * p.k;
  for (; base + (long)THREADS * U <= e1; base += (long)THREADS * U) strides<THREADS, true>(p, base, e1, row, t, dr, dt, sink);
  if (base < e1) strides<THREADS, false>(p, base, e1, row, t, dr, dt, sink);
}

__global__ __launch_bounds__(LDS_THREADS) void label_pairs_lds_kernel(PairArgs p) {
  extern __shared__ int bins[];                        // [G * G]
  const int cells = p.G * p.G;
  for (int c = threadIdx.x; c < cells; c += LDS_THREADS) bins[c] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  walk<LDS_THREADS>(p, [&](int key) {
    const unsigned long long have = __ballot(key >= 0);
    if (!have) return;
    const int leader = __ffsll((long long)have) - 1;
    const int lk = __builtin_amdgcn_readlane(key, leader);   // leader comes from a ballot: wave-uniform
    const unsigned long long same = __ballot(key == lk);
    if (key == lk) {
      if (lane == leader) atomicAdd(&bins[lk], __popcll(same));
    } else if (key >= 0) {
      atomicAdd(&bins[key], 1);
    }
  });
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += LDS_THREADS) {
    const int n = bins[c];
    if (n) add64(p.counts + c, n);
  }
}

__global__ __launch_bounds__(WAVE_THREADS) void label_pairs_wave_kernel(PairArgs p) {
  const int lane = threadIdx.x & (WAVE - 1);
  int held = -1;                                       // wave-uniform: the carried key and how many of it
  long long held_n = 0;
  walk<WAVE_THREADS>(p, [&](int key) {
    unsigned long long todo = __ballot(key >= 0);
    bool first = true;
    while (todo) {                                     // wave-uniform: every lane stays in
      const int leader = __ffsll((long long)todo) - 1;
      const int lk = __builtin_amdgcn_readlane(key, leader);   // leader comes from a ballot: wave-uniform
      const unsigned long long same = __ballot(key == lk);
      const int n = __popcll(same);
      if (first) {
        if (lk == held) {
          held_n += n;
        } else {
          if (held >= 0 && lane == 0) add64(p.counts + held, held_n);
          held = lk;
          held_n = n;
        }
        first = false;
      } else if (lane == leader) {
        add64(p.counts + lk, n);
      }
      todo &= ~same;
    }
  });
  if (held >= 0 && lane == 0) add64(p.counts + held, held_n);
}

}  // namespace

extern "C" int clipk_knn_label_pairs(const int64_t* idx, long long M, int k, const int32_t* row_labels,
                                     const int32_t* key_labels, long long Ny, int G, long long* counts, void* stream) {
  if (!idx || !row_labels || !key_labels || !counts || M < 1 || Ny < 1 || k < 1 || k > 1024 || G < 1)
    return CLIPK_ERR_BAD_ARG;
  if (G > CLIPK_LABEL_PAIRS_MAX_G || M > (1ll << 50)) return CLIPK_ERR_UNSUPPORTED;
  const bool lds = G <= LDS_MAX_G;
  const long total = (long)M * k;
  const int threads = lds ? LDS_THREADS : WAVE_THREADS;
  const size_t lds_bytes = lds ? (size_t)G * G * sizeof(int) : 0;
  // enough workgroups to fill the chip, none with less than four passes of its loop
  const long cap = (long)clipk_cu_count() * (lds ? (lds_bytes > 32768 ? 2 : 4) : 8);
  const long per = (long)threads * U * 4;
  long blocks = (total + per - 1) / per;
  blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
  long rows_per = ((long)M + blocks - 1) / blocks;
  const long quota = (long)INT32_MAX / k;              // the int32 bins of the lds kernel: fewer than 2^31 entries a workgroup
  if (rows_per > quota) rows_per = quota;
  blocks = ((long)M + rows_per - 1) / rows_per;
  if (blocks > INT32_MAX) return CLIPK_ERR_UNSUPPORTED;
  PairArgs p{idx, row_labels, key_labels, counts, (long)M, (long)Ny, rows_per, k, G};
  if (lds)
    hipLaunchKernelGGL(label_pairs_lds_kernel, dim3((unsigned)blocks), dim3(LDS_THREADS), lds_bytes, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(label_pairs_wave_kernel, dim3((unsigned)blocks), dim3(WAVE_THREADS), 0, (hipStream_t)stream, p);
  return clipk_check_launch();
}
