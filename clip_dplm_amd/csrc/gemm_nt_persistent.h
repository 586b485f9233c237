// gemm_nt_persistent.h — what the two persistent clipk_gemm_nt kernels share (gemm_nt_v3.hip: 256 x 256 tiles, one 8-wave
// workgroup per CU; gemm_nt_v4.hip: 128 x 256 tiles, two 4-wave workgroups per CU): device functions and host helpers, no
// kernel.  Both have the same wave tile (128 m x 64 n as acc[4][8], walked in quadrants of 64 m x 32 n), the same 64-deep
// K-tiles of XOR-swizzled 128-byte rows filled by buffer-descriptor LDS-DMA, and the same half-tiles by consumption
// order (X mh: 64 rows of an m-wave, from row m0 + 64 mh; W nh: 32 rows of each of the four n-waves, from row n0 + 32 nh).
// Their schedules - LDS map, piece assignment, phases, barriers, waits, stagger, tile loop - are the reason there are two
// kernels, and stay in the two files.
// Include it from exactly one kernel file per translation unit, and only from a kernel of this v3 / v4 kind: the names
// below (Params, BK, quad, rsrc_t, the CLIPK_* macros) land in that file's anonymous namespace and would collide with
// a Params or BK of its own.
#pragma once
#include "common.h"
#include "gemm_epilogue.h"
#include <stdlib.h>
#include <type_traits>

namespace {   // as the kernels' own file-local code: one copy per including file, internal linkage

constexpr int BK = 64;                          // K-tile depth

struct Params {
  const unsigned short* A; long lda;
  const unsigned short* B; long ldb;
  int M, N, K;
  EpiArgs e;
  int ntn, ntiles;
  int stagger;      // start-up delay in s_sleep(127) units, 0 = off (who waits: each kernel's own rule)
};

// one quadrant: 2 n-tiles x 4 m-tiles x 2 k-halves = 16 MFMAs (k outer so dependent accumulations sit 8 apart);
// KLO = 1: upper k-half only, for the last K-tile of a K % 64 == 32 problem (fetched as [K - 64, K), whose lower
// half was already accumulated by the K-tile before)
template <int NH, int MH, int KLO = 0>
__device__ __forceinline__ void quad(f32x4 (&acc)[4][8], const bf16x8 (&wf)[2][2][2], const bf16x8 (&xf)[4][2]) {
#pragma unroll
  for (int kk = KLO; kk < 2; ++kk)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[NH * 2 + t][MH * 4 + j] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[NH][t][kk], xf[j][kk], acc[NH * 2 + t][MH * 4 + j], 0, 0, 0);
}

#define CLIPK_BAR() __builtin_amdgcn_s_barrier()
#define CLIPK_SB() __builtin_amdgcn_sched_barrier(0)
#define CLIPK_STR2(x) #x
#define CLIPK_STR(x) CLIPK_STR2(x)
// counted wait that tolerates NS younger-than-the-loads store instructions (NS is a template constant 0 / 16 / 32)
#define CLIPK_VMCNT_PLUS(base, ns)                                                              \
  do {                                                                                          \
    if ((ns) == 0) asm volatile("s_waitcnt vmcnt(" CLIPK_STR(base) ")" ::: "memory");           \
    else if ((ns) == 16) asm volatile("s_waitcnt vmcnt(" CLIPK_STR(base) "+16)" ::: "memory");  \
    else asm volatile("s_waitcnt vmcnt(" CLIPK_STR(base) "+32)" ::: "memory");                  \
  } while (0)

using rsrc_t = decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, 0, 0, 0));

// descriptor over rows [row0, rows) of a [rows][K] operand: rows past the end fail the range check and load zeros
__device__ __forceinline__ rsrc_t operand_desc(const unsigned short* base, long ld, int row0, int rows, int K) {
  const long left = (long)rows - row0;
  const int bytes = left > 0 ? (int)(((left - 1) * ld + K) * 2) : 0;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (long)row0 * ld), 0, bytes, 0x00020000);
}

// tile -> origin and the four descriptors its LDS-DMA reads through, one per half-tile kind (scalar work only; the
// per-lane offsets never change)
template <int BM, int BN>
__device__ __forceinline__ void tile_source(const Params& p, int bid, int& m0, int& n0, rsrc_t& dx0, rsrc_t& dx1,
                                            rsrc_t& dw0, rsrc_t& dw1) {
  const int tile = xcd_remap(bid, p.ntiles);
  const int tm = tile / p.ntn, tn = tile - tm * p.ntn;
  m0 = tm * BM; n0 = tn * BN;
  dx0 = operand_desc(p.A, p.lda, m0, p.M, p.K); dx1 = operand_desc(p.A, p.lda, m0 + 64, p.M, p.K);
  dw0 = operand_desc(p.B, p.ldb, n0, p.N, p.K); dw1 = operand_desc(p.B, p.ldb, n0 + 32, p.N, p.K);
}

template <int MODE, class KernelOf>
void persistent_launch_mode(const Params& p, int nwg, int threads, int lds_bytes, hipStream_t st, KernelOf kernel_of) {
  const auto kernel = kernel_of(std::integral_constant<int, MODE>{});
  static std::atomic<uint64_t> attr_set{0};
  clipk_once_per_device(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  });
  hipLaunchKernelGGL(kernel, dim3(nwg), dim3(threads), lds_bytes, st, p);
}

// The launcher of both kernels, called by clipk_gemm_nt (gemm_nt.hip) after it validated the arguments (K % 32 == 0,
// K >= 160).  kernel_of(std::integral_constant<int, MODE>) names the kernel's instantiation for an epilogue mode.
template <class KernelOf>
int gemm_nt_persistent_launch(const clipk_gemm_args* a, void* stream, int BM, int BN, int workgroups_per_cu, int threads,
                              int lds_bytes, KernelOf kernel_of) {
  Params p = gemm_params_from<Params>(a);
  p.ntn = (a->N + BN - 1) / BN;
  p.ntiles = ((a->M + BM - 1) / BM) * p.ntn;
  // a multiple of 8 keeps "workgroup b runs on XCD b % 8" true for every tile it walks, so the XCD-contiguous tile
  // order (xcd_remap) still holds
  int nwg = (workgroups_per_cu * clipk_cu_count()) & ~7;
  { const int e = clipk_opt_get(OPT_GEMM_NWG); if (e >= 8) nwg = e & ~7; }                   // experiments only
  if (nwg > p.ntiles) nwg = p.ntiles;
  p.stagger = clipk_opt_get(OPT_GEMM_STAGGER);
  const int mode = select_epi_mode(a);
  if (mode == EPI_UNSUPPORTED || (a->rope_cos && mode != EPI_ROPE && mode != EPI_ROPE_IL))
    return CLIPK_ERR_UNSUPPORTED;                            // rotation: its own mode only
  with_epi_mode(mode, [&](auto m) {
    persistent_launch_mode<decltype(m)::value>(p, nwg, threads, lds_bytes, (hipStream_t)stream, kernel_of);
  });
  return clipk_check_launch();
}

}  // namespace
