// simce_tile.h — what only the tiled InfoNCE kernels (simce_tiled.hip: plain and class-aware; simce_hard.hip:
// hard-negative) share on top of cloud_tile.h's KeyWalk<BKT, true> and key_sum_tile.h's weighted key sum:
//   * SimceOps, the operand block every pass takes, simce_ops (its host filler) and simce_rebase (a batched launch's
//     per-problem operands);
//   * simce_key_class: the class id of a key row; simce_dscale_merge: the d scale partial of a gradient pass;
//   * simce_launch: the launch of a pass on the grid of key_split_plan, with its dynamic LDS allowed once per device.
// Each kernel keeps its own statistics, G formula, merge rule and partial format.
#pragma once
#include "key_sum_tile.h"
#include <math.h>

namespace {

// the gradient passes' dynamic LDS: K-loop buffers, G tile + staged key block, d scale partials of key-wave 1
constexpr int SIMCE_GRAD_LDS_FLOATS = KLOOP_LDS_FLOATS + KEYSUM_LDS_FLOATS + 2 * TQ;

// (The argument structs hold it LAST, behind the pass's own fields: the problem table z is the bulk of it, and a
// single-problem kernel then reads everything it needs from the first lines of its argument block.)
struct SimceOps {
  const float* X; int Mx;
  const float* Y; int Ny;                         // batch keys
  const float* Yc; int Nc;                        // cache keys behind them (Nc = 0: Yc = Y)
  int P;
  const float* scale; int label_offset;
  const int64_t* cls_x; const int64_t* cls_y;     // [Mx] / [Ny] class ids, or both null (all distinct)
  int tiles_per_split, ntiles;
  PairZ z;                                        // batched launch: the problems; outputs and partials follow one another
};

// zt: the batched launch of zt->nz problems of shape Mx x Ny (X, Y, Yc and the ids come from the table, in the kernel)
inline SimceOps simce_ops(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P, const float* scale,
                          int label_offset, const int64_t* cls_x, const int64_t* cls_y, const KeySplitPlan& k,
                          const PairZ* zt = nullptr) {
  SimceOps o{};
  o.X = X; o.Mx = Mx; o.Y = Y; o.Ny = Ny; o.Yc = Yc ? Yc : Y; o.Nc = Nc; o.P = P;
  o.scale = scale; o.label_offset = label_offset; o.cls_x = cls_x; o.cls_y = cls_y;
  o.tiles_per_split = k.tiles_per_split; o.ntiles = k.ntiles;
  if (zt) o.z = *zt;
  return o;
}

// batched launch: the operands of this workgroup's problem (blockIdx.z) from the table zt (the kernel argument's own,
// indexed in place); returns the rows of key-split partials that lie before the problem
__device__ __forceinline__ long simce_rebase(SimceOps& o, const PairZ& zt) {
  const int z = blockIdx.z;
  o.X = zt.E + (long)zt.xa[z] * o.Mx * o.P;
  o.Y = o.Yc = zt.E + (long)zt.ya[z] * o.Ny * o.P;
  o.cls_x = o.cls_y = zt.ids[z];
  return (long)z * gridDim.y * o.Mx;
}

// the class id of a key as query class cq sees it: cache keys and keys without ids are never same-class.  (The loop over
// a lane's 16 key rows stays with the caller, as for KeyWalk::key_bias.)
__device__ __forceinline__ int64_t simce_key_class(const int64_t* cls_y, int key, int Ny, int64_t cq) {
  return (cls_y && key < Ny) ? cls_y[key] : ~cq;
}

// d scale partial of query qg in split ks: lane halves, then the two key-waves through dsl [TQ]
__device__ __forceinline__ void simce_dscale_merge(float dsc, float* dsl, float* dsc_part, int ks, int Mx, int qg, int wm,
                                                   int wn, int li, int h) {
  dsc += __shfl_xor(dsc, 32, 64);
  if (wm == 1 && h == 0) dsl[wn * 32 + li] = dsc;
  __syncthreads();
  if (wm == 0 && h == 0 && qg < Mx) dsc_part[(long)ks * Mx + qg] = dsc + dsl[wn * 32 + li];
}

// one workgroup per (query block, key split, problem); lds > 0: dynamic LDS, allowed once per device and kernel
template <auto Kernel, typename Args>
int simce_launch(const Args& p, const KeySplitPlan& k, int problems, size_t lds, void* stream) {
  if (lds) {
    static std::atomic<uint64_t> attr_set{0};
    clipk_once_per_device(attr_set, [&] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
  }
  hipLaunchKernelGGL(Kernel, dim3(k.nqb, k.ksplit, problems), dim3(256), lds, (hipStream_t)stream, p);
  return clipk_check_launch();
}

}  // namespace
