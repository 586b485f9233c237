// cloud_keysum.h — what the cloud kernels with a weighted key sum (sinkhorn.hip's apply pass, kernel_sums.hip, kmeans.hip,
// label_dist_sums.hip) put behind cloud_tile.h's tile walk:
//   * key_sum_tile.h's key_sum_zero / key_sum_tile / key_sum_store (device functions; the InfoNCE kernels share them);
//   * split_sum_finalize: key-split slabs and row partials summed in split order.
// A header of its own because it holds a kernel: every file that includes it gets the kernel in its code object.
#pragma once
#include "key_sum_tile.h"

namespace {

// out[Mx][P] (null: skipped) and up to two row outputs (null: skipped), each the sum of its key-split partials in split
// order (a fixed order: deterministic)
__global__ __launch_bounds__(256) void split_sum_finalize(const float* slab, const float* part_a, const float* part_b,
                                                          int ksplit, int Mx, int P, float* out, float* row_a,
                                                          float* row_b) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  if (out) {
    const long n4 = (long)Mx * P / 4, slab_n = (long)Mx * P;
    for (long i = tid; i < n4; i += nth) {
      f32x4 a = reinterpret_cast<const f32x4*>(slab)[i];
      for (int s = 1; s < ksplit; ++s) a += reinterpret_cast<const f32x4*>(slab + (long)s * slab_n)[i];
      reinterpret_cast<f32x4*>(out)[i] = a;
    }
  }
  for (long i = tid; i < Mx; i += nth) {
    if (row_a) {
      float a = 0.f;
      for (int s = 0; s < ksplit; ++s) a += part_a[(long)s * Mx + i];
      row_a[i] = a;
    }
    if (row_b) {
      float a = 0.f;
      for (int s = 0; s < ksplit; ++s) a += part_b[(long)s * Mx + i];
      row_b[i] = a;
    }
  }
}

// the launch of split_sum_finalize on the workspace slabs [ksplit][Mx][P] and partials
inline void launch_split_sum_finalize(const float* slab, const float* part_a, const float* part_b, int ksplit, int Mx, int P,
                                      float* out, float* row_a, float* row_b, hipStream_t stream) {
  long blocks = out ? ((long)Mx * P / 4 + 255) / 256 : (Mx + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(split_sum_finalize, dim3((int)blocks), dim3(256), 0, stream, slab, part_a, part_b, ksplit, Mx, P, out,
                     row_a, row_b);
}

}  // namespace
