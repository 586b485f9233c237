// knn.hip — clipk_pair_sqdist: the squared Euclidean distances of LISTED pairs,
//   d2[i, t] = sum_p (X[i, p] - Y[idx[i, t], p])^2,
// the distances of a k-nearest-neighbour graph whose indices clipk_sim_knn found (retrieval.hip).  The walk orders keys by
// z = <x, y> - |y|^2 / 2, and |x|^2 - 2 z would cancel exactly where neighbours are closest, so the distances are summed
// from the differences instead: Mx k P work, nothing next to the walk's Mx Ny P.  x[idx] in torch would be an Mx x k x P
// tensor; here one thread owns one pair and streams the two rows 16 bytes at a time.
//
// Summation order (fixed: results do not depend on the launch shape): four running sums a_c over the columns p = c mod 4
// in ascending p, each updated by one fma a_c = fma(d, d, a_c) with d = fl(x - y); the result is fl(fl(a_0 + a_1) +
// fl(a_2 + a_3)).  An index outside [0, Ny) (the -1 of a short list) gives +inf.
#include "common.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void pair_sqdist_kernel(const float* X, long Mx, const float* Y, int Ny, int P,
                                                          const int64_t* idx, int k, float* d2) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;                    // pair (i, t) = (e / k, e % k)
  if (e >= Mx * k) return;
  const int64_t j = idx[e];
  if (j < 0 || j >= Ny) { d2[e] = INFINITY; return; }
  const float* x = X + (e / k) * P;
  const float* y = Y + j * P;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < P; p += 4) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + p), yv = *reinterpret_cast<const f32x4*>(y + p);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = __fsub_rn(xv[c], yv[c]);
      a[c] = fmaf(d, d, a[c]);
    }
  }
  d2[e] = __fadd_rn(__fadd_rn(a[0], a[1]), __fadd_rn(a[2], a[3]));
}

}  // namespace

extern "C" int clipk_pair_sqdist(const float* X, int Mx, const float* Y, int Ny, int P, const int64_t* idx, int k,
                                 float* d2, void* stream) {
  if (!X || !Y || !idx || !d2) return CLIPK_ERR_BAD_ARG;
  if (Mx <= 0 || Ny <= 0 || P <= 0 || k <= 0) return CLIPK_ERR_BAD_ARG;
  if (P % 4) return CLIPK_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(Y)) return CLIPK_ERR_BAD_ARG;
  const long pairs = (long)Mx * k;
  const long blocks = (pairs + 255) / 256;
  if (blocks > INT32_MAX) return CLIPK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pair_sqdist_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X, (long)Mx, Y, Ny, P,
                     idx, k, d2);
  return clipk_check_launch();
}
