// LARS norms pass: per-parameter sums of squares of weights and gradients over a flat fp32 arena
// range, one launch. gfx950, wave64.
//
// Workgroup k owns item k of the work list (lars.h): one fixed chunk of one parameter. It reads the
// chunk of w and of g once, as float4, adds the squares in fp64 (the square of an fp32 value is exact
// in fp64, so nothing overflows and the only rounding is the fp64 additions: relative error at most
// n * 2^-53), reduces with the fixed wave / LDS tree and stores the pair {sum w^2, sum g^2}. Like
// grad_sumsq_kernel (grad_norm.hip) the pass is bandwidth-bound with the fp64 FMAs riding along;
// its traffic is one read of the parameter range and one of the gradient range.
#include "lars.h"

#include "common.h"

namespace cdp {
namespace {

__device__ __forceinline__ double sq_add(double acc, float v) {
  const double d = (double)v;
  return fma(d, d, acc);
}

__global__ __launch_bounds__(256) void lars_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                        const LarsItem* __restrict__ items, double* __restrict__ part) {
  __shared__ double red[8];
  const LarsItem it = items[blockIdx.x];
  const float* __restrict__ wp = w + it.start;
  const float* __restrict__ gp = g + it.start;
  double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
  // each thread's elements are fixed by (item, threadIdx) alone
#pragma unroll 2
  for (int i = threadIdx.x; i < it.n4; i += 256) {
    const float4 a = ld4(wp + 4LL * i);
    const float4 b = ld4(gp + 4LL * i);
    w0 = sq_add(w0, a.x);
    w1 = sq_add(w1, a.y);
    w2 = sq_add(w2, a.z);
    w3 = sq_add(w3, a.w);
    g0 = sq_add(g0, b.x);
    g1 = sq_add(g1, b.y);
    g2 = sq_add(g2, b.z);
    g3 = sq_add(g3, b.w);
  }
  const double sw = wave_sum_d((w0 + w1) + (w2 + w3));
  const double sg = wave_sum_d((g0 + g1) + (g2 + g3));
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = sw;
    red[4 + (threadIdx.x >> 6)] = sg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2LL * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    part[2LL * blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

}  // namespace

void lars_norms_launch(const float* w, const float* g, const LarsItem* items, int nitems, double* part, hipStream_t st) {
  if (nitems < 1) return;
  hipLaunchKernelGGL(lars_norms_kernel, dim3(nitems), dim3(256), 0, st, w, g, items, part);
}

}  // namespace cdp
