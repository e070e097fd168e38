// Global gradient norm of a flat fp32 arena range and the stand-alone clip-scale pass. gfx950, wave64.
//
// grad_sumsq_kernel: P fp64 partial sums of squares, one per workgroup, each over one fixed
// contiguous chunk (kernels.h grad_norm_parts / grad_norm_chunk). The square of an fp32 value is
// exact in fp64, so no square overflows and the only rounding is the fp64 additions (relative error
// at most n * 2^-53); the pass is bandwidth-bound and the fp64 FMAs ride along. No atomics and no
// hand-off between workgroups: the partials are combined by every consumer in its own prologue
// (grad_clip.h), in one fixed order, which keeps norm and coefficient bitwise reproducible.
#include "common.h"
#include "grad_clip.h"
#include "kernels.h"

namespace cdp {
namespace {

__device__ __forceinline__ double sq_add(double acc, float v) {
  const double d = (double)v;
  return fma(d, d, acc);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n, long long chunk4,
                                                        double* __restrict__ part) {
  __shared__ double red[4];
  const long long n4 = n >> 2;
  const long long a = (long long)blockIdx.x * chunk4;
  const long long b = a + chunk4 < n4 ? a + chunk4 : n4;  // a workgroup past the end: a >= b, nothing to add
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  // chunk4 is a multiple of 256: each thread's elements are fixed by (blockIdx, threadIdx) alone
#pragma unroll 4
  for (long long i = a + threadIdx.x; i < b; i += 256) {
    const float4 v = ld4(g + 4 * i);
    s0 = sq_add(s0, v.x);
    s1 = sq_add(s1, v.y);
    s2 = sq_add(s2, v.z);
    s3 = sq_add(s3, v.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) s0 = sq_add(s0, g[(n4 << 2) + threadIdx.x]);
  double s = wave_sum_d((s0 + s1) + (s2 + s3));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ g, long long n,
                                                        const double* __restrict__ part, int nparts, float max_norm,
                                                        float* __restrict__ stats) {
  const ClipCoef c = clip_coef_block(part, nparts, max_norm);
  if (stats && blockIdx.x == 0 && threadIdx.x == 0) clip_write_stats(stats, c, false);
  const float k = c.coef;
  const bool keep0 = !(k == k);  // NaN coef: exact zeros (the arena's pad floats) stay zero
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = ld4(g + 4 * i);
    float4 r = make_float4(v.x * k, v.y * k, v.z * k, v.w * k);
    if (keep0) {
      if (v.x == 0.f) r.x = v.x;
      if (v.y == 0.f) r.y = v.y;
      if (v.z == 0.f) r.z = v.z;
      if (v.w == 0.f) r.w = v.w;
    }
    st4(g + 4 * i, r);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    const float v = g[i];
    g[i] = (keep0 && v == 0.f) ? v : v * k;
  }
}

}  // namespace

void grad_sumsq_launch(const float* g, long long n, double* part, hipStream_t st) {
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grad_norm_parts(n)), dim3(256), 0, st, g, n, grad_norm_chunk(n) / 4, part);
}

void clip_scale_launch(float* g, long long n, const double* part, int nparts, float max_norm, float* stats,
                       hipStream_t st) {
  long long b = ((n + 3) / 4 + 255) / 256;
  b = b < 1 ? 1 : (b > 4096 ? 4096 : b);
  hipLaunchKernelGGL(clip_scale_kernel, dim3((int)b), dim3(256), 0, st, g, n, part, nparts, max_norm, stats);
}

}  // namespace cdp
