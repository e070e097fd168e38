// Clip coefficient of a gradient-norm clip, derived on the device from the partial sums of squares
// grad_sumsq_kernel wrote (grad_norm.hip). Every consuming workgroup (the clip-scale pass, the fused
// SGD kernels) combines the partials itself in its prologue, in one fixed order, so all of them get
// the same bits without a fence, a ticket or a second launch: a few KB of L2 reads per workgroup.
#pragma once
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace cdp {

struct ClipCoef {
  float norm;  // (float)sqrt(sum of squares)
  float coef;  // min(max_norm / (norm + 1e-6), 1), NaN for a NaN norm (torch's clamp(max=1))
};

// For a 256-thread workgroup, all threads calling. Thread t sums partials t, t + 256, ... in fp64,
// then the fixed butterfly / LDS tree of the other reductions here. The coefficient is evaluated the
// way torch evaluates `max_norm / (total_norm + 1e-6)` for a Python-float max_norm in
// clip_grad_norm_ (Tensor.__rtruediv__): the reciprocal, then the product, each rounded once in fp32.
// The reciprocal is a plain fp32 `/`: the kernels are built without fast-math, where hipcc emits the
// correctly rounded division, so the result equals the host's bit for bit.
__device__ __forceinline__ ClipCoef clip_coef_block(const double* __restrict__ part, int nparts, float max_norm) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const double tot = (red[0] + red[1]) + (red[2] + red[3]);
  ClipCoef r;
  r.norm = (float)sqrt(tot);
  const float c = (1.f / (r.norm + 1e-6f)) * max_norm;
  r.coef = c > 1.f ? 1.f : c;
  return r;
}

// inf or NaN (the norm is never negative)
__device__ __forceinline__ bool clip_nonfinite(float norm) { return !(norm < INFINITY); }

// stats[0] = norm, stats[1] = coef; stats[2] counts the skipped steps. One thread of one workgroup.
__device__ __forceinline__ void clip_write_stats(float* __restrict__ stats, const ClipCoef& c, bool skipped) {
  stats[0] = c.norm;
  stats[1] = c.coef;
  if (skipped) stats[2] += 1.f;
}

}  // namespace cdp
