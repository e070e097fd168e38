// LARS (layer-wise adaptive rate scaling) over a flat fp32 arena range: the work list of the norms
// pass (lars.hip) and the prologue with which a workgroup of the fused SGD kernels (misc.hip) turns
// its parameter's partial sums of squares into the trust ratio q. gfx950, wave64.
//
// Layout of the plan (built on the host once per arena layout, ops.cpp lars_plan):
//   LarsParam[i]   one per parameter of the range, in arena order: its floats [off, off + 4 * n4)
//                  relative to the range start (the arena pads every parameter to whole float4 with
//                  zeros), its partials [part0, part0 + nparts) and where its ratio goes
//   LarsItem[k]    one (parameter, chunk) per workgroup of the norms pass; item k writes the pair
//                  part[2k] = sum w^2, part[2k + 1] = sum g^2 of its chunk. The items of one
//                  parameter are consecutive, so item k IS partial k.
// Chunk boundaries depend on the parameter's size alone (lars_nparts / lars_chunk4), every pair is
// stored on every call and each consumer adds a parameter's pairs in one fixed order: the ratios are
// bitwise reproducible and need no zeroing, no atomics and no hand-off between workgroups.
#pragma once
#include <math.h>

#include "common.h"

namespace cdp {

constexpr int kLarsMaxParts = 256;         // partials per parameter (one per thread of a consumer's prologue)
constexpr long long kLarsMinChunk4 = 2048;  // float4 per chunk before a parameter gets another one
inline int lars_nparts(long long n4) {
  const long long want = (n4 + kLarsMinChunk4 - 1) / kLarsMinChunk4;
  return want < 1 ? 1 : (want > kLarsMaxParts ? kLarsMaxParts : (int)want);
}
inline long long lars_chunk4(long long n4) {  // float4 per chunk: whole 256-thread rows (1024 floats)
  const long long p = lars_nparts(n4);
  const long long c4 = ((n4 + p - 1) / p + 255) / 256 * 256;
  return c4 > 256 ? c4 : 256;
}

struct LarsParam {
  long long off;  // first float, relative to the range start (a multiple of 4)
  long long n4;   // float4 of the parameter, pad included
  int part0, nparts;
  int slot;     // index of its ratio in trust_ratios (the param group's order)
  int matrix;   // ndim > 1: adapted and decayed even under exclude_bias_and_norm
};
struct LarsItem {
  long long start;  // first float, relative to the range start
  int n4;
  int param;
};

// The LARS block of a fused SGD launch. params == nullptr: off, the kernels run exactly as without
// this block. owner: the parameter that owns the elements of each workgroup of the consuming launch
// (plain step: implied by items; prep step: one entry per conv-weight segment, then one per rest
// chunk, the chunks cut at parameter boundaries).
struct LarsArgs {
  const LarsParam* params = nullptr;
  const LarsItem* items = nullptr;
  const int* owner = nullptr;
  const double* part = nullptr;
  float* ratios = nullptr;
  double eta = 0.0, wd = 0.0, eps = 0.0;
  int nitems = 0;
  int exclude = 1;
};

#ifdef __HIPCC__
// For a 256-thread workgroup, all threads calling with the same `pr`. q of one parameter from its
// partial pairs: thread t adds pairs t, t + 256, ... (nparts <= 256: at most one), then the fixed
// butterfly / LDS tree of the other reductions here, so every workgroup of the parameter gets the
// same bits. gsc = grad_scale * clip coefficient. q = eta * |w| / (gsc * |g| + wd * |w| + eps) in
// fp64, rounded once; 1 for a zero weight or gradient norm and for excluded parameters (whose
// partials are not read). inf / NaN propagate as IEEE gives.
__device__ __forceinline__ float lars_ratio_block(const LarsArgs& la, const LarsParam& pr, float gsc) {
  if (la.exclude && !pr.matrix) return 1.f;
  __shared__ double lred[8];
  double sw = 0.0, sg = 0.0;
  for (int i = threadIdx.x; i < pr.nparts; i += 256) {
    sw += la.part[2 * (pr.part0 + i)];
    sg += la.part[2 * (pr.part0 + i) + 1];
  }
  sw = wave_sum_d(sw);
  sg = wave_sum_d(sg);
  if ((threadIdx.x & 63) == 0) {
    lred[threadIdx.x >> 6] = sw;
    lred[4 + (threadIdx.x >> 6)] = sg;
  }
  __syncthreads();
  const double wn = sqrt((lred[0] + lred[1]) + (lred[2] + lred[3]));
  const double gn = fabs((double)gsc) * sqrt((lred[4] + lred[5]) + (lred[6] + lred[7]));
  if (wn == 0.0 || gn == 0.0) return 1.f;
  return (float)(la.eta * wn / (gn + la.wd * wn + la.eps));
}
#endif

void lars_norms_launch(const float* w, const float* g, const LarsItem* items, int nitems, double* part, hipStream_t st);

}  // namespace cdp
