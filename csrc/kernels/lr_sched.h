// Learning-rate schedule of the fused SGD / LARS step, evaluated on the device.
//
// The schedule is a dimensionless factor f(t) of the step index t >= 0 (the number of step() calls so
// far): linear warm-up (Goyal et al.) into a constant, cosine, polynomial (You et al.: power 2) or
// multi-step phase. The rate of a step is lr_t = float32(double(base) * f(t)), base being the rate the
// kernel would use without a schedule (lr_ptr ? lr_ptr[0] : lr_host). f is a pure function of
// (cfg, t): thread 0 of every workgroup of the SGD kernels evaluates lr_sched_factor itself in fp64
// and gets the same bits, so the schedule needs no launch of its own and no host-side value, and a
// replayed hipGraph steps at a new rate every time. The configuration lives in device memory (as the
// EMA's coefficients do), so it can be refilled between replays without re-capture.
//
// How t advances (SchedArgs::state = {t, arrivals}) is described at sched_arrive in step_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace cdp {

constexpr int kLrConstant = 0, kLrCosine = 1, kLrPoly = 2, kLrStep = 3;
constexpr int kLrMaxMilestones = 8;

struct LrSchedCfg {  // 128 bytes; filled by lr_sched_pack (ops.cpp), the only writer
  long long kind;          // kLr*
  long long warmup_steps;  // W >= 0
  long long total_steps;   // T > W (cosine, poly)
  long long nmilestones;   // <= kLrMaxMilestones (step)
  long long milestones[kLrMaxMilestones];  // strictly increasing
  double warmup_start_factor;              // s in [0, 1]
  double end_factor;                       // r >= 0
  double power;                            // > 0 (poly)
  double gamma;                            // > 0 (step)
};

__host__ __device__ __forceinline__ double lr_sched_factor(const LrSchedCfg& c, long long t) {
  const long long W = c.warmup_steps, T = c.total_steps;
  if (t < W) return c.warmup_start_factor + (1.0 - c.warmup_start_factor) * (double)t / (double)W;
  if (c.kind == kLrCosine || c.kind == kLrPoly) {
    const double r = c.end_factor;
    if (t >= T) return r;  // r itself, not the formula at u = 1
    const double u = (double)(t - W) / (double)(T - W);
    if (c.kind == kLrCosine) return r + (1.0 - r) * 0.5 * (1.0 + cos(3.14159265358979323846 * u));
    return r + (1.0 - r) * pow(1.0 - u, c.power);
  }
  if (c.kind == kLrStep) {
    double f = 1.0;  // gamma^k by k multiplications, k = milestones <= t
    for (int i = 0; i < kLrMaxMilestones; ++i)
      if (i < c.nmilestones && c.milestones[i] <= t) f *= c.gamma;
    return f;
  }
  return 1.0;
}

__host__ __device__ __forceinline__ float lr_sched_rate(const LrSchedCfg& c, long long t, float base) {
  return (float)((double)base * lr_sched_factor(c, t));
}

}  // namespace cdp
