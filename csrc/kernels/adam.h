// AdamW and LAMB over a flat fp32 arena range (adam.hip). gfx950, wave64.
//
// One step, for the step count t (the steps taken so far, a device word) and T = t + 1:
//   g' = gs * g                            gs = (maximize ? -1 : 1) * clip coefficient
//   m  = beta1 * m + (1 - beta1) * g'      v = beta2 * v + (1 - beta2) * g'^2
//   a  = (m / (1 - beta1^T)) / (sqrt(v) / sqrt(1 - beta2^T) + eps)
//   r  = a + wd * w                        w = w - (lr * q) * r
// AdamW is q = 1: w - lr * (a + wd * w) is torch's decoupled decay w * (1 - lr * wd) - lr * a with one
// rounding on w instead of three. LAMB (You et al., "Large Batch Optimization for Deep Learning"):
// q = |w| / |r| per adapted parameter tensor (1 when either norm is 0), wd = 0 and q = 1 for an excluded
// one (ndim <= 1 under exclude_bias_and_norm).
//
// The per-step scalars 1 / (1 - beta1^T) and 1 / sqrt(1 - beta2^T) are evaluated in fp64 by thread 0 of
// every workgroup from the device's t, rounded once to fp32 and shared through LDS: every workgroup of
// every launch of a step uses the same bits, a captured hipGraph step needs no host value, and the
// per-element arithmetic has no division by a bias correction. The rate is the host value, lr_ptr[0]
// or the schedule's lr_t, as in the SGD kernels.
//
// t advances as the learning-rate schedule's step does (sched_arrive, step_common.h): AdamArgs::state
// = {t, arrivals}; the last launch of a step (advance) counts its workgroups' arrivals and the last
// one stores t + 1. A step skipped by the clip (skip_nonfinite) stores nothing and does not advance t.
#pragma once
#include "common.h"
#include "kernels.h"
#include "lars.h"

namespace cdp {

struct AdamArgs {
  long long* state = nullptr;       // {t, arrivals}, int64, device
  double beta1 = 0.0, beta2 = 0.0;  // for the bias corrections (fp64, in the prologue)
  float b1 = 0.f, omb1 = 0.f;       // float32(beta1), float32(1 - beta1)
  float b2 = 0.f, omb2 = 0.f;
  float eps = 0.f, wd = 0.f;
  int maximize = 0;
  int advance = 0;  // this launch is the last of its step: it stores t + 1
};

// The LAMB block reuses the LARS work list (lars.h: LarsParam / LarsItem from lars_plan) and its
// partials' layout: item k owns part[2k] = sum w^2 and part[2k + 1] = sum r^2 of its chunk. LarsArgs's
// eta, wd and eps are not read. params == nullptr: off (AdamW).

// w, g, m, v: n floats each (LAMB: the plan's range). LAMB runs lamb_moments_launch first.
void adam_launch(float* w, const float* g, float* m, float* v, long long n, const float* lr_ptr, float lr,
                 const AdamArgs& ad, hipStream_t st, long long* counter = nullptr, const ClipArgs& clip = ClipArgs{},
                 const LarsArgs& lamb = LarsArgs{}, const EmaArgs& ema = EmaArgs{},
                 const SchedArgs& sched = SchedArgs{});
// LAMB pass 1: the new m, v and the pair {sum w^2, sum r^2} of every item (all pairs are stored unless
// the step is skipped). Reads t, never advances it.
void lamb_moments_launch(const float* w, const float* g, float* m, float* v, const AdamArgs& ad, const ClipArgs& clip,
                         const LarsArgs& lamb, hipStream_t st);
// workgroups of adam_launch over n floats without LAMB
int adam_grid(long long n);

}  // namespace cdp
