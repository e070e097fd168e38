// The parts of a fused optimizer step that every step kernel shares (the SGD kernels of misc.hip, the
// Adam kernels of adam.hip): the weight EMA, the gradient-norm clip's prologue, the learning-rate
// schedule's prologue and the arrival rule with which the last launch of a step advances a device
// counter. Device code only; each including file gets its own copies (internal linkage).
#pragma once
#include "common.h"
#include "grad_clip.h"
#include "kernels.h"

namespace cdp {
namespace {

// Weight EMA (EMA instantiations only; EmaArgs in kernels.h): e = d * e + omd * w_new with the op
// order of e.mul_(d).add_(w_new, alpha=omd). Every path of both kernels calls this one function, so
// they all agree bitwise. A skipped step did not happen: e stays, and the store that follows writes
// the same bits back.
__device__ __forceinline__ float ema_one(float e, float w_new, float d, float omd) { return fmaf(w_new, omd, e * d); }
template <bool CLIP>
__device__ __forceinline__ void ema_upd(bool skip, float4& e, const float4& w, float d, float omd) {
  if (CLIP && skip) return;
  e.x = ema_one(e.x, w.x, d, omd);
  e.y = ema_one(e.y, w.y, d, omd);
  e.z = ema_one(e.z, w.z, d, omd);
  e.w = ema_one(e.w, w.w, d, omd);
}
// gs *= coef and the skip decision, in the kernel's prologue (every workgroup gets the same bits);
// workgroup 0 records norm / coef / skipped steps
__device__ __forceinline__ bool sgd_clip_prologue(const ClipArgs& clip, float& gs) {
  const ClipCoef c = clip_coef_block(clip.part, clip.nparts, clip.max_norm);
  const bool skip = clip.skip_nonfinite && clip_nonfinite(c.norm);
  if (clip.stats && blockIdx.x == 0 && threadIdx.x == 0) clip_write_stats(clip.stats, c, skip);
  gs *= c.coef;
  return skip;
}

// Learning-rate schedule (SCHED instantiations only; SchedArgs in kernels.h, lr_sched.h). Thread 0 of the
// workgroup loads t and the configuration, evaluates lr_t in fp64 and shares it through LDS (one
// barrier); every workgroup of every launch of a step gets the same bits. It keeps t for sched_arrive;
// workgroup 0 records the rate (last_lr is read by no launch).
__device__ __forceinline__ float sgd_sched_prologue(const SchedArgs& sched, float base, float* s_lr, long long& t) {
  if (threadIdx.x == 0) {
    t = sched.state[0];
    const float lr = lr_sched_rate(*sched.cfg, t, base);
    *s_lr = lr;
    if (blockIdx.x == 0 && sched.last_lr) sched.last_lr[0] = lr;
  }
  __syncthreads();
  return *s_lr;
}
// The advance of t (the last launch of a step: sched.advance). Every workgroup must see the same t, so
// nobody may store t + 1 while another workgroup can still load t. The thread that loaded t arrives at
// the end of its workgroup's work, on every exit path, with one relaxed, agent-scope, returning integer
// add on the arrival word; the thread that draws the last ticket knows that every other workgroup has
// loaded t already, stores t + 1 and zeroes the arrival word for the next launch.
// Nothing inside the launch reads those stores (the next launch sees them across the kernel
// boundary), so there is no fence. Integer tickets leave the step bitwise reproducible: whoever is
// last stores the same values.
typedef __attribute__((address_space(1))) long long glb_i64;
__device__ __forceinline__ void sched_arrive(const SchedArgs& sched, long long t) {
  if (threadIdx.x != 0 || !sched.advance) return;
  const long long ticket =
      __hip_atomic_fetch_add((glb_i64*)(sched.state + 1), 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket == (long long)gridDim.x - 1) {
    sched.state[0] = t + 1;
    sched.state[1] = 0;
  }
}

}  // namespace
}  // namespace cdp
