// Fused AdamW / LAMB step over a flat fp32 arena range (adam.h). gfx950, wave64, 256-thread
// workgroups, float4 loads and stores.
//
// adam_kernel<CLIP, LAMB, EMA, SCHED> is the step. Without LAMB it is a grid-stride loop over the
// range, as sgd_kernel's plain path: 4 loads (w, g, m, v) and 3 stores (w, m, v) per element, 28
// bytes; with EMA one more load and store, 36. LAMB is two launches over the lars_plan work list, one
// workgroup per (parameter, chunk): lamb_moments_kernel reads w, g, m, v, stores the new m, v and its
// chunk's fp64 pair {sum w^2, sum r^2} (r stays in registers: there is no update arena), and
// adam_kernel<.., LAMB, ..> reads w and the new m, v, recomputes r with the same function (the same
// bits), derives its parameter's q from the pairs in its prologue and applies w -= (lr * q) * r: 24 +
// 16 = 40 bytes per element, 48 with EMA. Bandwidth-bound either way; the fp64 in the prologues is a
// few operations of one thread per workgroup.
//
// The clip's, the EMA's and the schedule's parts and the arrival rule are the SGD kernels' own
// (step_common.h).
#include "adam.h"

#include <stdexcept>

#include "common.h"
#include "step_common.h"

namespace cdp {
namespace {

struct AdamScal {
  float b1, omb1, b2, omb2, eps;
  float rbc1;   // float32(1 / (1 - beta1^T))
  float rbc2s;  // float32(1 / sqrt(1 - beta2^T))
};

// The per-element arithmetic; every path calls it: the float4 body and the scalar tail of the plain
// step, LAMB's pass 1 (MOMENTS) and pass 2 (!MOMENTS: m and v are the new ones already). Returns
// r = a + wd * w. Explicit fmaf throughout and contraction off, so the paths agree bitwise whatever the
// compiler would fuse. fp32 roundings: g' 1 (none for gs = +-1), m 2, v 3, then sqrt, the fma of the
// denominator, m * rbc1, the division and the fma of r: 5. The division and the square root are the
// correctly rounded ones (the kernels are built without fast-math). Zero g, m, v give a = 0 and zero w
// then r = 0: the arena's pad floats stay zero (the m == 0 test covers eps == 0, where 0 / 0 would be
// NaN).
template <bool MOMENTS>
__device__ __forceinline__ float adam_one(float w, float g, float& m, float& v, const AdamScal& s, float gs, float wd) {
#pragma clang fp contract(off)
  if (MOMENTS) {
    const float gg = g * gs;
    m = fmaf(gg, s.omb1, m * s.b1);
    v = fmaf(gg * gg, s.omb2, v * s.b2);
  }
  float a = (m * s.rbc1) / fmaf(sqrtf(v), s.rbc2s, s.eps);
  if (m == 0.f) a = 0.f;
  return fmaf(w, wd, a);
}
// w -= (lr * q) * r
__device__ __forceinline__ float adam_apply(float w, float r, float lrq) { return fmaf(r, -lrq, w); }

// The per-step scalars, once per workgroup: thread 0 loads t and evaluates the two bias corrections in
// fp64; each is rounded to fp32 once and shared through LDS (one barrier). It keeps t for adam_arrive.
__device__ __forceinline__ AdamScal adam_prologue(const AdamArgs& ad, float* s_bc, long long& t) {
  if (threadIdx.x == 0) {
    t = ad.state[0];
    const double T = (double)(t + 1);
    s_bc[0] = (float)(1.0 / (1.0 - pow(ad.beta1, T)));
    s_bc[1] = (float)(1.0 / sqrt(1.0 - pow(ad.beta2, T)));
  }
  __syncthreads();
  AdamScal s;
  s.b1 = ad.b1, s.omb1 = ad.omb1, s.b2 = ad.b2, s.omb2 = ad.omb2, s.eps = ad.eps;
  s.rbc1 = s_bc[0];
  s.rbc2s = s_bc[1];
  return s;
}
// The advance of t: sched_arrive's rule on AdamArgs::state.
__device__ __forceinline__ void adam_arrive(const AdamArgs& ad, long long t) {
  if (threadIdx.x != 0 || !ad.advance) return;
  const long long ticket =
      __hip_atomic_fetch_add((glb_i64*)(ad.state + 1), 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket == (long long)gridDim.x - 1) {
    ad.state[0] = t + 1;
    ad.state[1] = 0;
  }
}

// For a 256-thread workgroup, all threads calling with the same `pr`: q = |w| / |r| of one parameter from
// its partial pairs, by the fixed-order reduction of lars_ratio_block (lars.h), in fp64, rounded once; 1
// for a zero norm and for excluded parameters (whose partials are not read).
__device__ __forceinline__ float lamb_ratio_block(const LarsArgs& la, const LarsParam& pr) {
  if (la.exclude && !pr.matrix) return 1.f;
  __shared__ double lred[8];
  double sw = 0.0, sr = 0.0;
  for (int i = threadIdx.x; i < pr.nparts; i += 256) {
    sw += la.part[2 * (pr.part0 + i)];
    sr += la.part[2 * (pr.part0 + i) + 1];
  }
  sw = wave_sum_d(sw);
  sr = wave_sum_d(sr);
  if ((threadIdx.x & 63) == 0) {
    lred[threadIdx.x >> 6] = sw;
    lred[4 + (threadIdx.x >> 6)] = sr;
  }
  __syncthreads();
  const double wn = sqrt((lred[0] + lred[1]) + (lred[2] + lred[3]));
  const double rn = sqrt((lred[4] + lred[5]) + (lred[6] + lred[7]));
  if (wn == 0.0 || rn == 0.0) return 1.f;
  return (float)(wn / rn);
}

__device__ __forceinline__ double sq_add(double acc, float x) {
  const double d = (double)x;
  return fma(d, d, acc);
}

template <bool CLIP, bool LAMB, bool EMA, bool SCHED>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                  float* __restrict__ m, float* __restrict__ v, long long n,
                                                  const float* __restrict__ lr_ptr, float lr_host, AdamArgs ad,
                                                  long long* counter, ClipArgs clip, LarsArgs lamb, EmaArgs ema,
                                                  SchedArgs sched) {
  __shared__ float s_bc[2];
  const float ed = EMA ? ema.coef[0] : 0.f, eomd = EMA ? ema.coef[1] : 0.f;
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) counter[0] += 1;  // as sgd_kernel
  float gs = ad.maximize ? -1.f : 1.f;
  bool skip = false;
  if (CLIP) skip = sgd_clip_prologue(clip, gs);
  float lr = lr_ptr ? lr_ptr[0] : lr_host;
  long long sched_t = 0, adam_t = 0;  // (thread 0)
  if (SCHED) {
    __shared__ float s_lr;
    lr = sgd_sched_prologue(sched, lr, &s_lr, sched_t);
  }
  const AdamScal s = adam_prologue(ad, s_bc, adam_t);
  if (CLIP && skip) {
    // the step did not happen: nothing is stored and t stays; the schedule counts the iteration
    if (SCHED) sched_arrive(sched, sched_t);
    return;
  }
  if (LAMB) {
    // one workgroup per (parameter, chunk) item of pass 1's work list: whole float4s of one parameter
    const LarsItem it = lamb.items[blockIdx.x];
    const LarsParam pr = lamb.params[it.param];
    const float q = lamb_ratio_block(lamb, pr);
    if ((int)blockIdx.x == pr.part0 && threadIdx.x == 0) lamb.ratios[pr.slot] = q;
    const float lrq = lr * q;
    const float wd = lamb.exclude && !pr.matrix ? 0.f : ad.wd;
    for (int i = threadIdx.x; i < it.n4; i += 256) {
      const long long e = it.start + 4LL * i;
      float4 wv = ld4(w + e);
      float4 mv = ld4(m + e);
      float4 vv = ld4(v + e);
      wv.x = adam_apply(wv.x, adam_one<false>(wv.x, 0.f, mv.x, vv.x, s, gs, wd), lrq);
      wv.y = adam_apply(wv.y, adam_one<false>(wv.y, 0.f, mv.y, vv.y, s, gs, wd), lrq);
      wv.z = adam_apply(wv.z, adam_one<false>(wv.z, 0.f, mv.z, vv.z, s, gs, wd), lrq);
      wv.w = adam_apply(wv.w, adam_one<false>(wv.w, 0.f, mv.w, vv.w, s, gs, wd), lrq);
      st4(w + e, wv);
      if (EMA) {
        float4 ev = ld4(ema.e + e);
        ema_upd<false>(false, ev, wv, ed, eomd);
        st4(ema.e + e, ev);
      }
    }
    if (SCHED) sched_arrive(sched, sched_t);
    adam_arrive(ad, adam_t);
    return;
  }
  const float wd = ad.wd;
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 wv = ld4(w + 4 * i);
    const float4 gv = ld4(g + 4 * i);
    float4 mv = ld4(m + 4 * i);
    float4 vv = ld4(v + 4 * i);
    wv.x = adam_apply(wv.x, adam_one<true>(wv.x, gv.x, mv.x, vv.x, s, gs, wd), lr);
    wv.y = adam_apply(wv.y, adam_one<true>(wv.y, gv.y, mv.y, vv.y, s, gs, wd), lr);
    wv.z = adam_apply(wv.z, adam_one<true>(wv.z, gv.z, mv.z, vv.z, s, gs, wd), lr);
    wv.w = adam_apply(wv.w, adam_one<true>(wv.w, gv.w, mv.w, vv.w, s, gs, wd), lr);
    st4(w + 4 * i, wv);
    st4(m + 4 * i, mv);
    st4(v + 4 * i, vv);
    if (EMA) {
      float4 ev = ld4(ema.e + 4 * i);
      ema_upd<false>(false, ev, wv, ed, eomd);
      st4(ema.e + 4 * i, ev);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    float mm = m[i], vv = v[i];
    const float ww = adam_apply(w[i], adam_one<true>(w[i], g[i], mm, vv, s, gs, wd), lr);
    w[i] = ww;
    m[i] = mm;
    v[i] = vv;
    if (EMA) ema.e[i] = ema_one(ema.e[i], ww, ed, eomd);
  }
  if (SCHED) sched_arrive(sched, sched_t);
  adam_arrive(ad, adam_t);
}

// LAMB pass 1. Workgroup k owns item k: it stores the new m, v of its chunk and the pair
// {sum w^2, sum r^2}, the squares added in fp64 (exact for fp32 values, so nothing overflows) with the
// fixed wave / LDS tree of lars_norms_kernel. Every pair is stored on every call that is not skipped.
template <bool CLIP>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, AdamArgs ad,
                                                          ClipArgs clip, LarsArgs lamb) {
  __shared__ float s_bc[2];
  __shared__ double red[8];
  float gs = ad.maximize ? -1.f : 1.f;
  bool skip = false;
  if (CLIP) skip = sgd_clip_prologue(clip, gs);
  long long adam_t = 0;
  const AdamScal s = adam_prologue(ad, s_bc, adam_t);
  if (CLIP && skip) return;  // pass 2 skips too and reads no pair
  const LarsItem it = lamb.items[blockIdx.x];
  const LarsParam pr = lamb.params[it.param];
  const float wd = lamb.exclude && !pr.matrix ? 0.f : ad.wd;
  double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  // each thread's elements are fixed by (item, threadIdx) alone
  for (int i = threadIdx.x; i < it.n4; i += 256) {
    const long long e = it.start + 4LL * i;
    const float4 wv = ld4(w + e);
    const float4 gv = ld4(g + e);
    float4 mv = ld4(m + e);
    float4 vv = ld4(v + e);
    const float rx = adam_one<true>(wv.x, gv.x, mv.x, vv.x, s, gs, wd);
    const float ry = adam_one<true>(wv.y, gv.y, mv.y, vv.y, s, gs, wd);
    const float rz = adam_one<true>(wv.z, gv.z, mv.z, vv.z, s, gs, wd);
    const float rw = adam_one<true>(wv.w, gv.w, mv.w, vv.w, s, gs, wd);
    st4(m + e, mv);
    st4(v + e, vv);
    w0 = sq_add(w0, wv.x);
    w1 = sq_add(w1, wv.y);
    w2 = sq_add(w2, wv.z);
    w3 = sq_add(w3, wv.w);
    r0 = sq_add(r0, rx);
    r1 = sq_add(r1, ry);
    r2 = sq_add(r2, rz);
    r3 = sq_add(r3, rw);
  }
  const double sw = wave_sum_d((w0 + w1) + (w2 + w3));
  const double sr = wave_sum_d((r0 + r1) + (r2 + r3));
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = sw;
    red[4 + (threadIdx.x >> 6)] = sr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* part = const_cast<double*>(lamb.part);
    part[2LL * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    part[2LL * blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

}  // namespace

int adam_grid(long long n) {
  long long b = ((n + 3) / 4 + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// 16 instantiations, CLIP x LAMB x EMA x SCHED, chosen as sgd_launch chooses its own
void adam_launch(float* w, const float* g, float* m, float* v, long long n, const float* lr_ptr, float lr,
                 const AdamArgs& ad, hipStream_t st, long long* counter, const ClipArgs& clip, const LarsArgs& lamb,
                 const EmaArgs& ema, const SchedArgs& sched) {
  if (!ad.state) throw std::runtime_error("adam: the step count {t, arrivals} is required");
  if ((ema.e != nullptr) != (ema.coef != nullptr)) throw std::runtime_error("adam: ema and ema_coef go together");
  if ((sched.state != nullptr) != (sched.cfg != nullptr)) throw std::runtime_error("adam: sched state and cfg go together");
  if (n < 1 || (lamb.params && lamb.nitems < 1)) throw std::runtime_error("adam: empty range");
  const dim3 grid(lamb.params ? lamb.nitems : adam_grid(n));
#define CDP_ADAM(CLIP, LAMB, EMA, SCHED)                                                                              \
  hipLaunchKernelGGL((adam_kernel<CLIP, LAMB, EMA, SCHED>), grid, dim3(256), 0, st, w, g, m, v, n, lr_ptr, lr, ad, \
                     counter, clip, lamb, ema, sched)
#define CDP_ADAM_S(CLIP, LAMB, EMA)                   \
  do {                                                \
    if (sched.state) CDP_ADAM(CLIP, LAMB, EMA, true); \
    else CDP_ADAM(CLIP, LAMB, EMA, false);            \
  } while (0)
#define CDP_ADAM_E(CLIP, LAMB)               \
  do {                                       \
    if (ema.e) CDP_ADAM_S(CLIP, LAMB, true); \
    else CDP_ADAM_S(CLIP, LAMB, false);      \
  } while (0)
  if (lamb.params) {
    if (clip.part) CDP_ADAM_E(true, true);
    else CDP_ADAM_E(false, true);
  } else {
    if (clip.part) CDP_ADAM_E(true, false);
    else CDP_ADAM_E(false, false);
  }
#undef CDP_ADAM_E
#undef CDP_ADAM_S
#undef CDP_ADAM
}

void lamb_moments_launch(const float* w, const float* g, float* m, float* v, const AdamArgs& ad, const ClipArgs& clip,
                         const LarsArgs& lamb, hipStream_t st) {
  if (!ad.state) throw std::runtime_error("lamb_moments: the step count {t, arrivals} is required");
  if (!lamb.params || lamb.nitems < 1) throw std::runtime_error("lamb_moments: the plan of lars_plan is required");
  if (clip.part)
    hipLaunchKernelGGL(lamb_moments_kernel<true>, dim3(lamb.nitems), dim3(256), 0, st, w, g, m, v, ad, clip, lamb);
  else
    hipLaunchKernelGGL(lamb_moments_kernel<false>, dim3(lamb.nitems), dim3(256), 0, st, w, g, m, v, ad, clip, lamb);
}

}  // namespace cdp
