// Squeeze-and-Excitation tail of a residual block (Hu et al., "Squeeze-and-Excitation Networks"):
//   z[n][c] = mean_hw u[n][hw][c]                      squeeze
//   h[n][j] = relu(W1[j][:] . z[n][:] + b1[j])         j < Cr
//   g[n][c] = sigmoid(W2[c][:] . h[n][:] + b2[c])
//   out     = relu(s[n] * g[n][c] * u + r)             s: optional stochastic-depth row
// with u the block's last BatchNorm output and r its shortcut, both NHWC fp32.
//
// All of it is memory-bound NHWC streaming plus, per image, a 1 x C x Cr and a 1 x Cr x C
// matrix-vector product. The matrix instructions do not fit those: every MFMA shape produces a tile
// of at least 4 x 4 outputs and an image brings ONE row, so three quarters or more of each instruction
// would multiply padding, and at 2 C Cr flops per image (0.5 MFLOP at C = 2048) the products cost less
// than reading the weights once. They are plain FMAs on 16-byte loads: one wave per hidden unit
// (layer 1), one thread per output channel (layer 2).
//
// The three NHWC passes and the two NHWC reductions share one split of an image (SeSplit): a
// workgroup owns pixels [chunk * cpix, (chunk + 1) * cpix) of ONE image, so the gate row g[n][:] (and
// s[n], dpool[n][:]) is fetched once per thread into registers, never per pixel. Inside a workgroup
// thread t owns channel quad t % TQ (TQ = min(C / 4, 256); quads TQ apart when C / 4 > 256) and walks
// the pixels of row group t / TQ, RG = 256 / TQ apart: consecutive lanes read consecutive 16-byte
// words of the chunk, whatever C is.
//
// Determinism: the reductions are sums in a fixed order (per thread over its pixels, over the row
// groups through LDS, over the chunks in ascending order in the per-image kernels, over the batch in
// ascending order in the parameter gradients). No float atomics anywhere; the only atomics are the
// integer max of the act-max publication (act_max.h), which is order-independent.
#include <algorithm>

#include "act_max.h"
#include "common.h"
#include "kernels.h"

namespace cdp {

namespace {

static_assert(kMaxSeC == kMaxActC, "the scale pass keeps its channel maxima in an ActMaxBlock<kMaxActC>");
constexpr int kSeThreads = 256;
constexpr int kSeMaxChunks = 64;  // pixel chunks per image at most (bounds the partial rows)
// the two per-image kernels: a batch brings only N workgroups, each walking W1 and W2 once, so a workgroup is
// as large as it can be (16 waves to hide the weight loads behind)
constexpr int kSeImgThreads = 1024;

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 div4(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
// gout where the block's ReLU passed (out > 0), else 0
__device__ __forceinline__ float4 relu_route4(float4 gout, float4 out) {
  return make_float4(out.x > 0.f ? gout.x : 0.f, out.y > 0.f ? gout.y : 0.f, out.z > 0.f ? gout.z : 0.f,
                     out.w > 0.f ? gout.w : 0.f);
}

// A workgroup's place in the split: image n, pixels [p0, p1) of it, and the thread's quad / row group.
struct SeWork {
  int n, p0, p1, C4, TQ, RG, cq, row;
  bool live;  // the thread has a row group (256 need not be a multiple of TQ)
  long long img;  // float offset of image n
  __device__ SeWork(int HW, int C, int nchunk, int cpix) {
    n = blockIdx.x / nchunk;
    const int ch = blockIdx.x - n * nchunk;
    p0 = ch * cpix;
    p1 = min(HW, p0 + cpix);
    C4 = C >> 2;
    TQ = min(C4, kSeThreads);
    RG = kSeThreads / TQ;
    row = threadIdx.x / TQ;
    cq = threadIdx.x - row * TQ;
    live = row < RG;
    img = (long long)n * HW * C;
  }
};

// ------------------------------------------------------------------ NHWC reductions
// part[n][chunk][c] = sum over the chunk's pixels of u (BWD = false: the squeeze) or of
// dz * u, dz = gout * (out > 0) (BWD = true: the gate's gradient before s[n] and the sigmoid).
// Four independent accumulators per thread keep four 16-byte loads per operand in flight; they and
// the row groups (LDS) are combined in a fixed order.
template <bool BWD>
__device__ __forceinline__ void se_reduce_body(const float* __restrict__ u, const float* __restrict__ gout,
                                               const float* __restrict__ out, float* __restrict__ part, int HW,
                                               int C, int nchunk, int cpix) {
  __shared__ float4 red[kSeThreads];
  const SeWork w(HW, C, nchunk, cpix);
  const int tid = threadIdx.x;
  float* dst = part + (long long)blockIdx.x * C;
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    float4 a[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    if (w.live && q < w.C4) {
      auto term = [&](int p) {
        const long long off = w.img + (long long)p * C + 4 * q;
        const float4 uv = ld4(u + off);
        if constexpr (!BWD) return uv;
        else {
          const float4 dz = relu_route4(ld4(gout + off), ld4(out + off));
          return make_float4(dz.x * uv.x, dz.y * uv.y, dz.z * uv.z, dz.w * uv.w);
        }
      };
      int p = w.p0 + w.row;
      for (; p + 3 * w.RG < w.p1; p += 4 * w.RG) {
        float4 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = term(p + k * w.RG);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = add4(a[k], t[k]);
      }
      for (; p < w.p1; p += w.RG) a[0] = add4(a[0], term(p));
    }
    red[tid] = add4(add4(a[0], a[1]), add4(a[2], a[3]));
    __syncthreads();
    if (tid < w.TQ && q < w.C4) {  // row group 0's threads: the quad's row groups in ascending order
      float4 t = red[tid];
      for (int r = 1; r < w.RG; ++r) t = add4(t, red[r * w.TQ + tid]);
      st4(dst + 4 * q, t);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kSeThreads) void se_squeeze_kernel(const float* __restrict__ u, float* __restrict__ part,
                                                                int HW, int C, int nchunk, int cpix) {
  se_reduce_body<false>(u, nullptr, nullptr, part, HW, C, nchunk, cpix);
}

__global__ __launch_bounds__(kSeThreads) void se_bwd_reduce_kernel(const float* __restrict__ gout,
                                                                   const float* __restrict__ out,
                                                                   const float* __restrict__ u,
                                                                   float* __restrict__ part, int HW, int C, int nchunk,
                                                                   int cpix) {
  se_reduce_body<true>(u, gout, out, part, HW, C, nchunk, cpix);
}

// ------------------------------------------------------------------ excitation (one workgroup per image)
// sigmoid(a) from e = exp(-|a|) in (0, 1], as bce_grad (misc.hip): 1 / (1 + e) or e / (1 + e), finite and
// in [0, 1] for every finite a; a NaN stays a NaN
__device__ __forceinline__ float se_sigmoid(float a) {
  const float e = expf(-fabsf(a));
  return (a >= 0.f ? 1.f : e) / (1.f + e);
}

// w2v: W2's rows can be read as float4 (Cr % 4 == 0 and a 16-byte aligned base)
__global__ __launch_bounds__(kSeImgThreads) void se_excite_kernel(const float* __restrict__ part, int nchunk,
                                                               const float* __restrict__ w1,
                                                               const float* __restrict__ b1,
                                                               const float* __restrict__ w2,
                                                               const float* __restrict__ b2, float* __restrict__ z,
                                                               float* __restrict__ h, float* __restrict__ g, int C,
                                                               int Cr, float hw, int w2v) {
  __shared__ __attribute__((aligned(16))) float sz[kMaxActC];
  __shared__ __attribute__((aligned(16))) float sh[kMaxSeCr];
  const int n = blockIdx.x, tid = threadIdx.x, C4 = C >> 2;
  // z = (the chunk partials in ascending chunk order) / HW
  const float* prow = part + (long long)n * nchunk * C;
  for (int q = tid; q < C4; q += kSeImgThreads) {
    float4 a = ld4(prow + 4 * q);
    for (int k = 1; k < nchunk; ++k) a = add4(a, ld4(prow + (long long)k * C + 4 * q));
    a = div4(a, hw);
    st4(sz + 4 * q, a);
    st4(z + (long long)n * C + 4 * q, a);
  }
  __syncthreads();
  // layer 1: one wave per hidden unit, lanes stride W1[j][:] by quads, butterfly sum
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < Cr; j += kSeImgThreads / kWave) {
    const float* wr = w1 + (long long)j * C;
    float4 a = f4zero();
    for (int q = lane; q < C4; q += kWave) a = fma4(ld4(wr + 4 * q), ld4(sz + 4 * q), a);
    const float s = wave_sum((a.x + a.y) + (a.z + a.w));
    if (lane == 0) {
      const float hv = relu_nan(s + b1[j]);
      sh[j] = hv;
      h[(long long)n * Cr + j] = hv;
    }
  }
  __syncthreads();
  // layer 2: one thread per output channel over its contiguous W2 row
  for (int c = tid; c < C; c += kSeImgThreads) {
    const float* wr = w2 + (long long)c * Cr;
    float a = 0.f;
    if (w2v) {
      float4 a4 = f4zero();
      for (int j = 0; j < Cr; j += 4) a4 = fma4(ld4(wr + j), ld4(sh + j), a4);
      a = (a4.x + a4.y) + (a4.z + a4.w);
    } else {
      for (int j = 0; j < Cr; ++j) a = fmaf(wr[j], sh[j], a);
    }
    g[(long long)n * C + c] = se_sigmoid(a + b2[c]);
  }
}

// Backward of the excitation for image n, from the chunk partials of sum_hw dz * u:
//   dg = s[n] * partials, da2 = dg g (1 - g), da1 = (W2^T da2) masked by h > 0,
//   dpool = (W1^T da1) / HW   (the squeeze's gradient, the same for every pixel of the image)
__global__ __launch_bounds__(kSeImgThreads) void se_excite_bwd_kernel(const float* __restrict__ part, int nchunk,
                                                                   const float* __restrict__ w1,
                                                                   const float* __restrict__ w2,
                                                                   const float* __restrict__ h,
                                                                   const float* __restrict__ g,
                                                                   const float* __restrict__ drop_scale,
                                                                   float* __restrict__ da2, float* __restrict__ da1,
                                                                   float* __restrict__ dpool, int C, int Cr,
                                                                   float hw) {
  __shared__ __attribute__((aligned(16))) float sda2[kMaxActC];
  __shared__ float sred[kSeImgThreads];
  __shared__ float sda1[kMaxSeCr];
  const int n = blockIdx.x, tid = threadIdx.x, C4 = C >> 2;
  const float s = drop_scale ? drop_scale[n] : 1.f;
  const float* prow = part + (long long)n * nchunk * C;
  for (int q = tid; q < C4; q += kSeImgThreads) {
    float4 a = ld4(prow + 4 * q);
    for (int k = 1; k < nchunk; ++k) a = add4(a, ld4(prow + (long long)k * C + 4 * q));
    if (drop_scale) a = scale4(a, s);
    const float4 gv = ld4(g + (long long)n * C + 4 * q);
    const float4 v = make_float4(a.x * gv.x * (1.f - gv.x), a.y * gv.y * (1.f - gv.y), a.z * gv.z * (1.f - gv.z),
                                 a.w * gv.w * (1.f - gv.w));
    st4(sda2 + 4 * q, v);
    st4(da2 + (long long)n * C + 4 * q, v);
  }
  __syncthreads();
  // dh[j] = sum_c W2[c][j] da2[c]: thread (j, row group) sums the channels RGj apart (consecutive
  // lanes read consecutive floats of a W2 row), then unit j's thread adds the row groups in order
  const int RGj = kSeImgThreads / Cr;  // Cr <= kMaxSeCr = 256
  const int rg = tid / Cr, j = tid - rg * Cr;
  float a = 0.f;
  if (rg < RGj)
    for (int c = rg; c < C; c += RGj) a = fmaf(w2[(long long)c * Cr + j], sda2[c], a);
  sred[tid] = a;
  __syncthreads();
  if (tid < Cr) {
    float t = sred[tid];
    for (int r = 1; r < RGj; ++r) t += sred[r * Cr + tid];
    const float v = h[(long long)n * Cr + tid] > 0.f ? t : 0.f;
    sda1[tid] = v;
    da1[(long long)n * Cr + tid] = v;
  }
  __syncthreads();
  for (int q = tid; q < C4; q += kSeImgThreads) {
    float4 acc = f4zero();
    for (int jj = 0; jj < Cr; ++jj) {
      const float d = sda1[jj];
      acc = fma4(ld4(w1 + (long long)jj * C + 4 * q), make_float4(d, d, d, d), acc);
    }
    st4(dpool + (long long)n * C + 4 * q, div4(acc, hw));
  }
}

// dW1[j][c] = sum_n da1[n][j] z[n][c], dW2[c][j] = sum_n da2[n][c] h[n][j], db1 = sum_n da1,
// db2 = sum_n da2: one thread per output element, the batch in ascending order.
__global__ __launch_bounds__(kSeThreads) void se_param_grad_kernel(const float* __restrict__ da1,
                                                                   const float* __restrict__ da2,
                                                                   const float* __restrict__ z,
                                                                   const float* __restrict__ h,
                                                                   float* __restrict__ dw1, float* __restrict__ db1,
                                                                   float* __restrict__ dw2, float* __restrict__ db2,
                                                                   int N, int C, int Cr) {
  const int i = blockIdx.x * kSeThreads + threadIdx.x;
  const int nw = C * Cr;
  float a = 0.f;
  if (i < nw) {
    const int j = i / C, c = i - j * C;
    for (int n = 0; n < N; ++n) a = fmaf(da1[(long long)n * Cr + j], z[(long long)n * C + c], a);
    dw1[i] = a;
  } else if (i < 2 * nw) {
    const int k = i - nw, c = k / Cr, j = k - c * Cr;
    for (int n = 0; n < N; ++n) a = fmaf(da2[(long long)n * C + c], h[(long long)n * Cr + j], a);
    dw2[k] = a;
  } else if (i < 2 * nw + Cr) {
    const int j = i - 2 * nw;
    for (int n = 0; n < N; ++n) a += da1[(long long)n * Cr + j];
    db1[j] = a;
  } else if (i < 2 * nw + Cr + C) {
    const int c = i - 2 * nw - Cr;
    for (int n = 0; n < N; ++n) a += da2[(long long)n * C + c];
    db2[c] = a;
  }
}

// ------------------------------------------------------------------ NHWC passes
// out = relu_nan((s[n] g[n][c]) u + r), publishing out's per-image / per-channel |max| (am.img != null:
// the f16x2 engine) so the next block's GEMMs take their operand scales from it. A workgroup writes one
// image, so its image maximum is the single slot 0 of the LDS window (img0 = n), and a thread's channel
// maxima stay in registers of its fixed quad until the end of the quad's pixels.
template <bool DROP>
__global__ __launch_bounds__(kSeThreads) void se_scale_act_kernel(const float* __restrict__ u,
                                                                  const float* __restrict__ r,
                                                                  const float* __restrict__ g,
                                                                  const float* __restrict__ drop_scale,
                                                                  float* __restrict__ out, int N, int HW, int C,
                                                                  int nchunk, int cpix, ActMaxOut am) {
  __shared__ ActMaxBlock<kMaxActC> sam;
  const SeWork w(HW, C, nchunk, cpix);
  const int tid = threadIdx.x;
  const bool want = am.img != nullptr;
  if (want) {
    sam.init(tid, kSeThreads);
    __syncthreads();
  }
  ImgRun run;
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    if (!(w.live && q < w.C4)) continue;
    float4 gs = ld4(g + (long long)w.n * C + 4 * q);
    if constexpr (DROP) gs = scale4(gs, drop_scale[w.n]);  // (a dropped image: 0 * u + r is r, bitwise)
    float4 cm = f4zero();
    const float* ub = u + w.img + 4 * q;
    const float* rb = r + w.img + 4 * q;
    float* ob = out + w.img + 4 * q;
    for (int p = w.p0 + w.row; p < w.p1; p += 4 * w.RG) {
      float4 uv[4], rv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long off = (long long)min(p + k * w.RG, w.p1 - 1) * C;  // past the end: reload, unused
        uv[k] = ld4(ub + off);
        rv[k] = ld4(rb + off);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p + k * w.RG >= w.p1) break;
        float4 zv = fma4(gs, uv[k], rv[k]);
        zv = make_float4(relu_nan(zv.x), relu_nan(zv.y), relu_nan(zv.z), relu_nan(zv.w));
        st4(ob + (long long)(p + k * w.RG) * C, zv);
        if (want) {
          run.add(w.n, absmax4(zv), sam, w.n, am);
          cm = absmax4(cm, zv);
        }
      }
    }
    if (want) sam.add_ch4(4 * q, cm);
  }
  if (want) {
    run.flush(sam, w.n, am);
    __syncthreads();
    sam.publish(am, w.n, N, 0, C, C, blockIdx.x % kActCopies, tid, kSeThreads);
  }
}

// du = dz (s[n] g[n][c]) + dpool[n][c], dz = gout * (out > 0); DRES: dr = dz (the shortcut's gradient)
template <bool DROP, bool DRES>
__global__ __launch_bounds__(kSeThreads) void se_bwd_apply_kernel(const float* __restrict__ gout,
                                                                  const float* __restrict__ out,
                                                                  const float* __restrict__ g,
                                                                  const float* __restrict__ dpool,
                                                                  const float* __restrict__ drop_scale,
                                                                  float* __restrict__ du, float* __restrict__ dr,
                                                                  int HW, int C, int nchunk, int cpix) {
  const SeWork w(HW, C, nchunk, cpix);
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    if (!(w.live && q < w.C4)) continue;
    float4 gs = ld4(g + (long long)w.n * C + 4 * q);
    if constexpr (DROP) gs = scale4(gs, drop_scale[w.n]);
    const float4 dp = ld4(dpool + (long long)w.n * C + 4 * q);
    const long long base = w.img + 4 * q;
    for (int p = w.p0 + w.row; p < w.p1; p += 4 * w.RG) {
      float4 gv[4], ov[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long off = base + (long long)min(p + k * w.RG, w.p1 - 1) * C;
        gv[k] = ld4(gout + off);
        ov[k] = ld4(out + off);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p + k * w.RG >= w.p1) break;
        const long long off = base + (long long)(p + k * w.RG) * C;
        const float4 dz = relu_route4(gv[k], ov[k]);
        st4(du + off, fma4(dz, gs, dp));
        if constexpr (DRES) st4(dr + off, dz);
      }
    }
  }
}

}  // namespace

SeSplit se_split(int N, int HW, int C, bool reduce, int cus) {
  const int TQ = std::min(C / 4, kSeThreads), RG = kSeThreads / TQ;
  // a reduction's chunk must be worth its partial row and its LDS combine; a pass only has to give every
  // row group a couple of pixels
  const int min_pix = reduce ? 64 : std::max(8, 2 * RG);
  const int want = (4 * cus + N - 1) / N;  // chunks per image for four workgroups per CU
  const int most = std::max(1, HW / min_pix);
  int nchunk = std::max(1, std::min(std::min(want, most), kSeMaxChunks));
  const int cpix = (HW + nchunk - 1) / nchunk;
  nchunk = (HW + cpix - 1) / cpix;  // no empty trailing chunk
  return SeSplit{nchunk, cpix};
}

void se_squeeze_launch(const float* u, int N, int HW, int C, SeSplit sp, float* part, hipStream_t st) {
  hipLaunchKernelGGL(se_squeeze_kernel, dim3(N * sp.nchunk), dim3(kSeThreads), 0, st, u, part, HW, C, sp.nchunk,
                     sp.cpix);
}

void se_excite_launch(const float* part, int nchunk, const float* w1, const float* b1, const float* w2,
                      const float* b2, int N, int HW, int C, int Cr, float* z, float* h, float* g, hipStream_t st) {
  const int w2v = (Cr % 4) == 0 && (reinterpret_cast<uintptr_t>(w2) & 15) == 0;
  hipLaunchKernelGGL(se_excite_kernel, dim3(N), dim3(kSeImgThreads), 0, st, part, nchunk, w1, b1, w2, b2, z, h, g, C, Cr,
                     (float)HW, w2v);
}

void se_scale_act_launch(const float* u, const float* r, const float* g, const float* drop_scale, float* out, int N,
                         int HW, int C, SeSplit sp, ActMaxOut am, hipStream_t st) {
  hipLaunchKernelGGL(drop_scale ? se_scale_act_kernel<true> : se_scale_act_kernel<false>, dim3(N * sp.nchunk),
                     dim3(kSeThreads), 0, st, u, r, g, drop_scale, out, N, HW, C, sp.nchunk, sp.cpix, am);
}

void se_bwd_reduce_launch(const float* gout, const float* out, const float* u, int N, int HW, int C, SeSplit sp,
                          float* part, hipStream_t st) {
  hipLaunchKernelGGL(se_bwd_reduce_kernel, dim3(N * sp.nchunk), dim3(kSeThreads), 0, st, gout, out, u, part, HW, C,
                     sp.nchunk, sp.cpix);
}

void se_excite_bwd_launch(const float* part, int nchunk, const float* w1, const float* w2, const float* h,
                          const float* g, const float* drop_scale, int N, int HW, int C, int Cr, float* da2,
                          float* da1, float* dpool, hipStream_t st) {
  hipLaunchKernelGGL(se_excite_bwd_kernel, dim3(N), dim3(kSeImgThreads), 0, st, part, nchunk, w1, w2, h, g, drop_scale,
                     da2, da1, dpool, C, Cr, (float)HW);
}

void se_param_grad_launch(const float* da1, const float* da2, const float* z, const float* h, int N, int C, int Cr,
                          float* dw1, float* db1, float* dw2, float* db2, hipStream_t st) {
  const int total = 2 * C * Cr + Cr + C;
  hipLaunchKernelGGL(se_param_grad_kernel, dim3((total + kSeThreads - 1) / kSeThreads), dim3(kSeThreads), 0, st, da1,
                     da2, z, h, dw1, db1, dw2, db2, N, C, Cr);
}

void se_bwd_apply_launch(const float* gout, const float* out, const float* g, const float* dpool,
                         const float* drop_scale, float* du, float* dr, int N, int HW, int C, SeSplit sp,
                         hipStream_t st) {
  auto k = drop_scale ? (dr ? se_bwd_apply_kernel<true, true> : se_bwd_apply_kernel<true, false>)
                      : (dr ? se_bwd_apply_kernel<false, true> : se_bwd_apply_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(N * sp.nchunk), dim3(kSeThreads), 0, st, gout, out, g, dpool, drop_scale, du, dr, HW, C,
                     sp.nchunk, sp.cpix);
}

}  // namespace cdp
