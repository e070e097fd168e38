// GroupNorm of a conv output, fused with the rest of a residual block's tail (Wu & He, "Group Normalization"):
//   out = act(s[n] * ((y - mean[n,g]) * rstd[n,g] * gamma[c] + beta[c]) + r)
// y, r, out NHWC fp32 [N][HW][C]; mean and biased variance over the Cg * HW values of (image n, group g),
// Cg = C / G, rstd = 1 / sqrt(var + eps); act the NaN-propagating ReLU or the identity; r the optional
// shortcut and s the optional stochastic-depth row (with r only). Backward, with dz = gout * (out > 0) (or gout),
// t = s[n] dz and xhat = (y - mean) rstd:
//   s1[n,c] = sum_hw t, s2[n,c] = sum_hw t xhat, dbeta = sum_n s1, dgamma = sum_n s2,
//   a[n,g] = sum_{c in g} gamma s1, b[n,g] = sum_{c in g} gamma s2,
//   dy = rstd (gamma t - (a + xhat b) / (Cg HW)), dr = dz.
//
// All of it is memory-bound NHWC streaming plus reductions of Cg * HW values per (image, group). The matrix
// instructions do not fit: there is no product of two operands with a shared inner dimension here, only sums of
// one stream (the statistics) or of an elementwise product (s2), so an MFMA would multiply by a matrix of ones
// and spend its tile on padding. The sums are plain FMAs behind 16-byte loads.
//
// Work split (the split of se.hip, se_split): a workgroup owns pixels [chunk * cpix, (chunk + 1) * cpix) of ONE
// image. Thread t owns channel quad t % TQ (TQ = min(C / 4, 256); quads TQ apart when C / 4 > 256) and walks
// the pixels of row group t / TQ, RG = 256 / TQ apart, so consecutive lanes read consecutive 16-byte words.
// A quad lies in one group (Cg % 4 == 0) or holds 2 or 4 whole groups (Cg = 2, 1); the launchers take nothing
// else.
//
// Forward, two launches: gn_stats_kernel leaves one (mean, M2) pair per (image, chunk, channel); gn_apply_kernel
// opens with a prologue in which EVERY workgroup of an image merges that image's partials -- the chunks of a
// channel in ascending order, then the channels of a group, both by Chan's update -- into an LDS table of
// mean / rstd per group. There is no finalize launch, and all workgroups of an image derive the same bits.
// Backward, three launches: gn_bwd_reduce_kernel (s1, s2 per chunk), gn_param_grad_kernel (dgamma, dbeta) and
// gn_bwd_apply_kernel, whose prologue builds a and b of its image in LDS the same way.
//
// Variance: a chunk's sums are taken of d = y - K with K the chunk's own first pixel of the channel, so
// M2 = sum d^2 - (sum d)^2 / n cancels at the scale of the spread, not of the mean (y = 1000 + randn keeps
// 1e-6; a plain sum of squares loses the variance there), and the merges never subtract squares.
//
// Determinism: every sum runs in a fixed order (a thread over its pixels, the row groups through LDS, the chunks
// ascending, the slices of a group ascending). No float atomics; the only atomics are the integer max of the
// act-max publication (act_max.h), which is order-independent. Nothing synchronises with the host.
#include <algorithm>

#include "act_max.h"
#include "common.h"
#include "kernels.h"

namespace cdp {

namespace {

static_assert(kMaxGnC == kMaxActC, "the apply passes keep their channel maxima in an ActMaxBlock<kMaxActC>");
constexpr int kGnThreads = 256;  // se_split's TQ / RG assume 256 threads per workgroup too
constexpr int kGnSlices = 64;    // threads that share one group's channels in a prologue, at most
constexpr int kPgCh = 16;        // gn_param_grad_kernel: channels per workgroup (x 2 planes x 8 row groups)

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 relu4(float4 v) {
  return make_float4(relu_nan(v.x), relu_nan(v.y), relu_nan(v.z), relu_nan(v.w));
}
// gout where the block's ReLU passed (out > 0), else 0
__device__ __forceinline__ float4 relu_route4(float4 gout, float4 out) {
  return make_float4(out.x > 0.f ? gout.x : 0.f, out.y > 0.f ? gout.y : 0.f, out.z > 0.f ? gout.z : 0.f,
                     out.w > 0.f ? gout.w : 0.f);
}
// four scalar loads: a parameter's arena slot need not be 16-byte aligned
__device__ __forceinline__ float4 ld4s(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }
// the per-group entries of channel quad c0 .. c0 + 3 (one group when Cg % 4 == 0, else 2 or 4)
__device__ __forceinline__ float4 quad_groups(const float* tab, int c0, int Cg) {
  if (Cg >= 4) {
    const float v = tab[c0 / Cg];
    return make_float4(v, v, v, v);
  }
  return make_float4(tab[c0 / Cg], tab[(c0 + 1) / Cg], tab[(c0 + 2) / Cg], tab[(c0 + 3) / Cg]);
}

// A workgroup's place in the split: image n, pixels [p0, p1) of it, and the thread's quad / row group.
struct GnWork {
  int n, p0, p1, C4, TQ, RG, cq, row;
  bool live;      // the thread has a row group (256 need not be a multiple of TQ)
  long long img;  // float offset of image n
  __device__ GnWork(int HW, int C, int nchunk, int cpix) {
    n = blockIdx.x / nchunk;
    const int ch = blockIdx.x - n * nchunk;
    p0 = ch * cpix;
    p1 = min(HW, p0 + cpix);
    C4 = C >> 2;
    TQ = min(C4, kGnThreads);
    RG = kGnThreads / TQ;
    row = threadIdx.x / TQ;
    cq = threadIdx.x - row * TQ;
    live = row < RG;
    img = (long long)n * HW * C;
  }
};

// Count, mean and sum of squared deviations of a set of values; Chan's update joins two sets (n > 0 in both).
struct Mom {
  float n, mean, m2;
};
__device__ __forceinline__ Mom chan(Mom a, Mom b) {
  const float n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
  return Mom{n, fmaf(d, f, a.mean), a.m2 + b.m2 + d * d * (a.n * f)};
}
// The pair the backward prologue folds: plain sums.
struct Pair {
  float a, b;
};
__device__ __forceinline__ Pair chan(Pair x, Pair y) { return Pair{x.a + y.a, x.b + y.b}; }

// Threads per group of a prologue's channel fold: a power of two, at most Cg, kGnSlices and 256 / G.
__device__ __forceinline__ int gn_slices(int G, int Cg) {
  int S = 1;
  while (2 * S <= Cg && 2 * S * G <= kGnThreads && 2 * S <= kGnSlices) S *= 2;
  return S;
}

// Fold the channels of every group: slice j of group g joins channels g Cg + j, + S, ... in ascending order
// (`leaf(c)`), then the group's first thread joins its S slices in ascending order and hands the result to
// `done(g, v)`. `sl` holds one value per thread. Ends with a barrier.
template <class T, class Leaf, class Done>
__device__ __forceinline__ void gn_fold_groups(T* sl, int G, int Cg, Leaf leaf, Done done) {
  const int S = gn_slices(G, Cg), tid = threadIdx.x;
  for (int i0 = 0; i0 < G * S; i0 += kGnThreads) {  // (one round unless S == 1 and G > 256)
    const int i = i0 + tid, g = i / S, j = i - g * S;
    if (i < G * S) {
      const int c0 = g * Cg;
      T v = leaf(c0 + j);
      for (int c = j + S; c < Cg; c += S) v = chan(v, leaf(c0 + c));
      if (S == 1) done(g, v);
      else sl[tid] = v;
    }
    if (S > 1) {
      __syncthreads();
      if (i < G * S && j == 0) {
        T v = sl[tid];
        for (int k = 1; k < S; ++k) v = chan(v, sl[tid + k]);
        done(g, v);
      }
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ forward statistics
// part[n][chunk][0][c] = mean, part[n][chunk][1][c] = M2 of channel c over the chunk's pixels (the count is the
// chunk's length). Four independent accumulator pairs per thread keep four 16-byte loads in flight; they and
// the row groups (LDS) are combined in a fixed order. Every row group of a quad shifts by the same K.
__global__ __launch_bounds__(kGnThreads) void gn_stats_kernel(const float* __restrict__ y, float* __restrict__ part,
                                                              int HW, int C, int nchunk, int cpix) {
  __shared__ float4 red[2][kGnThreads];
  const GnWork w(HW, C, nchunk, cpix);
  const int tid = threadIdx.x;
  float* dst = part + (long long)blockIdx.x * 2 * C;
  const float cnt = (float)(w.p1 - w.p0);
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    float4 sd[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    float4 sq[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    float4 K = f4zero();
    if (w.live && q < w.C4) {
      const float* yb = y + w.img + 4 * q;
      K = ld4(yb + (long long)w.p0 * C);
      int p = w.p0 + w.row;
      for (; p + 3 * w.RG < w.p1; p += 4 * w.RG) {
        float4 d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = sub4(ld4(yb + (long long)(p + k * w.RG) * C), K);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          sd[k] = add4(sd[k], d[k]);
          sq[k] = fma4(d[k], d[k], sq[k]);
        }
      }
      for (; p < w.p1; p += w.RG) {
        const float4 d = sub4(ld4(yb + (long long)p * C), K);
        sd[0] = add4(sd[0], d);
        sq[0] = fma4(d, d, sq[0]);
      }
    }
    red[0][tid] = add4(add4(sd[0], sd[1]), add4(sd[2], sd[3]));
    red[1][tid] = add4(add4(sq[0], sq[1]), add4(sq[2], sq[3]));
    __syncthreads();
    if (tid < w.TQ && q < w.C4) {  // row group 0's threads (they hold K): the row groups in ascending order
      float4 a = red[0][tid], b = red[1][tid];
      for (int r = 1; r < w.RG; ++r) {
        a = add4(a, red[0][r * w.TQ + tid]);
        b = add4(b, red[1][r * w.TQ + tid]);
      }
      const float4 m = make_float4(a.x / cnt, a.y / cnt, a.z / cnt, a.w / cnt);
      st4(dst + 4 * q, add4(K, m));
      st4(dst + C + 4 * q, make_float4(fmaf(-a.x, m.x, b.x), fmaf(-a.y, m.y, b.y), fmaf(-a.z, m.z, b.z),
                                       fmaf(-a.w, m.w, b.w)));
    }
    __syncthreads();
  }
}

// The act-max bookkeeping both apply passes share: a workgroup writes one image, so its image maximum is slot 0
// of the LDS window (img0 = n), and a thread's channel maxima stay in registers until its quad's pixels end.
struct GnActMax {
  ActMaxBlock<kMaxActC>& sam;
  const ActMaxOut& am;
  ImgRun run;
  bool want;
  __device__ GnActMax(ActMaxBlock<kMaxActC>& s, const ActMaxOut& o) : sam(s), am(o), want(o.img != nullptr) {
    if (want) sam.init(threadIdx.x, kGnThreads);  // (a barrier of the prologue follows before any add)
  }
  __device__ __forceinline__ void add(int n, float4 v, float4& cm) {
    if (want) {
      run.add(n, absmax4(v), sam, n, am);
      cm = absmax4(cm, v);
    }
  }
  __device__ __forceinline__ void quad_done(int c0, float4 cm) {
    if (want) sam.add_ch4(c0, cm);
  }
  __device__ void publish(int n, int N, int C) {
    if (!want) return;
    run.flush(sam, n, am);
    __syncthreads();
    sam.publish(am, n, N, 0, C, C, blockIdx.x % kActCopies, threadIdx.x, kGnThreads);
  }
};

// ------------------------------------------------------------------ forward apply
// part / rchunk / rcpix: gn_stats_kernel's partials and their split. Chunk 0 of an image stores its table to
// stats[n][g] = (mean, rstd) for the backward.
template <bool RELU, bool RES>
__global__ __launch_bounds__(kGnThreads) void gn_apply_kernel(
    const float* __restrict__ y, const float* __restrict__ r, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ drop_scale, const float* __restrict__ part, int rchunk,
    int rcpix, float* __restrict__ stats, float* __restrict__ out, int N, int HW, int C, int G, float eps, int nchunk,
    int cpix, ActMaxOut am) {
  extern __shared__ float s_tab[];  // gn_tab_bytes(C, G): sized by the layer, so narrow layers keep their occupancy
  float *s_cm = s_tab, *s_c2 = s_tab + C;                  // a channel's mean and M2 over the image
  float *s_mean = s_tab + 2 * C, *s_rstd = s_mean + G;  // per group
  __shared__ Mom s_sl[kGnThreads];
  __shared__ ActMaxBlock<kMaxActC> sam;
  const GnWork w(HW, C, nchunk, cpix);
  const int tid = threadIdx.x, Cg = C / G;
  GnActMax amx(sam, am);
  // prologue: the image's chunks per channel in ascending order, then the channels of each group
  const float* prow = part + (long long)w.n * rchunk * 2 * C;
  for (int c = tid; c < C; c += kGnThreads) {
    Mom m{(float)min(HW, rcpix), prow[c], prow[C + c]};
    for (int k = 1; k < rchunk; ++k) {
      const float* pk = prow + (long long)k * 2 * C;
      m = chan(m, Mom{(float)(min(HW, (k + 1) * rcpix) - k * rcpix), pk[c], pk[C + c]});
    }
    s_cm[c] = m.mean;
    s_c2[c] = m.m2;
  }
  __syncthreads();
  const bool first = w.p0 == 0;
  float* srow = stats + (long long)w.n * G * 2;
  gn_fold_groups<Mom>(
      s_sl, G, Cg, [&](int c) { return Mom{(float)HW, s_cm[c], s_c2[c]}; },
      [&](int g, Mom m) {
        const float rstd = 1.f / sqrtf(fmaxf(m.m2 / m.n, 0.f) + eps);  // (a NaN in the group is in the mean)
        s_mean[g] = m.mean;
        s_rstd[g] = rstd;
        if (first) {
          srow[2 * g] = m.mean;
          srow[2 * g + 1] = rstd;
        }
      });
  // body: normalise, affine, scale row, residual, ReLU, store
  const float s = drop_scale ? drop_scale[w.n] : 1.f;  // (1: the products below are exact)
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    if (!(w.live && q < w.C4)) continue;
    const float4 mean = quad_groups(s_mean, 4 * q, Cg);
    const float4 rg = mul4(quad_groups(s_rstd, 4 * q, Cg), ld4s(gamma + 4 * q));
    const float4 bt = ld4s(beta + 4 * q);
    const float4 s4 = make_float4(s, s, s, s);
    float4 cm = f4zero();
    const float* yb = y + w.img + 4 * q;
    const float* rb = RES ? r + w.img + 4 * q : nullptr;
    float* ob = out + w.img + 4 * q;
    for (int p = w.p0 + w.row; p < w.p1; p += 4 * w.RG) {
      float4 yv[4], rv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long off = (long long)min(p + k * w.RG, w.p1 - 1) * C;  // past the end: reload, unused
        yv[k] = ld4(yb + off);
        if constexpr (RES) rv[k] = ld4(rb + off);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p + k * w.RG >= w.p1) break;
        float4 v = fma4(sub4(yv[k], mean), rg, bt);
        if constexpr (RES) v = fma4(s4, v, rv[k]);  // (a dropped image: 0 * v + r is r, bitwise)
        if constexpr (RELU) v = relu4(v);
        st4(ob + (long long)(p + k * w.RG) * C, v);
        amx.add(w.n, v, cm);
      }
    }
    amx.quad_done(4 * q, cm);
  }
  amx.publish(w.n, N, C);
}

// ------------------------------------------------------------------ backward reductions
// part[n][chunk][0][c] = s1, [1][c] = s2 over the chunk's pixels, the stochastic-depth scale included.
template <bool RELU>
__global__ __launch_bounds__(kGnThreads) void gn_bwd_reduce_kernel(
    const float* __restrict__ gout, const float* __restrict__ out, const float* __restrict__ y,
    const float* __restrict__ stats, const float* __restrict__ drop_scale, float* __restrict__ part, int HW, int C,
    int G, int nchunk, int cpix) {
  __shared__ float4 red[2][kGnThreads];
  const GnWork w(HW, C, nchunk, cpix);
  const int tid = threadIdx.x, Cg = C / G;
  const float* srow = stats + (long long)w.n * G * 2;
  const float s = drop_scale ? drop_scale[w.n] : 1.f;
  float* dst = part + (long long)blockIdx.x * 2 * C;
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    float4 a1[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    float4 a2[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    if (w.live && q < w.C4) {
      float4 mean, rstd;
      {
        const int c0 = 4 * q;
        const int g0 = c0 / Cg, g1 = (c0 + 1) / Cg, g2 = (c0 + 2) / Cg, g3 = (c0 + 3) / Cg;
        mean = make_float4(srow[2 * g0], srow[2 * g1], srow[2 * g2], srow[2 * g3]);
        rstd = make_float4(srow[2 * g0 + 1], srow[2 * g1 + 1], srow[2 * g2 + 1], srow[2 * g3 + 1]);
      }
      const long long base = w.img + 4 * q;
      auto step = [&](int p, float4& s1, float4& s2) {
        const long long off = base + (long long)p * C;
        float4 dz = ld4(gout + off);
        if constexpr (RELU) dz = relu_route4(dz, ld4(out + off));
        const float4 xh = mul4(sub4(ld4(y + off), mean), rstd);
        s1 = add4(s1, dz);
        s2 = fma4(dz, xh, s2);
      };
      int p = w.p0 + w.row;
      for (; p + 3 * w.RG < w.p1; p += 4 * w.RG) {
#pragma unroll
        for (int k = 0; k < 4; ++k) step(p + k * w.RG, a1[k], a2[k]);
      }
      for (; p < w.p1; p += w.RG) step(p, a1[0], a2[0]);
    }
    red[0][tid] = add4(add4(a1[0], a1[1]), add4(a1[2], a1[3]));
    red[1][tid] = add4(add4(a2[0], a2[1]), add4(a2[2], a2[3]));
    __syncthreads();
    if (tid < w.TQ && q < w.C4) {
      float4 a = red[0][tid], b = red[1][tid];
      for (int r = 1; r < w.RG; ++r) {
        a = add4(a, red[0][r * w.TQ + tid]);
        b = add4(b, red[1][r * w.TQ + tid]);
      }
      st4(dst + 4 * q, scale4(a, s));
      st4(dst + C + 4 * q, scale4(b, s));
    }
    __syncthreads();
  }
}

// dbeta[c] / dgamma[c] = the rows (image, chunk) of plane 0 / 1: a workgroup owns kPgCh channels of both planes,
// eight row groups each sum the rows 8 apart in ascending order, then the row groups are added in order.
__global__ __launch_bounds__(kGnThreads) void gn_param_grad_kernel(const float* __restrict__ part, int rows, int C,
                                                                   float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
  __shared__ float red[kGnThreads];
  constexpr int kCols = 2 * kPgCh, kRows = kGnThreads / kCols;
  const int tid = threadIdx.x, col = tid % kCols, rg = tid / kCols;
  const int plane = col / kPgCh, c = blockIdx.x * kPgCh + col % kPgCh;
  float a = 0.f;
  if (c < C)
    for (int row = rg; row < rows; row += kRows) a += part[((long long)row * 2 + plane) * C + c];
  red[tid] = a;
  __syncthreads();
  if (tid < kCols && c < C) {
    float t = red[tid];
    for (int r = 1; r < kRows; ++r) t += red[r * kCols + tid];
    (plane ? dgamma : dbeta)[c] = t;
  }
}

// ------------------------------------------------------------------ backward apply
// dy = rstd (gamma t - (a + xhat b) / (Cg HW)), t = s dz; DRES: dr = dz. Publishes dy's act maxima: per image
// they scale the data-gradient GEMM of the conv before, per channel its weight-gradient GEMM.
template <bool RELU, bool DRES>
__global__ __launch_bounds__(kGnThreads) void gn_bwd_apply_kernel(
    const float* __restrict__ gout, const float* __restrict__ out, const float* __restrict__ y,
    const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ drop_scale,
    const float* __restrict__ part, int rchunk, float* __restrict__ dy, float* __restrict__ dr, int N, int HW, int C,
    int G, int nchunk, int cpix, ActMaxOut am) {
  extern __shared__ float s_tab[];                 // gn_tab_bytes(C, G)
  float *s_1 = s_tab, *s_2 = s_tab + C;            // gamma s1, gamma s2 of the image per channel
  float *s_a = s_tab + 2 * C, *s_b = s_a + G;  // a / (Cg HW), b / (Cg HW) per group
  __shared__ Pair s_sl[kGnThreads];
  __shared__ ActMaxBlock<kMaxActC> sam;
  const GnWork w(HW, C, nchunk, cpix);
  const int tid = threadIdx.x, Cg = C / G;
  GnActMax amx(sam, am);
  const float* prow = part + (long long)w.n * rchunk * 2 * C;
  for (int c = tid; c < C; c += kGnThreads) {
    float a = prow[c], b = prow[C + c];
    for (int k = 1; k < rchunk; ++k) {
      a += prow[(long long)k * 2 * C + c];
      b += prow[(long long)k * 2 * C + C + c];
    }
    const float gm = gamma[c];
    s_1[c] = gm * a;
    s_2[c] = gm * b;
  }
  __syncthreads();
  const float inv = 1.f / ((float)Cg * (float)HW);
  gn_fold_groups<Pair>(
      s_sl, G, Cg, [&](int c) { return Pair{s_1[c], s_2[c]}; },
      [&](int g, Pair v) {
        s_a[g] = v.a * inv;
        s_b[g] = v.b * inv;
      });
  const float* srow = stats + (long long)w.n * G * 2;
  const float s = drop_scale ? drop_scale[w.n] : 1.f;
  for (int q0 = 0; q0 < w.C4; q0 += w.TQ) {
    const int q = q0 + w.cq;
    if (!(w.live && q < w.C4)) continue;
    const int c0 = 4 * q;
    const int g0 = c0 / Cg, g1 = (c0 + 1) / Cg, g2 = (c0 + 2) / Cg, g3 = (c0 + 3) / Cg;
    const float4 mean = make_float4(srow[2 * g0], srow[2 * g1], srow[2 * g2], srow[2 * g3]);
    const float4 rstd = make_float4(srow[2 * g0 + 1], srow[2 * g1 + 1], srow[2 * g2 + 1], srow[2 * g3 + 1]);
    const float4 av = quad_groups(s_a, c0, Cg), bv = quad_groups(s_b, c0, Cg);
    const float4 gs = scale4(ld4s(gamma + c0), s);  // gamma t = (gamma s) dz
    float4 cm = f4zero();
    const long long base = w.img + c0;
    for (int p = w.p0 + w.row; p < w.p1; p += 4 * w.RG) {
      float4 gv[4], ov[4], yv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long off = base + (long long)min(p + k * w.RG, w.p1 - 1) * C;
        gv[k] = ld4(gout + off);
        if constexpr (RELU) ov[k] = ld4(out + off);
        yv[k] = ld4(y + off);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p + k * w.RG >= w.p1) break;
        const long long off = base + (long long)(p + k * w.RG) * C;
        float4 dz = gv[k];
        if constexpr (RELU) dz = relu_route4(dz, ov[k]);
        const float4 xh = mul4(sub4(yv[k], mean), rstd);
        const float4 v = mul4(rstd, sub4(mul4(gs, dz), fma4(xh, bv, av)));
        st4(dy + off, v);
        if constexpr (DRES) st4(dr + off, dz);
        amx.add(w.n, v, cm);
      }
    }
    amx.quad_done(c0, cm);
  }
  amx.publish(w.n, N, C);
}

// LDS table of a prologue: two floats per channel and two per group (at most 32 KB, C = G = 2048)
size_t gn_tab_bytes(int C, int G) { return sizeof(float) * 2 * ((size_t)C + G); }

}  // namespace

void gn_stats_launch(const float* y, int N, int HW, int C, SeSplit sp, float* part, hipStream_t st) {
  hipLaunchKernelGGL(gn_stats_kernel, dim3(N * sp.nchunk), dim3(kGnThreads), 0, st, y, part, HW, C, sp.nchunk,
                     sp.cpix);
}

void gn_apply_launch(const float* y, const float* r, const float* gamma, const float* beta, const float* drop_scale,
                     const float* part, SeSplit rs, float* stats, float* out, int N, int HW, int C, int G, float eps,
                     bool relu, SeSplit sp, ActMaxOut am, hipStream_t st) {
  auto k = relu ? (r ? gn_apply_kernel<true, true> : gn_apply_kernel<true, false>)
                : (r ? gn_apply_kernel<false, true> : gn_apply_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(N * sp.nchunk), dim3(kGnThreads), gn_tab_bytes(C, G), st, y, r, gamma, beta, drop_scale,
                     part, rs.nchunk, rs.cpix, stats, out, N, HW, C, G, eps, sp.nchunk, sp.cpix, am);
}

void gn_bwd_reduce_launch(const float* gout, const float* out, const float* y, const float* stats,
                          const float* drop_scale, int N, int HW, int C, int G, SeSplit sp, float* part,
                          hipStream_t st) {
  hipLaunchKernelGGL(out ? gn_bwd_reduce_kernel<true> : gn_bwd_reduce_kernel<false>, dim3(N * sp.nchunk),
                     dim3(kGnThreads), 0, st, gout, out, y, stats, drop_scale, part, HW, C, G, sp.nchunk, sp.cpix);
}

void gn_param_grad_launch(const float* part, int rows, int C, float* dgamma, float* dbeta, hipStream_t st) {
  hipLaunchKernelGGL(gn_param_grad_kernel, dim3((C + kPgCh - 1) / kPgCh), dim3(kGnThreads), 0, st, part, rows, C,
                     dgamma, dbeta);
}

void gn_bwd_apply_launch(const float* gout, const float* out, const float* y, const float* stats, const float* gamma,
                         const float* drop_scale, const float* part, int rchunk, float* dy, float* dr, int N, int HW,
                         int C, int G, SeSplit sp, ActMaxOut am, hipStream_t st) {
  auto k = out ? (dr ? gn_bwd_apply_kernel<true, true> : gn_bwd_apply_kernel<true, false>)
               : (dr ? gn_bwd_apply_kernel<false, true> : gn_bwd_apply_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(N * sp.nchunk), dim3(kGnThreads), gn_tab_bytes(C, G), st, gout, out, y, stats, gamma,
                     drop_scale, part, rchunk, dy, dr, N, HW, C, G, sp.nchunk, sp.cpix, am);
}

}  // namespace cdp
