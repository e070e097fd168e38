// Small fused kernels: softmax and binary cross-entropy (fwd / bwd / accuracy), fused SGD, CIFAR-style
// augmentation, weight transpose for conv data-gradients, stack-mean for the gather/scatter
// strategy, and generic scale / channel-sum helpers. gfx950, wave64.
//
// Reference anchors:
//   CrossEntropyLoss            /root/reference/src/Part 1/main.py:110,39
//   accuracy (max(1), eq, sum)  /root/reference/src/Part 1/main.py:70-71
//   optim.SGD(lr .1, mom .9, wd 1e-4)   /root/reference/src/Part 1/main.py:114-115
//   RandomCrop(32,4)+HFlip+Normalize    /root/reference/src/Part 1/main.py:82-93
//   torch.mean(torch.stack(inputs), 0)  /root/reference/src/Part 2a/main.py:122
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "act_max.h"
#include "common.h"
#include "erase.h"
#include "grad_clip.h"
#include "lars.h"
#include "kernels.h"
#include "mix.h"
#include "rrc.h"
#include "step_common.h"
#include "x3_common.h"

namespace cdp {
namespace {

// ------------------------------------------------------------------ cross-entropy
// One block of 1024 threads. Narrow rows (C <= 64, e.g. CIFAR's 10 classes): one row per thread;
// wide rows (ImageNet's 1000): one row per wave. Per-row loss = logsumexp - logit[target]; the mean
// (fp64 block reduction, deterministic) and the top-1 correct count are written once.
//
// LS (label smoothing eps > 0, target distribution (1 - eps) onehot(t) + eps / C):
//   loss = logsumexp(z) - (1 - eps) z_t - (eps / C) sum_c z_c
//        = log(sum_c exp(z_c - mx)) + (1 - eps) (mx - z_t) - (eps / C) sum_c (z_c - mx)
// TK (topk > 1): a row is correct when rank < topk, rank = #{c : z_c > z_t, or z_c == z_t and c < t}
// (ties to the lower index, the argmax path's first-occurrence rule); not correct with a target out
// of range or a NaN target logit. Without LS / TK the instantiation is the plain kernel: eps and
// topk are not read.
__device__ __forceinline__ float xent_ls_row(float lse_rel, float mx, float zt, float sz, float eps, int C) {
  return lse_rel + (1.f - eps) * (mx - zt) - (eps / (float)C) * sz;
}
__device__ __forceinline__ int xent_above(float v, int c, float zt, int t) {
  return (v > zt || (v == zt && c < t)) ? 1 : 0;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// MIX (a second target per row, tgt_b, and a device-side weight lam[0]: mixup / CutMix):
//   loss = lam CE_eps(z, t_a) + (1 - lam) CE_eps(z, t_b)
//        = logsumexp(z) - (1 - eps) (lam z_ta + (1 - lam) z_tb) - (eps / C) sum_c z_c
// in the same max-relative form; either target out of range poisons the loss. No correct count.
template <bool LS>
__device__ __forceinline__ float xent_mix_row(float lse_rel, float mx, float zta, float ztb, float lam, float sz,
                                              float eps, int C) {
  const float d = lam * (mx - zta) + (1.f - lam) * (mx - ztb);
  return LS ? lse_rel + (1.f - eps) * d - (eps / (float)C) * sz : lse_rel + d;
}

template <bool LS, bool TK, bool MIX>
__global__ __launch_bounds__(1024) void xent_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ tgt,
                                                       int B, int C, float* __restrict__ loss,
                                                       long long* __restrict__ correct, float* __restrict__ sum_out,
                                                       float eps, int topk, const long long* __restrict__ tgt_b,
                                                       const float* __restrict__ lam_p) {
  __shared__ double red[16];
  __shared__ int redc[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  double acc = 0.0;
  int nc = 0;
  float lam = 1.f;
  if (MIX) lam = lam_p[0];
  if (C <= 64) {
    for (int r = tid; r < B; r += 1024) {
      const float* row = logits + (long long)r * C;
      float mx = row[0];
      int am = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > mx) { mx = v; am = c; }
      }
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(row[c] - mx);
      const long long t = tgt[r];
      const bool tok = t >= 0 && t < C;  // out-of-range targets poison the loss instead of reading OOB
      if (MIX) {
        const long long tb = tgt_b[r];
        const bool ok = tok && tb >= 0 && tb < C;
        float sz = 0.f;
        if (LS)
          for (int c = 0; c < C; ++c) sz += row[c] - mx;
        acc += ok ? (double)xent_mix_row<LS>(logf(se), mx, row[t], row[tb], lam, sz, eps, C) : (double)NAN;
      } else if (LS) {
        float sz = 0.f;
        for (int c = 0; c < C; ++c) sz += row[c] - mx;
        acc += tok ? (double)xent_ls_row(logf(se), mx, row[t], sz, eps, C) : (double)NAN;
      } else {
        acc += tok ? (double)(logf(se) + mx - row[t]) : (double)NAN;
      }
      if (TK) {
        if (tok) {
          const float zt = row[t];
          int rank = 0;
          for (int c = 0; c < C; ++c) rank += xent_above(row[c], c, zt, (int)t);
          nc += (zt == zt && rank < topk) ? 1 : 0;
        }
      } else {
        nc += (tok && am == (int)t) ? 1 : 0;
      }
    }
  } else if (C <= 1024) {
    // a wave's rows r = wid + 16 k (the loop below's assignment and order) four at a time, every
    // logit of the four loaded before the first is reduced: one memory round trip per four rows
    // (ResNet's 1000 classes: 40 -> a few us per call)
    constexpr int RB = 4, J = 16;
    for (int rb = wid; rb < B; rb += 16 * RB) {
      float v[RB][J];
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const int r = rb + 16 * k;
        const float* row = logits + (long long)(r < B ? r : 0) * C;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int c = lane + 64 * j;
          v[k][j] = (r < B && c < C) ? row[c] : -INFINITY;
        }
      }
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const int r = rb + 16 * k;
        if (r >= B) break;
        float mx = -INFINITY;
        int am = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (v[k][j] > mx) { mx = v[k][j]; am = lane + 64 * j; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float omx = __shfl_xor(mx, o, kWave);
          const int oam = __shfl_xor(am, o, kWave);
          if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
        }
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (lane + 64 * j < C) se += expf(v[k][j] - mx);
        se = wave_sum(se);
        float sz = 0.f;
        if (LS) {
#pragma unroll
          for (int j = 0; j < J; ++j)
            if (lane + 64 * j < C) sz += v[k][j] - mx;
          sz = wave_sum(sz);
        }
        int rank = 0;
        bool tkok = false;
        if (TK) {
          // every lane reads the row's target and target logit (one address: a broadcast load)
          const long long t = tgt[r];
          if (t >= 0 && t < C) {
            const float zt = logits[(long long)r * C + t];
            tkok = zt == zt;
#pragma unroll
            for (int j = 0; j < J; ++j)
              if (lane + 64 * j < C) rank += xent_above(v[k][j], lane + 64 * j, zt, (int)t);
          }
          rank = wave_sum_i(rank);
        }
        if (lane == 0) {
          const long long t = tgt[r];
          const bool tok = t >= 0 && t < C;
          if (MIX) {
            const long long tb = tgt_b[r];
            const float* zr = logits + (long long)r * C;
            acc += (tok && tb >= 0 && tb < C) ? (double)xent_mix_row<LS>(logf(se), mx, zr[t], zr[tb], lam, sz, eps, C)
                                              : (double)NAN;
          } else if (LS)
            acc += tok ? (double)xent_ls_row(logf(se), mx, logits[(long long)r * C + t], sz, eps, C) : (double)NAN;
          else
            acc += tok ? (double)(logf(se) + mx - logits[(long long)r * C + t]) : (double)NAN;
          if (TK)
            nc += (tkok && rank < topk) ? 1 : 0;
          else
            nc += (tok && am == (int)t) ? 1 : 0;
        }
      }
    }
  } else {
    for (int r = wid; r < B; r += 16) {
      const float* row = logits + (long long)r * C;
      float mx = -INFINITY;
      int am = 0x7fffffff;
      for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        if (v > mx) { mx = v; am = c; }
      }
      // wave argmax: larger value wins, ties -> smaller index (first occurrence)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float omx = __shfl_xor(mx, o, kWave);
        const int oam = __shfl_xor(am, o, kWave);
        if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
      }
      float se = 0.f;
      for (int c = lane; c < C; c += 64) se += expf(row[c] - mx);
      se = wave_sum(se);
      float sz = 0.f;
      if (LS) {
        for (int c = lane; c < C; c += 64) sz += row[c] - mx;
        sz = wave_sum(sz);
      }
      int rank = 0;
      bool tkok = false;
      if (TK) {
        const long long t = tgt[r];
        if (t >= 0 && t < C) {
          const float zt = row[t];
          tkok = zt == zt;
          for (int c = lane; c < C; c += 64) rank += xent_above(row[c], c, zt, (int)t);
        }
        rank = wave_sum_i(rank);
      }
      if (lane == 0) {
        const long long t = tgt[r];
        const bool tok = t >= 0 && t < C;
        if (MIX) {
          const long long tb = tgt_b[r];
          acc += (tok && tb >= 0 && tb < C) ? (double)xent_mix_row<LS>(logf(se), mx, row[t], row[tb], lam, sz, eps, C)
                                            : (double)NAN;
        } else if (LS)
          acc += tok ? (double)xent_ls_row(logf(se), mx, row[t], sz, eps, C) : (double)NAN;
        else
          acc += tok ? (double)(logf(se) + mx - row[t]) : (double)NAN;
        if (TK)
          nc += (tkok && rank < topk) ? 1 : 0;
        else
          nc += (tok && am == (int)t) ? 1 : 0;
      }
    }
  }
  acc = wave_sum_d(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nc += __shfl_xor(nc, o, kWave);
  if (lane == 0) {
    red[wid] = acc;
    redc[wid] = nc;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    long long n = 0;
    for (int i = 0; i < 16; ++i) {
      s += red[i];
      n += redc[i];
    }
    if (loss) loss[0] = (float)(s / (double)B);
    if (sum_out) sum_out[0] = (float)s;
    if (correct) correct[0] += n;
  }
}

// dlogits = (softmax - onehot) * gscale[0] / B; LS: (softmax - (1 - eps) onehot - eps / C) * gscale[0] / B
// MIX: dlogits = (softmax - (1 - eps) (lam onehot_a + (1 - lam) onehot_b) - eps / C) * gscale[0] / B, for every
// eps (0 included); with t_a == t_b the two one-hot weights add on the same class. Each step is rounded
// on its own (no contraction), so xent_bwd_kernel and xent_linear_bwd_kernel give the same bits.
struct XentMixW {
  float wa, wb, off;
};
__device__ __forceinline__ XentMixW xent_mix_w(float lam, float eps, int C) {
  const float on = 1.f - eps;
  return XentMixW{on * lam, on * (1.f - lam), eps / (float)C};
}
__device__ __forceinline__ float xent_mix_grad(float e, float inv, bool isa, bool isb, const XentMixW& w, float k) {
  const float sm = __fmul_rn(e, inv);
  const float tw = __fadd_rn(isa ? w.wa : 0.f, isb ? w.wb : 0.f);
  return __fmul_rn(__fsub_rn(__fsub_rn(sm, tw), w.off), k);
}

template <bool LS, bool MIX>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ tgt,
                                                      const float* __restrict__ gscale, int B, int C,
                                                      float* __restrict__ dlogits, float eps,
                                                      const long long* __restrict__ tgt_b,
                                                      const float* __restrict__ lam_p) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* row = logits + (long long)r * C;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(row[c] - mx);
  se = wave_sum(se);
  const float k = gscale[0] / (float)B;
  const float inv = 1.f / se;
  const long long t = tgt[r];
  const float on = 1.f - eps, off = eps / (float)C;  // (LS only)
  if (MIX) {
    const long long tb = tgt_b[r];
    const XentMixW mw = xent_mix_w(lam_p[0], eps, C);
    for (int c = lane; c < C; c += 64)
      dlogits[(long long)r * C + c] = xent_mix_grad(expf(row[c] - mx), inv, c == t, c == tb, mw, k);
    return;
  }
  for (int c = lane; c < C; c += 64) {
    const float sm = expf(row[c] - mx) * inv;
    if (LS)
      dlogits[(long long)r * C + c] = (sm - (c == t ? on : 0.f) - off) * k;
    else
      dlogits[(long long)r * C + c] = (sm - (c == t ? 1.f : 0.f)) * k;
  }
}

// ------------------------------------------------------------------ binary cross-entropy
// Every logit its own one-vs-rest sigmoid classifier, against the dense target that mixup / CutMix and
// label smoothing define, formed in registers from the row's two class indices and xent_mix_w's weights:
//   y[r][c] = ((c == t_a ? wa : 0) + (c == t_b ? wb : 0)) + off     each + rounded on its own
//   thr_on:  y = y > thr ? 1 : 0
//   l = max(z, 0) - z y + log1p(exp(-|z|))                          finite for every finite z
//   loss = sum l / (B C), or / B with sum_classes;  dz = (sigmoid(z) - y) * gscale / (B C), or / B
// Without a second target lam = 1 and no class matches t_b: the arithmetic of lam[0] == 1.
struct BceArgs {
  float thr;
  int thr_on, sum_classes;
};
__device__ __forceinline__ float bce_y(bool isa, bool isb, const XentMixW& w, const BceArgs& a) {
  const float y = __fadd_rn(__fadd_rn(isa ? w.wa : 0.f, isb ? w.wb : 0.f), w.off);
  return a.thr_on ? (y > a.thr ? 1.f : 0.f) : y;
}
__device__ __forceinline__ float bce_elem(float z, float y) {
  return __fadd_rn(__fsub_rn(fmaxf(z, 0.f), __fmul_rn(z, y)), log1pf(expf(-fabsf(z))));
}
// sigmoid(z) from e = exp(-|z|) in (0, 1]: 1 / (1 + e) or e / (1 + e), in [0, 1] for every finite z
__device__ __forceinline__ float bce_grad(float z, float y, float k) {
  const float e = expf(-fabsf(z));
  const float sg = __fdiv_rn(z >= 0.f ? 1.f : e, __fadd_rn(1.f, e));
  return __fmul_rn(__fsub_rn(sg, y), k);
}
__device__ __forceinline__ float bce_k(float g, int B, int C, int sum_classes) {
  return sum_classes ? g / (float)B : g / ((float)B * (float)C);
}

// One block of 1024 threads in xent_fwd_kernel's three row layouts (C <= 64: a row per thread; C <= 1024: a
// wave's rows held in registers, two at a time; wider: a row per wave); every thread adds its elements in
// fp64 in a fixed order, then the fp64 block reduction: one writer, the same bits on every run. A target
// out of [0, C) in either slot adds a NaN.
template <bool MIX>
__global__ __launch_bounds__(1024) void bce_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ tgt,
                                                      int B, int C, float* __restrict__ loss, float eps, BceArgs ba,
                                                      const long long* __restrict__ tgt_b,
                                                      const float* __restrict__ lam_p) {
  __shared__ double red[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  double acc = 0.0;
  float lam = 1.f;
  if (MIX) lam = lam_p[0];
  const XentMixW mw = xent_mix_w(lam, eps, C);
  if (C <= 64) {
    for (int r = tid; r < B; r += 1024) {
      const float* row = logits + (long long)r * C;
      const long long t = tgt[r];
      long long tb = -1;
      if (MIX) tb = tgt_b[r];
      const bool ok = t >= 0 && t < C && (!MIX || (tb >= 0 && tb < C));
      for (int c = 0; c < C; ++c) acc += (double)bce_elem(row[c], bce_y(c == t, c == tb, mw, ba));
      if (!ok) acc += (double)NAN;
    }
  } else if (C <= 1024) {
    // rows wid + 16 k two at a time, all loaded before the first is used (as xent_fwd_kernel's four; two keep
    // the exp / log1p temporaries beside the tile within the 128 registers of a 1024-thread block)
    constexpr int RB = 2, J = 16;
    for (int rb = wid; rb < B; rb += 16 * RB) {
      float v[RB][J];
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const int r = rb + 16 * k;
        const float* row = logits + (long long)(r < B ? r : 0) * C;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int c = lane + 64 * j;
          v[k][j] = (r < B && c < C) ? row[c] : 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const int r = rb + 16 * k;
        if (r >= B) break;
        const long long t = tgt[r];  // (one address per wave: a broadcast load)
        long long tb = -1;
        if (MIX) tb = tgt_b[r];
        const bool ok = t >= 0 && t < C && (!MIX || (tb >= 0 && tb < C));
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int c = lane + 64 * j;
          if (c < C) acc += (double)bce_elem(v[k][j], bce_y(c == t, c == tb, mw, ba));
        }
        if (!ok && lane == 0) acc += (double)NAN;
      }
    }
  } else {
    for (int r = wid; r < B; r += 16) {
      const float* row = logits + (long long)r * C;
      const long long t = tgt[r];
      long long tb = -1;
      if (MIX) tb = tgt_b[r];
      const bool ok = t >= 0 && t < C && (!MIX || (tb >= 0 && tb < C));
      for (int c = lane; c < C; c += 64) acc += (double)bce_elem(row[c], bce_y(c == t, c == tb, mw, ba));
      if (!ok && lane == 0) acc += (double)NAN;
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) red[wid] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < 16; ++i) s += red[i];
    loss[0] = (float)(s / (ba.sum_classes ? (double)B : (double)B * (double)C));
  }
}

// Elementwise, xent_bwd_kernel's block shape (a wave per row, four rows per block). A row with a target out
// of range has no such class: no index matches. Every step rounded on its own (bce_y, bce_grad), so
// xent_linear_bwd_kernel's BCE mode gives the same bits.
template <bool MIX>
__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ tgt,
                                                     const float* __restrict__ gscale, int B, int C,
                                                     float* __restrict__ dlogits, float eps, BceArgs ba,
                                                     const long long* __restrict__ tgt_b,
                                                     const float* __restrict__ lam_p) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* row = logits + (long long)r * C;
  const float k = bce_k(gscale[0], B, C, ba.sum_classes);
  float lam = 1.f;
  if (MIX) lam = lam_p[0];
  const XentMixW mw = xent_mix_w(lam, eps, C);
  const long long t = tgt[r];
  long long tb = -1;
  if (MIX) tb = tgt_b[r];
  for (int c = lane; c < C; c += 64)
    dlogits[(long long)r * C + c] = bce_grad(row[c], bce_y(c == t, c == tb, mw, ba), k);
}

// ------------------------------------------------------------------ SGD (torch semantics)
// d_p = g*gs (+wd*p); buf = first ? d_p : buf*m + (1-damp)*d_p; d_p = nesterov ? d_p + m*buf : buf;
// p -= lr*d_p. Op order and fma placement follow ATen's add(alpha) (fmadd) so results match
// torch.optim.SGD to the last ulp on the same inputs.
__device__ __forceinline__ void sgd_one(float& p, float g, float& b, float lr, float m, float damp, float wd, float gs,
                                        bool nesterov, bool first, bool maximize, bool has_mom) {
  float d = g * gs;
  if (maximize) d = -d;
  if (wd != 0.f) d = fmaf(p, wd, d);
  if (has_mom) {
    if (first) b = d;
    else b = fmaf(d, 1.f - damp, b * m);
    d = nesterov ? fmaf(b, m, d) : b;
  }
  p = fmaf(d, -lr, p);
}

// Gradient-norm clip (CLIP instantiations only; ClipArgs in kernels.h): skip is workgroup-uniform. A
// skipped step leaves p and a loaded momentum value as they are, so the stores that follow write the
// same bits back; a skipped first momentum step stores zeros (the next, non-first step then computes
// buf = 0 * m + d_p = d_p, the first-step rule, for dampening 0).
template <bool CLIP>
__device__ __forceinline__ void sgd_upd(bool skip, float& p, float g, float& b, float lr, float m, float damp, float wd,
                                        float gs, bool nesterov, bool first, bool maximize, bool has_mom) {
  if (CLIP && skip) {
    if (has_mom && first) b = 0.f;
    return;
  }
  sgd_one(p, g, b, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
}
// The weight EMA (ema_one, ema_upd), the clip's prologue (sgd_clip_prologue), the learning-rate schedule's
// (sgd_sched_prologue) and the arrival rule that advances its step (sched_arrive) are in step_common.h:
// the Adam kernels (adam.hip) use the same ones.

// LARS (LARS instantiations only; LarsArgs in lars.h): the workgroup's elements all belong to the
// parameter `pr`. Its trust ratio q scales the two per-parameter values of sgd_one: gs = (gs * coef) * q
// and wd = wd_w * q (wd_w: wd, or 0 for an excluded parameter), so d = q * (g * gs * coef + wd * p).
// The parameter's first workgroup records q.
__device__ __forceinline__ void sgd_lars_prologue(const LarsArgs& lars, const LarsParam& pr, bool first_wg, float& gs,
                                                  float& wd) {
  const float q = lars_ratio_block(lars, pr, gs);
  if (first_wg && threadIdx.x == 0) lars.ratios[pr.slot] = q;
  gs *= q;
  wd = (lars.exclude && !pr.matrix ? 0.f : wd) * q;
}

template <bool CLIP, bool LARS, bool EMA, bool SCHED>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                 long long n, const float* __restrict__ lr_ptr, float lr_host, float m,
                                                 float damp, float wd, float gs, int flags, long long* counter,
                                                 ClipArgs clip, LarsArgs lars, EmaArgs ema, SchedArgs sched) {
  const bool nesterov = flags & 1, first = flags & 2, maximize = flags & 4, has_mom = flags & 8;
  const float ed = EMA ? ema.coef[0] : 0.f, eomd = EMA ? ema.coef[1] : 0.f;
  // a data loader's step counter advanced by the step (one dispatch less per step; the counter is
  // read by this step's augment kernel, which ran before)
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) counter[0] += 1;
  bool skip = false;
  if (CLIP) skip = sgd_clip_prologue(clip, gs);
  float lr = lr_ptr ? lr_ptr[0] : lr_host;
  long long sched_t = 0;  // (thread 0 of the SCHED instantiations)
  if (SCHED) {
    __shared__ float s_lr;
    lr = sgd_sched_prologue(sched, lr, &s_lr, sched_t);
  }
  if (LARS) {
    // one workgroup per (parameter, chunk) item of the norms pass's work list: whole float4s of one
    // parameter, so the ratio is workgroup-uniform
    const LarsItem it = lars.items[blockIdx.x];
    const LarsParam pr = lars.params[it.param];
    sgd_lars_prologue(lars, pr, (int)blockIdx.x == pr.part0, gs, wd);
    for (int i = threadIdx.x; i < it.n4; i += 256) {
      const long long e = it.start + 4LL * i;
      float4 pv = ld4(p + e);
      const float4 gv = ld4(g + e);
      float4 bv = has_mom && !first ? ld4(buf + e) : f4zero();
      sgd_upd<CLIP>(skip, pv.x, gv.x, bv.x, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      sgd_upd<CLIP>(skip, pv.y, gv.y, bv.y, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      sgd_upd<CLIP>(skip, pv.z, gv.z, bv.z, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      sgd_upd<CLIP>(skip, pv.w, gv.w, bv.w, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      st4(p + e, pv);
      if (has_mom) st4(buf + e, bv);
      if (EMA) {
        float4 ev = ld4(ema.e + e);
        ema_upd<CLIP>(skip, ev, pv, ed, eomd);
        st4(ema.e + e, ev);
      }
    }
    if (SCHED) sched_arrive(sched, sched_t);
    return;
  }
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  float dummy = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = ld4(p + 4 * i);
    const float4 gv = ld4(g + 4 * i);
    float4 bv = has_mom && !first ? ld4(buf + 4 * i) : f4zero();
    sgd_upd<CLIP>(skip, pv.x, gv.x, bv.x, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
    sgd_upd<CLIP>(skip, pv.y, gv.y, bv.y, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
    sgd_upd<CLIP>(skip, pv.z, gv.z, bv.z, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
    sgd_upd<CLIP>(skip, pv.w, gv.w, bv.w, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
    st4(p + 4 * i, pv);
    if (has_mom) st4(buf + 4 * i, bv);
    if (EMA) {
      float4 ev = ld4(ema.e + 4 * i);
      ema_upd<CLIP>(skip, ev, pv, ed, eomd);
      st4(ema.e + 4 * i, ev);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    float bb = has_mom && !first ? buf[i] : 0.f;
    float pp = p[i];
    sgd_upd<CLIP>(skip, pp, g[i], has_mom ? bb : dummy, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
    p[i] = pp;
    if (has_mom) buf[i] = bb;
    if (EMA && !(CLIP && skip)) ema.e[i] = ema_one(ema.e[i], pp, ed, eomd);
  }
  if (SCHED) sched_arrive(sched, sched_t);
}

// ------------------------------------------------------------------ weight maxima
// A 32x32 (co, ci) tile's contribution to its weight's maxima (weight_max_elems layout, kernels.h):
// the per-co partial of its ci block and the per-ci partial of its co block. Threads fold their
// values into s[0..32) (by co) and s[32..64) (by ci) with LDS atomics (zeroed by the caller before a
// barrier); after a barrier the first 64 threads store the 64 partials.
__device__ __forceinline__ void tile_max_add(unsigned* s, int co_local, int ci_local, float v) {
  const unsigned b = __float_as_uint(fabsf(v));
  if (b) {
    lds_max_u32(&s[co_local], b);
    lds_max_u32(&s[32 + ci_local], b);
  }
}
__device__ __forceinline__ void tile_max_store(const unsigned* s, float* __restrict__ wmax, int Co, int Ci, int co0,
                                               int ci0) {
  const int t = threadIdx.x;
  const int nci = (Ci + 31) / 32;
  if (t < 32 && co0 + t < Co) wmax[(long long)(ci0 / 32) * Co + co0 + t] = __uint_as_float(s[t]);
  else if (t >= 32 && t < 64 && ci0 + t - 32 < Ci)
    wmax[(long long)nci * Co + (long long)(co0 / 32) * Ci + ci0 + t - 32] = __uint_as_float(s[t]);
}

// ------------------------------------------------------------------ SGD + next-step weight preparation
// One pass over the parameter arena per step: the optimizer that writes W also emits what the next
// forward / backward GEMMs need from it (weight_prep_kernel's products): the f16x2 |max| partial of
// every 32x32 (co, ci) block and, where asked, W^T [ci][tap][co] (the data-gradient B operand).
// Blocks [0, nblk_w) own one (conv weight, co32, ci32) tile over all taps: load p / g / buf of the
// tile (branch-free buffer loads, TG taps per round trip), update exactly as sgd_kernel (same
// sgd_one), store p / buf in place, then the |max| and the transpose of the NEW p through LDS.
// Blocks [nblk_w, ...) each run sgd_kernel's float4 update over one chunk of the arena that no conv
// weight covers (biases, BatchNorm parameters, the classifier).
// EMA: the weight average e (EmaArgs) is updated from the new p on every path. The tile paths load e
// only after p and buf have left, into the registers of g and buf: measured with the compiler's
// report, +2 to +3 VGPRs over the EMA = false instantiation, which is the kernel without this block.
template <bool CLIP, bool LARS, bool EMA, bool SCHED>
__global__ __launch_bounds__(256) void sgd_prep_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ buf, const SgdPrepSeg* __restrict__ segs,
                                                      int nseg, int nblk_w, const SgdPrepChunk* __restrict__ chunks,
                                                      float* __restrict__ part, const float* __restrict__ lr_ptr,
                                                      float lr_host, float m, float damp, float wd, float gs,
                                                      int flags, long long* counter, ClipArgs clip, LarsArgs lars,
                                                      EmaArgs ema, SchedArgs sched) {
  // taps per group: 3 x 3 float4 in flight per thread keeps the kernel near 64 VGPRs (8 waves per
  // SIMD for this bandwidth-bound pass; a whole 3x3 filter per group held 256 VGPRs, 1 wave per SIMD)
  constexpr int TG = 3;
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) counter[0] += 1;  // as sgd_kernel
  __shared__ float tile[TG][32][33];
  __shared__ unsigned smax[64];
  bool skip = false;
  if (CLIP) skip = sgd_clip_prologue(clip, gs);  // as sgd_kernel; the |max| / W^T below are of the unchanged p
  const bool nesterov = flags & 1, first = flags & 2, maximize = flags & 4, has_mom = flags & 8;
  float lr = lr_ptr ? lr_ptr[0] : lr_host;
  long long sched_t = 0;  // as sgd_kernel
  if (SCHED) {
    __shared__ float s_lr;
    lr = sgd_sched_prologue(sched, lr, &s_lr, sched_t);
  }
  const float ed = EMA ? ema.coef[0] : 0.f, eomd = EMA ? ema.coef[1] : 0.f;
  const int b = blockIdx.x;
  if (b >= nblk_w) {
    const SgdPrepChunk ch = chunks[b - nblk_w];
    if (LARS) {  // the plan cut the rest chunks at parameter boundaries: one owner per chunk
      const LarsParam pr = lars.params[lars.owner[nseg + b - nblk_w]];
      sgd_lars_prologue(lars, pr, ch.start == pr.off, gs, wd);
    }
    for (int i = threadIdx.x; i < ch.n4; i += 256) {
      const long long e = ch.start + 4LL * i;
      float4 pv = ld4(p + e);
      const float4 gv = ld4(g + e);
      float4 bv = has_mom && !first ? ld4(buf + e) : f4zero();
      sgd_upd<CLIP>(skip, pv.x, gv.x, bv.x, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      sgd_upd<CLIP>(skip, pv.y, gv.y, bv.y, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      sgd_upd<CLIP>(skip, pv.z, gv.z, bv.z, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      sgd_upd<CLIP>(skip, pv.w, gv.w, bv.w, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
      st4(p + e, pv);
      if (has_mom) st4(buf + e, bv);
      if (EMA) {
        float4 ev = ld4(ema.e + e);
        ema_upd<CLIP>(skip, ev, pv, ed, eomd);
        st4(ema.e + e, ev);
      }
    }
    if (SCHED) sched_arrive(sched, sched_t);
    return;
  }
  int si = 0;
  while (si + 1 < nseg && segs[si + 1].blk0 <= b) ++si;
  const SgdPrepSeg sg = segs[si];
  if (LARS) sgd_lars_prologue(lars, lars.params[lars.owner[si]], b == sg.blk0, gs, wd);  // a tile is of one weight
  const int Co = sg.co, T = sg.t, Ci = sg.ci;
  float* __restrict__ wt = sg.wt;
  const int local = b - sg.blk0;
  const int nci = (Ci + 31) / 32;
  const int co0 = (local / nci) * 32, ci0 = (local % nci) * 32;
  const unsigned bytes = (unsigned)((long long)Co * T * Ci * 4);
  float* const pw = p + sg.off;
  float* const bw = buf ? buf + sg.off : nullptr;
  const __amdgpu_buffer_rsrc_t pr = make_rsrc(pw, bytes);
  const __amdgpu_buffer_rsrc_t gr = make_rsrc(g + sg.off, bytes);
  const __amdgpu_buffer_rsrc_t br = make_rsrc(has_mom && !first ? bw : pw, bytes);
  float* const ew = EMA ? ema.e + sg.off : pw;  // read only by the EMA instantiations
  const __amdgpu_buffer_rsrc_t er = make_rsrc(ew, bytes);
  if (threadIdx.x < 64) smax[threadIdx.x] = 0u;
  __syncthreads();
  if ((Ci & 3) == 0) {
    float4 mx4 = f4zero();  // |max| of the NEW (co, ci .. ci + 3) values over the taps
    // float4 along ci: thread (co row tid / 8, ci quad tid % 8) of the 32 x 32 tile, one (co, tap)
    // row of 32 ci per 8 threads (128 B), every tap of the group; the transpose goes through LDS
    // and leaves as float4 runs of 4 co of W^T [ci][tap][co]
    const int rco = threadIdx.x >> 3, c4 = threadIdx.x & 7;
    const int co = co0 + rco, ci = ci0 + 4 * c4;
    const bool ok = co < Co && ci < Ci;
    for (int t0 = 0; t0 < T; t0 += TG) {
      float4 vp[TG], vg[TG], vb[TG];
      unsigned off[TG];
#pragma unroll
      for (int q = 0; q < TG; ++q) {
        off[q] = (ok && t0 + q < T) ? (unsigned)(((co * T + t0 + q) * Ci + ci) * 4) : kOOB;
        vp[q] = bload4(pr, off[q]);
        vg[q] = bload4(gr, off[q]);
        vb[q] = has_mom && !first ? bload4(br, off[q]) : f4zero();
      }
#pragma unroll
      for (int q = 0; q < TG; ++q) {
        sgd_upd<CLIP>(skip, vp[q].x, vg[q].x, vb[q].x, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
        sgd_upd<CLIP>(skip, vp[q].y, vg[q].y, vb[q].y, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
        sgd_upd<CLIP>(skip, vp[q].z, vg[q].z, vb[q].z, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
        sgd_upd<CLIP>(skip, vp[q].w, vg[q].w, vb[q].w, lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
        if (off[q] != kOOB) {
          st4(pw + (off[q] >> 2), vp[q]);
          if (has_mom) st4(bw + (off[q] >> 2), vb[q]);
          mx4 = make_float4(fmaxf(mx4.x, fabsf(vp[q].x)), fmaxf(mx4.y, fabsf(vp[q].y)), fmaxf(mx4.z, fabsf(vp[q].z)),
                            fmaxf(mx4.w, fabsf(vp[q].w)));
        }
      }
      if (EMA) {
        // after p / buf left: e takes over the registers of g and buf, not a fourth array in flight
        float4 ve[TG];
#pragma unroll
        for (int q = 0; q < TG; ++q) ve[q] = bload4(er, off[q]);
#pragma unroll
        for (int q = 0; q < TG; ++q) {
          ema_upd<CLIP>(skip, ve[q], vp[q], ed, eomd);
          if (off[q] != kOOB) st4(ew + (off[q] >> 2), ve[q]);
        }
      }
      if (wt) {
#pragma unroll
        for (int q = 0; q < TG; ++q) {
          tile[q][rco][4 * c4] = vp[q].x;
          tile[q][rco][4 * c4 + 1] = vp[q].y;
          tile[q][rco][4 * c4 + 2] = vp[q].z;
          tile[q][rco][4 * c4 + 3] = vp[q].w;
        }
        __syncthreads();
        // thread (ci row tid / 8, co quad tid % 8): W^T[ci][tap][co .. co + 3]
        const int rci = threadIdx.x >> 3, q4 = threadIdx.x & 7;
        const int ci_o = ci0 + rci, co_o = co0 + 4 * q4;
#pragma unroll
        for (int q = 0; q < TG; ++q) {
          const int tap = t0 + q;
          if (tap >= T) break;
          if (ci_o < Ci && co_o + 3 < Co) {
            st4(wt + ((long long)ci_o * T + tap) * Co + co_o,
                make_float4(tile[q][4 * q4][rci], tile[q][4 * q4 + 1][rci], tile[q][4 * q4 + 2][rci],
                            tile[q][4 * q4 + 3][rci]));
          } else if (ci_o < Ci) {
            for (int j = 0; j < 4 && co_o + j < Co; ++j)
              wt[((long long)ci_o * T + tap) * Co + co_o + j] = tile[q][4 * q4 + j][rci];
          }
        }
        __syncthreads();
      }
    }
    const float4 z = mx4;  // (this thread's co row rco, ci quad c4)
    tile_max_add(smax, rco, 4 * c4, z.x);
    tile_max_add(smax, rco, 4 * c4 + 1, z.y);
    tile_max_add(smax, rco, 4 * c4 + 2, z.z);
    tile_max_add(smax, rco, 4 * c4 + 3, z.w);
  } else {
    // Ci not a multiple of 4 (an RGB stem's 3 input channels): one element per lane
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    float mco[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < T; t0 += TG) {
      float vp[TG][4], vg[TG][4], vb[TG][4];
      unsigned off[TG][4];
#pragma unroll
      for (int q = 0; q < TG; ++q)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int co = co0 + ty + 8 * jj, ci = ci0 + tx, tap = t0 + q;
          off[q][jj] = (co < Co && ci < Ci && tap < T) ? (unsigned)(((co * T + tap) * Ci + ci) * 4) : kOOB;
          vp[q][jj] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pr, (int)off[q][jj], 0, 0));
          vg[q][jj] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gr, (int)off[q][jj], 0, 0));
          vb[q][jj] = has_mom && !first
                          ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(br, (int)off[q][jj], 0, 0))
                          : 0.f;
        }
#pragma unroll
      for (int q = 0; q < TG; ++q)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          sgd_upd<CLIP>(skip, vp[q][jj], vg[q][jj], vb[q][jj], lr, m, damp, wd, gs, nesterov, first, maximize, has_mom);
          if (off[q][jj] != kOOB) {
            pw[off[q][jj] >> 2] = vp[q][jj];
            if (has_mom) bw[off[q][jj] >> 2] = vb[q][jj];
            mco[jj] = fmaxf(mco[jj], fabsf(vp[q][jj]));
          }
        }
      if (EMA) {
        float ve[TG][4];
#pragma unroll
        for (int q = 0; q < TG; ++q)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            ve[q][jj] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(er, (int)off[q][jj], 0, 0));
#pragma unroll
        for (int q = 0; q < TG; ++q)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            if (off[q][jj] != kOOB && !(CLIP && skip)) ew[off[q][jj] >> 2] = ema_one(ve[q][jj], vp[q][jj], ed, eomd);
      }
      if (wt) {
#pragma unroll
        for (int q = 0; q < TG; ++q)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) tile[q][ty + 8 * jj][tx] = vp[q][jj];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TG; ++q) {
          const int tap = t0 + q;
          if (tap >= T) break;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int ci = ci0 + ty + 8 * jj, co = co0 + tx;
            if (ci < Ci && co < Co) wt[((long long)ci * T + tap) * Co + co] = tile[q][tx][ty + 8 * jj];
          }
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) tile_max_add(smax, ty + 8 * jj, tx, mco[jj]);
  }
  __syncthreads();
  tile_max_store(smax, part + sg.pofs, Co, Ci, co0, ci0);
  if (SCHED) sched_arrive(sched, sched_t);
}

// ------------------------------------------------------------------ augmentation
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// out[b][h][w][c] (NHWC fp32) from uint8 HWC images[idx[b]], with optional RandomCrop(pad) and
// RandomHorizontalFlip(0.5) drawn from a counter-based hash of (seed, *counter, b), then
// ToTensor (/255) and Normalize(mean, std). Padding is zero in uint8 space (torchvision fill=0).
struct AugImage {
  const unsigned char* src;
  int oy, ox;
  bool fl;
};
// image b of the batch: its source and its own crop / flip draws
__device__ __forceinline__ AugImage aug_image(const unsigned char* __restrict__ imgs, long long src_i, int H, int W,
                                              int C, int pad, int flip, unsigned long long seed,
                                              unsigned long long ctr, int b) {
  const unsigned long long r = splitmix64(seed ^ splitmix64(ctr * 0x100000001B3ull + (unsigned long long)b));
  const int span = 2 * pad + 1;
  AugImage a;
  a.oy = pad ? (int)(r % span) - pad : 0;
  a.ox = pad ? (int)((r >> 16) % span) - pad : 0;
  a.fl = flip && ((r >> 40) & 1);
  a.src = imgs + src_i * (long long)H * W * C;
  return a;
}
// channel c of output pixel (h, w) of such an image, normalised
__device__ __forceinline__ const unsigned char* aug_pixel(const AugImage& a, int h, int w, int H, int W, int C,
                                                          bool& in) {
  const int ww = a.fl ? (W - 1 - w) : w;  // flip applied after the crop (torchvision order)
  const int sh = h + a.oy, sw = ww + a.ox;
  in = (unsigned)sh < (unsigned)H && (unsigned)sw < (unsigned)W;
  return a.src + (long long)(in ? sh * W + sw : 0) * C;
}

// MIX (mixup / CutMix on, see mix.h): image b is paired with p = B - 1 - b (batch reversal); every
// workgroup evaluates the batch's mix parameters itself, workgroup (0, 0) publishes them in mix[8].
// With X the batch this kernel writes without MIX at the same seed and counter:
//   mixup   out[b] = lam X[b] + (1 - lam) X[p]
//   cutmix  out[b] = X[p] inside the box, X[b] outside (bitwise)
//   none    out[b] = X[b] (bitwise; the partner image is not read)
// and labels_b[b] = labels of image p. The partner's crop and flip are its own draws (hashed with p).
// ERASE (RandomErasing on, see erase.h; 3-channel images): X above is X_e, the batch with every image's
// own box filled: X_e[b] = fill(b) inside erase_draw(b)'s box and X[b] (bitwise) outside. Erasing comes
// before mixing, so the partner shows its own box and noise (keyed by p), exactly as in its own output.
// Every workgroup evaluates the draws itself, workgroup (0, b) publishes image b's row in erase[b][5].
template <bool MIX, bool ERASE>
__global__ __launch_bounds__(256) void augment_kernel(const unsigned char* __restrict__ imgs,
                                                     const long long* __restrict__ idx, long long idx_off, int B,
                                                     int H, int W, int C, float m0, float m1, float m2, float is0,
                                                     float is1, float is2, int pad, int flip,
                                                     const long long* __restrict__ counter, unsigned long long seed,
                                                     float* __restrict__ out, long long nbatches,
                                                     const long long* __restrict__ labels,
                                                     long long* __restrict__ labels_out, MixCfg cfg,
                                                     float* __restrict__ mix, long long* __restrict__ labels_b,
                                                     EraseCfg ecfg, int* __restrict__ erase) {
  const int b = blockIdx.y;
  if (b >= B) return;
  const unsigned long long ctr = counter ? (unsigned long long)counter[0] : 0ull;
  // nbatches > 0: the batch offset into idx follows the step counter, so a replayed hipGraph walks
  // the epoch order without a host-side index copy per step
  const long long off = nbatches > 0 ? idx_off + (long long)(ctr % (unsigned long long)nbatches) * B : idx_off;
  const long long src_i = idx ? idx[off + b] : (off + b);
  if (labels_out && blockIdx.x == 0 && threadIdx.x == 0) labels_out[b] = labels[src_i];
  const AugImage ia = aug_image(imgs, src_i, H, W, C, pad, flip, seed, ctr, b);
  const float mean[3] = {m0, m1, m2};
  const float istd[3] = {is0, is1, is2};
  const int npix = H * W;
  float* dst = out + (long long)b * npix * C;
  EraseImg ea, eb;
  if (ERASE) {
    ea = erase_image(seed, ctr, b, ecfg, H, W);
    if (blockIdx.x == 0 && threadIdx.x == 0) erase_publish(erase + (long long)b * kEraseRow, ea.bx);
  }
  if (!MIX) {
    // one thread per output pixel, all its channels (one index decode per pixel, not per element)
    for (int px = blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += gridDim.x * blockDim.x) {
      const int h = px / W, w = px - (px / W) * W;
      if (ERASE && erase_in(ea.bx, h, w)) {  // (an erased pixel does not read its source)
        for (int c = 0; c < 3; ++c) dst[(long long)px * 3 + c] = erase_fill(ea, ecfg.mode, px, c);
        continue;
      }
      bool in;
      const unsigned char* sp = aug_pixel(ia, h, w, H, W, C, in);
      for (int c = 0; c < C; ++c) {
        const float v = in ? (float)sp[c] * (1.f / 255.f) : 0.f;
        const int ci = c < 3 ? c : 2;
        dst[(long long)px * C + c] = (v - mean[ci]) * istd[ci];
      }
    }
    return;
  }
  const MixParams mp = mix_draw(seed, ctr, cfg, H, W);
  const int p = B - 1 - b;
  const long long src_p = idx ? idx[off + p] : (off + p);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (labels_b) labels_b[b] = labels[src_p];
    if (b == 0 && mix) mix_publish(mix, mp);
  }
  const AugImage ib = aug_image(imgs, src_p, H, W, C, pad, flip, seed, ctr, p);
  if (ERASE && mp.mode != kMixNone) eb = erase_image(seed, ctr, p, ecfg, H, W);
  // The mode is uniform over the grid: mixup reads both images; CutMix and none read one source per
  // pixel, in the unmixed kernel's loop.
  if (mp.mode == kMixMixup) {
    const float lam = mp.lam, oml = 1.f - mp.lam;
    for (int px = blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += gridDim.x * blockDim.x) {
      const int h = px / W, w = px - (px / W) * W;
      bool ina, inb;
      const unsigned char* spa = aug_pixel(ia, h, w, H, W, C, ina);
      const unsigned char* spb = aug_pixel(ib, h, w, H, W, C, inb);
      const bool era = ERASE && erase_in(ea.bx, h, w), erb = ERASE && erase_in(eb.bx, h, w);
      for (int c = 0; c < C; ++c) {
        const float va = ina ? (float)spa[c] * (1.f / 255.f) : 0.f;
        const float vb = inb ? (float)spb[c] * (1.f / 255.f) : 0.f;
        const int ci = c < 3 ? c : 2;
        float xa = (va - mean[ci]) * istd[ci], xb = (vb - mean[ci]) * istd[ci];
        if (era) xa = erase_fill(ea, ecfg.mode, px, ci);
        if (erb) xb = erase_fill(eb, ecfg.mode, px, ci);
        dst[(long long)px * C + c] = lam * xa + oml * xb;
      }
    }
    return;
  }
  const bool cut = mp.mode == kMixCutmix;
  for (int px = blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += gridDim.x * blockDim.x) {
    const int h = px / W, w = px - (px / W) * W;
    // CutMix: the pixel comes whole from the partner inside the box, from the image itself outside
    const bool box = cut && h >= mp.y0 && h < mp.y1 && w >= mp.x0 && w < mp.x1;
    if (ERASE && erase_in(box ? eb.bx : ea.bx, h, w)) {  // the source image's own box and noise
      for (int c = 0; c < 3; ++c) dst[(long long)px * 3 + c] = erase_fill(box ? eb : ea, ecfg.mode, px, c);
      continue;
    }
    AugImage s;
    s.src = box ? ib.src : ia.src;
    s.oy = box ? ib.oy : ia.oy;
    s.ox = box ? ib.ox : ia.ox;
    s.fl = box ? ib.fl : ia.fl;
    bool in;
    const unsigned char* sp = aug_pixel(s, h, w, H, W, C, in);
    for (int c = 0; c < C; ++c) {
      const float v = in ? (float)sp[c] * (1.f / 255.f) : 0.f;
      const int ci = c < 3 ? c : 2;
      dst[(long long)px * C + c] = (v - mean[ci]) * istd[ci];
    }
  }
}

// mix[i] = the published row of step counter first + i: mix_draw over n consecutive counters (the
// schedule a loader will follow, for logging and for the distribution tests)
__global__ __launch_bounds__(256) void mix_params_kernel(unsigned long long seed, long long first, long long n,
                                                        MixCfg cfg, int H, int W, float* __restrict__ mix) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mix_publish(mix + i * kMixRow, mix_draw(seed, (unsigned long long)(first + i), cfg, H, W));
}

// ------------------------------------------------------------------ augmentation with a resize
// out[b][y][x][c] (NHWC fp32, OH x OW) from a window {top, left, h, w} of the uint8 HWC images[idx[b]]:
// RandomResizedCrop (train: the window is rrc_draw's, rrc.h) or resize + center crop (eval: the central
// window the launcher computed), then the flip of aug_image's hash, ToTensor and Normalize. Bilinear,
// align_corners = false, no antialias, evaluated inside the window (neighbours clamp at the window's
// edge: torchvision's crop-then-resize). The source coordinate of output index o of an axis of
// n_out from n_in is exact in integers: with n = max((2 o + 1) n_in - n_out, 0),
//   i0 = n / (2 n_out), i1 = min(i0 + 1, n_in - 1), lam = float(n % (2 n_out)) / float(2 n_out)
// so each weight carries one rounding. The blend is in the 0 .. 255 domain and is not re-quantised to
// uint8 before the normalisation. Every sum of two products is written as one product and one fmaf:
// the build contracts (-ffp-contract=fast fuses a product into a sum wherever it finds one, differently
// from one caller to the next, and no pragma stops it), and the MIX instantiation must give the bits of
// the plain one; in this form nothing is left to fuse.
struct RszWin {  // an image's window and flip, as the drawing lane leaves them in LDS
  int top, left, h, w, fl;
};
struct RszTap {  // the two neighbours along one axis and the weight of the second
  int i0, i1;
  float lam;
  int pad_;
};
constexpr int kRszCols = 1024;  // output columns per pass: 4 per thread

__device__ __forceinline__ RszTap rsz_tap(int o, int n_in, int n_out) {
  const unsigned num = (unsigned)max((2 * o + 1) * n_in - n_out, 0);  // < 2^31 for sizes < 32768
  const unsigned den = 2u * (unsigned)n_out;
  const unsigned i0 = num / den;
  RszTap t;
  t.i0 = min((int)i0, n_in - 1);
  t.i1 = min((int)i0 + 1, n_in - 1);
  t.lam = (float)(num - i0 * den) / (float)den;
  t.pad_ = 0;
  return t;
}
__device__ __forceinline__ RszWin rsz_window(int train, const RrcCfg& rc, int eh, int ew, int flip,
                                             unsigned long long seed, unsigned long long ctr, int b, int H, int W) {
  RrcWindow r{(H - eh) / 2, (W - ew) / 2, eh, ew};
  if (train) r = rrc_draw(seed, ctr, b, rc, H, W);
  // the flip bit of aug_image's hash: the same bit with the resize on or off
  const AugImage a = aug_image(nullptr, 0, H, W, 3, 0, flip, seed, ctr, b);
  return RszWin{r.top, r.left, r.h, r.w, a.fl ? 1 : 0};
}
// the rows of an image's window that output row y blends, and their weights
struct RszRows {
  const unsigned char* r0;
  const unsigned char* r1;
  float w0, w1;
};
__device__ __forceinline__ RszRows rsz_rows(const unsigned char* __restrict__ imgs, long long src_i, const RszWin& wn,
                                            int y, int H, int W, int OH) {
  const RszTap t = rsz_tap(y, wn.h, OH);
  const unsigned char* base = imgs + (src_i * H + wn.top) * (long long)W * 3 + (long long)wn.left * 3;
  return RszRows{base + (long long)t.i0 * W * 3, base + (long long)t.i1 * W * 3, 1.f - t.lam, t.lam};
}
// channel c of one output pixel, normalised ((v / 255 - mean) / std, the plain kernel's expression)
__device__ __forceinline__ float rsz_sample(const RszRows& rw, const RszTap& ct, int c, float mean, float istd) {
  const int o0 = ct.i0 * 3 + c, o1 = ct.i1 * 3 + c;
  const float wx0 = 1.f - ct.lam, wx1 = ct.lam;
  const float t = fmaf(wx1, (float)rw.r0[o1], wx0 * (float)rw.r0[o0]);
  const float u = fmaf(wx1, (float)rw.r1[o1], wx0 * (float)rw.r1[o0]);
  const float v = fmaf(rw.w1, u, rw.w0 * t);
  return fmaf(v, 1.f / 255.f, -mean) * istd;
}

// Shape of the work: blockIdx.y = image, blockIdx.x strides over passes of 256 / (quads per row) rows.
// A thread owns 4 consecutive output pixels of a row (12 contiguous floats: three 16-byte stores when
// OW % 4 == 0 and out is 16-byte aligned, `vec`; scalar stores otherwise) and keeps its columns over
// its rows. Thread 0 evaluates the window (under MIX also the partner's and the batch's mix) and shares
// it through LDS; the per-column taps (flip included) are computed once per workgroup, also in LDS.
// MIX: as augment_kernel's, with X the batch the <false> instantiation writes: the partner p = B - 1 - b
// is resampled through its own window and flip, and the CutMix box is in output pixels.
// ERASE: as augment_kernel's, the boxes in OH x OW output pixels. Thread 0 draws the one or two boxes with
// the windows and shares them through the same LDS hand-off (no barrier of its own); erased values
// replace a pixel's lanes of v[12] before the store, so the 16-byte store path is the plain one. The box
// test is uniform over every wavefront that a box's edge does not cross.
template <bool MIX, bool ERASE>
__global__ __launch_bounds__(256) void augment_resize_kernel(
    const unsigned char* __restrict__ imgs, const long long* __restrict__ idx, long long idx_off, int B, int H, int W,
    int OH, int OW, float m0, float m1, float m2, float is0, float is1, float is2, int train, RrcCfg rc, int eh, int ew,
    int flip, const long long* __restrict__ counter, unsigned long long seed, float* __restrict__ out,
    long long nbatches, const long long* __restrict__ labels, long long* __restrict__ labels_out,
    int* __restrict__ crops, MixCfg cfg, float* __restrict__ mix, long long* __restrict__ labels_b, int vec,
    EraseCfg ecfg, int* __restrict__ erase) {
  constexpr int NI = MIX ? 2 : 1;
  __shared__ RszWin s_win[NI];
  __shared__ MixParams s_mp;
  __shared__ RszTap s_tap[NI][kRszCols];
  __shared__ EraseImg s_er[NI];  // (referenced under ERASE only)
  const int b = blockIdx.y;
  if (b >= B) return;
  const unsigned long long ctr = counter ? (unsigned long long)counter[0] : 0ull;
  const long long off = nbatches > 0 ? idx_off + (long long)(ctr % (unsigned long long)nbatches) * B : idx_off;
  const int p = B - 1 - b;
  const long long src_a = idx ? idx[off + b] : (off + b);
  const long long src_p = MIX ? (idx ? idx[off + p] : (off + p)) : src_a;
  if (threadIdx.x == 0) {
    const RszWin wa = rsz_window(train, rc, eh, ew, flip, seed, ctr, b, H, W);
    s_win[0] = wa;
    MixParams mp{kMixNone, 1.f, 1.f, 0, 0, 0, 0};
    if (MIX) {
      mp = mix_draw(seed, ctr, cfg, OH, OW);
      s_win[NI - 1] = rsz_window(train, rc, eh, ew, flip, seed, ctr, p, H, W);
    }
    s_mp = mp;
    if (ERASE) {
      s_er[0] = erase_image(seed, ctr, b, ecfg, OH, OW);
      if (MIX && mp.mode != kMixNone) s_er[NI - 1] = erase_image(seed, ctr, p, ecfg, OH, OW);
      if (blockIdx.x == 0) erase_publish(erase + (long long)b * kEraseRow, s_er[0].bx);
    }
    if (blockIdx.x == 0) {
      if (labels_out) labels_out[b] = labels[src_a];
      int* row = crops + (long long)b * kCropRow;
      row[0] = wa.top;
      row[1] = wa.left;
      row[2] = wa.h;
      row[3] = wa.w;
      row[4] = wa.fl;
      if (MIX) {
        if (labels_b) labels_b[b] = labels[src_p];
        if (b == 0 && mix) mix_publish(mix, mp);
      }
    }
  }
  __syncthreads();
  const RszWin wa = s_win[0], wp = s_win[NI - 1];
  const int mode = MIX ? s_mp.mode : kMixNone;  // uniform over the grid
  const int by0 = s_mp.y0, by1 = s_mp.y1, bx0 = s_mp.x0, bx1 = s_mp.x1;
  const float lam = s_mp.lam, oml = 1.f - s_mp.lam;
  EraseImg ea, ep;
  if (ERASE) {
    ea = s_er[0];
    ep = s_er[NI - 1];  // (drawn, and used below, only when the batch is mixed)
  }
  const float mean[3] = {m0, m1, m2};
  const float istd[3] = {is0, is1, is2};
  const int nq = (OW + 3) >> 2;           // quads per row
  const int nqt = nq < 256 ? nq : 256;    // quads per pass
  const int rpp = 256 / nqt;              // rows per pass
  const int r = threadIdx.x / nqt, q = threadIdx.x - r * nqt;
  float* dst = out + (long long)b * OH * OW * 3;
  for (int c0 = 0; c0 < OW; c0 += kRszCols) {
    if (c0) __syncthreads();  // the previous pass's readers are done with the taps
    const int ncol = min(kRszCols, OW - c0);
    for (int x = threadIdx.x; x < ncol; x += 256) {
      const int xo = c0 + x;
      s_tap[0][x] = rsz_tap(wa.fl ? OW - 1 - xo : xo, wa.w, OW);  // flip after the resize (torchvision order)
      if (MIX && mode != kMixNone) s_tap[NI - 1][x] = rsz_tap(wp.fl ? OW - 1 - xo : xo, wp.w, OW);
    }
    __syncthreads();
    const int x0 = c0 + 4 * q;
    if (r >= rpp || x0 >= OW) continue;
    for (int y = blockIdx.x * rpp + r; y < OH; y += gridDim.x * rpp) {
      const RszRows ra = rsz_rows(imgs, src_a, wa, y, H, W, OH);
      RszRows rb = ra;
      if (MIX && mode != kMixNone) rb = rsz_rows(imgs, src_p, wp, y, H, W, OH);
      float v[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        const int xl = min(x, OW - 1) - c0;  // (a lane past the row's end computes its last pixel again)
        const RszTap ta = s_tap[0][xl];
        const long long pix = (long long)y * OW + x;  // (past the row's end: in no box, and not stored)
        if (MIX && mode == kMixMixup) {
          const RszTap tb = s_tap[NI - 1][xl];
          const bool era = ERASE && erase_in(ea.bx, y, x), erb = ERASE && erase_in(ep.bx, y, x);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float xa = rsz_sample(ra, ta, c, mean[c], istd[c]), xb = rsz_sample(rb, tb, c, mean[c], istd[c]);
            if (era) xa = erase_fill(ea, ecfg.mode, pix, c);
            if (erb) xb = erase_fill(ep, ecfg.mode, pix, c);
            v[3 * j + c] = lam * xa + oml * xb;
          }
        } else if (MIX && mode == kMixCutmix) {
          // the pixel comes whole from the partner inside the box, from the image itself outside
          const bool box = y >= by0 && y < by1 && x >= bx0 && x < bx1;
          const RszTap ts = box ? s_tap[NI - 1][xl] : ta;
          RszRows rs;
          rs.r0 = box ? rb.r0 : ra.r0;
          rs.r1 = box ? rb.r1 : ra.r1;
          rs.w0 = box ? rb.w0 : ra.w0;
          rs.w1 = box ? rb.w1 : ra.w1;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * j + c] = rsz_sample(rs, ts, c, mean[c], istd[c]);
          if (ERASE && erase_in(box ? ep.bx : ea.bx, y, x)) {  // the source image's own box and noise
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * j + c] = erase_fill(box ? ep : ea, ecfg.mode, pix, c);
          }
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * j + c] = rsz_sample(ra, ta, c, mean[c], istd[c]);
          if (ERASE && erase_in(ea.bx, y, x)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * j + c] = erase_fill(ea, ecfg.mode, pix, c);
          }
        }
      }
      float* o = dst + ((long long)y * OW + x0) * 3;
      if (vec) {  // OW % 4 == 0: the quad is whole and 16-byte aligned
        st4(o, make_float4(v[0], v[1], v[2], v[3]));
        st4(o + 4, make_float4(v[4], v[5], v[6], v[7]));
        st4(o + 8, make_float4(v[8], v[9], v[10], v[11]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < OW) {
            o[3 * j] = v[3 * j];
            o[3 * j + 1] = v[3 * j + 1];
            o[3 * j + 2] = v[3 * j + 2];
          }
      }
    }
  }
}

// win[i][b] = {top, left, h, w}: rrc_draw of step counter first + i and image slot b, i < n (the windows a
// loader will publish, for logging and for the distribution tests)
__global__ __launch_bounds__(256) void rrc_params_kernel(unsigned long long seed, long long first, long long total,
                                                        int B, RrcCfg rc, int H, int W, int* __restrict__ win) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const RrcWindow r = rrc_draw(seed, (unsigned long long)(first + i / B), (int)(i % B), rc, H, W);
  win[4 * i] = r.top;
  win[4 * i + 1] = r.left;
  win[4 * i + 2] = r.h;
  win[4 * i + 3] = r.w;
}

// rows[i][b] = {on, top, left, h, w}: erase_draw of step counter first + i and image slot b, i < n (the rows a
// loader will publish: the counterpart of rrc_params_kernel)
__global__ __launch_bounds__(256) void erase_params_kernel(unsigned long long seed, long long first, long long total,
                                                          int B, EraseCfg ecfg, int H, int W, int* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  erase_publish(rows + i * kEraseRow, erase_draw(seed, (unsigned long long)(first + i / B), (int)(i % B), ecfg, H, W));
}
// out[b][y][x][c] = erase_noise(seed, ctr, b, (y OW + x) 3 + c): the fill noise of one counter, through the
// function the augment kernels call (per3 = 3 OH OW elements per image)
__global__ __launch_bounds__(256) void erase_noise_kernel(unsigned long long seed, unsigned long long ctr,
                                                         long long total, long long per3, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long b = i / per3;
    out[i] = erase_noise(seed, ctr, (int)b, i - b * per3);
  }
}

__global__ void counter_inc_kernel(long long* c) { c[0] += 1; }
// The schedule's step without an SGD launch: one thread does what the last arrival of sched_arrive does.
__global__ void lr_sched_advance_kernel(SchedArgs sched, const float* __restrict__ lr_ptr, float lr_host) {
  const long long t = sched.state[0];
  const float lr = lr_sched_rate(*sched.cfg, t, lr_ptr ? lr_ptr[0] : lr_host);
  sched.state[0] = t + 1;
  sched.state[1] = 0;
  if (sched.last_lr) sched.last_lr[0] = lr;
}
// out[i] = lr_t of step first + i, i < n (the rates sgd_sched_prologue gives at those steps): the
// schedule's counterpart of mix_params_kernel / rrc_params_kernel
__global__ __launch_bounds__(256) void lr_sched_table_kernel(const LrSchedCfg* __restrict__ cfg,
                                                            const float* __restrict__ lr_ptr, float lr_host,
                                                            long long first, long long n, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = lr_sched_rate(*cfg, first + i, lr_ptr ? lr_ptr[0] : lr_host);
}

// dX of a stride-2 conv's sub-pixel parity classes with no filter taps (bit 2 ph + pw of mask):
// zeros, float4 along C (NHWC), one thread per float4 of the classes' pixels
__global__ __launch_bounds__(256) void subpixel_zero_kernel(float* __restrict__ dx, int N, int H, int W, int C4,
                                                            int mask, FastDiv fd_C4, FastDiv fd_W) {
  const long long total = (long long)N * H * W * C4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int pix = (int)(i / C4);  // < 2^31 pixels (launcher)
    const int t = fdiv(pix, fd_W);
    const int w = pix - t * W;
    const int h = t % H;
    if ((mask >> (2 * (h & 1) + (w & 1))) & 1) st4(dx + 4 * i, f4zero());
  }
}

// ------------------------------------------------------------------ weight transpose
// W[co][tap][ci] -> Wt[ci][tap][co]   (tap = kh*KW+kw; conv data-gradient uses Wt as its B^T)
__global__ __launch_bounds__(256) void wtrans_kernel(const float* __restrict__ w, float* __restrict__ wt, int Co,
                                                     int T, int Ci) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z;
  const int co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int co = co0 + j, ci = ci0 + tx;
    tile[j][tx] = (co < Co && ci < Ci) ? w[((long long)co * T + tap) * Ci + ci] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int ci = ci0 + j, co = co0 + tx;
    if (ci < Ci && co < Co) wt[((long long)ci * T + tap) * Co + co] = tile[tx][j];
  }
}

// ------------------------------------------------------------------ weight preparation
// One launch for all conv weights of a step (replaces a transpose launch per layer plus the
// |max| pass): block (segment, co32, ci32) walks the T taps of its 32x32 (co, ci) block, writes its
// per-co and per-ci |max| partials (the f16x2 operand scales of the weight's two GEMM roles) and,
// when asked, the tile transposed through LDS.
// Taps go in groups of TG: all of a group's loads are issued before any is used (branch-free: out
// of range elements read 0 through the buffer range check), so a 3x3 filter costs one memory round
// trip per block instead of nine.
__global__ __launch_bounds__(256) void weight_prep_kernel(WeightPrepArgs a, float* __restrict__ part) {
  constexpr int TG = 9;
  __shared__ float tile[TG][32][33];
  __shared__ unsigned smax[64];
  const int b = blockIdx.x;
  int seg = 0;
  while (seg + 1 < a.nseg && a.blk0[seg + 1] <= b) ++seg;
  const int Co = a.co[seg], T = a.t[seg], Ci = a.ci[seg];
  const float* __restrict__ w = a.w[seg];
  float* __restrict__ wt = a.wt[seg];
  const int local = b - a.blk0[seg];
  const int nci = (Ci + 31) / 32;
  const int co0 = (local / nci) * 32, ci0 = (local % nci) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(w, (unsigned)((long long)Co * T * Ci * 4));
  if (threadIdx.x < 64) smax[threadIdx.x] = 0u;
  __syncthreads();
  float mco[4] = {0.f, 0.f, 0.f, 0.f};  // |max| of (co0 + ty + 8 jj, ci0 + tx) over the taps
  for (int t0 = 0; t0 < T; t0 += TG) {
    float v[TG][4];
#pragma unroll
    for (int g = 0; g < TG; ++g)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int co = co0 + ty + 8 * jj, ci = ci0 + tx, tap = t0 + g;
        const unsigned o = (co < Co && ci < Ci && tap < T) ? (unsigned)(((co * T + tap) * Ci + ci) * 4) : kOOB;
        v[g][jj] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wr, (int)o, 0, 0));
      }
#pragma unroll
    for (int g = 0; g < TG; ++g)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) mco[jj] = fmaxf(mco[jj], fabsf(v[g][jj]));
    if (wt) {
#pragma unroll
      for (int g = 0; g < TG; ++g)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) tile[g][ty + 8 * jj][tx] = v[g][jj];
      __syncthreads();
#pragma unroll
      for (int g = 0; g < TG; ++g) {
        const int tap = t0 + g;
        if (tap >= T) break;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int ci = ci0 + ty + 8 * jj, co = co0 + tx;
          if (ci < Ci && co < Co) wt[((long long)ci * T + tap) * Co + co] = tile[g][tx][ty + 8 * jj];
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) tile_max_add(smax, ty + 8 * jj, tx, mco[jj]);
  __syncthreads();
  tile_max_store(smax, part + a.pofs[seg], Co, Ci, co0, ci0);
}

// ------------------------------------------------------------------ channel padding
// out[p][0..C4) = (x[p][0..C), 0...) for NHWC pixels p: the RGB stem's 3 -> 4 channel padding in
// one pass (one float4 store per pixel) over a contiguous pixel range per block, plus the padded
// tensor's per-image / per-channel |max| (act_max.h) the f16x2 GEMM scales need.
__global__ __launch_bounds__(256) void pad_c4_kernel(const float* __restrict__ x, int N, long long HW, int C,
                                                     float* __restrict__ out, FastDiv fd_HW, ActMaxOut am) {
  __shared__ ActMaxBlock<4> sam;
  const bool want = am.img != nullptr;
  const long long npix = (long long)N * HW;
  const long long per = (npix + gridDim.x - 1) / gridDim.x;
  const long long p0 = (long long)blockIdx.x * per, p1 = min(npix, p0 + per);
  const int img0 = (int)(min(p0, npix - 1) / HW);
  if (want) {
    sam.init(threadIdx.x, 256);
    __syncthreads();
  }
  ImgRun run;
  float4 cm = f4zero();
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    const float* src = x + p * C;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = c < C ? src[c] : 0.f;
    const float4 z = make_float4(v[0], v[1], v[2], v[3]);
    st4(out + p * 4, z);
    if (want) {
      run.add(fdiv((int)p, fd_HW), absmax4(z), sam, img0, am);
      cm = absmax4(cm, z);
    }
  }
  if (want) {
    run.flush(sam, img0, am);
    sam.add_ch4(0, cm);
    __syncthreads();
    sam.publish(am, img0, N, 0, 4, 4, blockIdx.x % kActCopies, threadIdx.x, 256);
  }
}

// ------------------------------------------------------------------ stack mean / scale / colsum
struct StackSrcs {
  const float* p[kMaxStackSrcs];
};
__global__ __launch_bounds__(256) void stack_mean_kernel(StackSrcs srcs, int k, long long n, float* __restrict__ dst) {
  const float inv = 1.f / (float)k;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += srcs.p[j][i];
    dst[i] = s * inv;
  }
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, long long n, float a) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    x[i] *= a;
}

// out[c] (+)= sum_r x[r][c]   (Linear bias gradient)
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int R, int C, float* __restrict__ out,
                                                     int accumulate) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  __shared__ float red[4][64];
  float s = 0.f;
  if (c < C)
    for (int r = rl; r < R; r += 4) s += x[(long long)r * C + c];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
    const float t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    out[c] = accumulate ? out[c] + t : t;
  }
}

// ------------------------------------------------------------------ narrow Linear (classifier heads)
// O <= 16 outputs (VGG-11's fc1 is 512 -> 10: a 128x128 MFMA tile would be >90% padding).
constexpr int SL_MAXO = 16;

// y[r][o] = x[r] . W[o] + b[o]: one wave per row; each lane keeps its slice of x in registers,
// accumulates all O partial dot products, and the wave reduces them through LDS once.
__global__ __launch_bounds__(256) void small_linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ b, int B, int I, int O,
                                                               float* __restrict__ y) {
  __shared__ float red[4][SL_MAXO][65];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wv;
  float part[SL_MAXO];
#pragma unroll
  for (int o = 0; o < SL_MAXO; ++o) part[o] = 0.f;
  if (r < B) {
    const float* xr = x + (long long)r * I;
    for (int i = lane; i < I; i += 64) {
      const float xv = xr[i];
      // no per-o branch: clamped rows keep every load unconditional (a runtime-predicated load per
      // element makes hipcc wait vmcnt(0) around each one); rows >= O are never stored
#pragma unroll
      for (int o = 0; o < SL_MAXO; ++o) part[o] = fmaf(xv, w[(long long)min(o, O - 1) * I + i], part[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < SL_MAXO; ++o) red[wv][o][lane] = part[o];
  __syncthreads();
  if (r < B && lane < O) {
    float s = 0.f;
    for (int k = 0; k < 64; ++k) s += red[wv][lane][k];
    y[(long long)r * O + lane] = s + (b ? b[lane] : 0.f);
  }
}

// One launch for all three gradients:
//   blocks [0, nbx)          dX[r][i] = sum_o dy[r][o] * W[o][i]       (thread per element)
//   blocks [nbx, nbx + nbw)  dW[o][i] = sum_r dy[r][o] * x[r][i]       (16 columns x 16 row-lanes per
//                            block; every thread accumulates all O outputs of its column)
//   last block               db[o]    = sum_r dy[r][o]
// (dy: global memory, or the block's LDS copy in xent_linear_bwd_kernel)
__device__ __forceinline__ void small_linear_bwd_body(const float* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ w, int B, int I, int O,
                                                      float* __restrict__ dx, float* __restrict__ dw,
                                                      float* __restrict__ db, int nbx, int nbw, int bid) {
  __shared__ float red[16][SL_MAXO][17];
  if (bid < nbx) {
    const long long e = (long long)bid * 256 + threadIdx.x;
    if (e >= (long long)B * I) return;
    const int r = (int)(e / I), i = (int)(e % I);
    float s = 0.f;
    for (int o = 0; o < O; ++o) s = fmaf(dy[(long long)r * O + o], w[(long long)o * I + i], s);
    dx[e] = s;
  } else if (bid < nbx + nbw) {
    const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int i = (bid - nbx) * 16 + col;
    float acc[SL_MAXO];
#pragma unroll
    for (int o = 0; o < SL_MAXO; ++o) acc[o] = 0.f;
    if (i < I) {
      for (int r = rl; r < B; r += 16) {
        const float xv = x[(long long)r * I + i];
#pragma unroll
        for (int o = 0; o < SL_MAXO; ++o) acc[o] = fmaf(dy[(long long)r * O + min(o, O - 1)], xv, acc[o]);
      }
    }
#pragma unroll
    for (int o = 0; o < SL_MAXO; ++o) red[rl][o][col] = acc[o];
    __syncthreads();
    // 256 threads finish 16 columns x O outputs
    const int o = threadIdx.x >> 4;
    if (o < O && i - col + (threadIdx.x & 15) < I) {
      const int c = threadIdx.x & 15;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += red[k][o][c];
      dw[(long long)o * I + (bid - nbx) * 16 + c] = s;
    }
  } else if (db) {
    __shared__ float rdb[4][64];
    const int o = threadIdx.x & 63, rl = threadIdx.x >> 6;
    float s = 0.f;
    if (o < O)
      for (int r = rl; r < B; r += 4) s += dy[(long long)r * O + o];
    rdb[rl][o] = s;
    __syncthreads();
    if (rl == 0 && o < O) db[o] = rdb[0][o] + rdb[1][o] + rdb[2][o] + rdb[3][o];
  }
}

__global__ __launch_bounds__(256) void small_linear_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ w, int B, int I, int O,
                                                               float* __restrict__ dx, float* __restrict__ dw,
                                                               float* __restrict__ db, int nbx, int nbw) {
  small_linear_bwd_body(dy, x, w, B, I, O, dx, dw, db, nbx, nbw, blockIdx.x);
}

// The classifier's backward in one launch (CrossEntropyLoss -> Linear(512, 10), the reference's
// fc1 + criterion, /root/reference/src/Part 1/model.py:40-45 with main.py:39-40,110): every block
// first forms dlogits = (softmax(logits) - onehot(t)) * gscale / B for all B rows in its LDS (one
// thread per row, O <= 16 classes), block 0 also stores it (the loss's gradient autograd passes on),
// then the block does its part of the narrow Linear's gradients:
//   blocks [0, nbx)          16 columns i of dX x 32 rows (16 row lanes x 16 columns), each
//                            dX[r][i] = sum_o dy[r][o] W[o][i] in small_linear_bwd_body's order; with a
//                            BatchNorm link (lk.y != null: the input is the last VGG block's pooled,
//                            1x1 output, so column i is channel i) the block also reduces that block's
//                            BN backward partials from the dX it just formed -- sum dz, sum dz * xhat,
//                            sum xhat over each 2x2 window through max-pool + ReLU, as bn_bwd_reduce --
//                            into part[row chunk][i][0..ps), so the block's backward takes them instead of a
//                            statistics launch of its own (ops/functional.py _BNLink)
//   blocks [nbx, nbx + nbw)  dW, last block db (small_linear_bwd_body)
// Three launches (xent_bwd, small_linear_bwd, bn_bwd_reduce) and two kernel boundaries less per step.
// LS (label smoothing eps > 0): dlogits = (softmax - (1 - eps) onehot(t) - eps / O) * gscale / B, as
// xent_bwd_kernel<true>; the sdy tile then carries the smoothed gradient and nothing else differs.
// MIX (tgt_b, lam: xent_bwd_kernel<., true>'s gradient, bit for bit, for every eps): the butterfly sum
// order whatever eps is, and xent_mix_grad's rounding steps.
// BCE (binary cross-entropy, bce_bwd_kernel<MIX>'s gradient, bit for bit): only the rows' dlogits differ,
// dlogits = (sigmoid(z) - y) * gscale / (B O), or / B; no softmax, so nothing is reduced over the classes.
// LS is not read (eps is: it shapes y). The instantiations without BCE do not read ba.
template <bool LS, bool MIX, bool BCE = false>
__global__ __launch_bounds__(256) void xent_linear_bwd_kernel(const float* __restrict__ logits,
                                                              const long long* __restrict__ tgt,
                                                              const float* __restrict__ gscale,
                                                              const float* __restrict__ x, const float* __restrict__ w,
                                                              int B, int I, int O, float* __restrict__ dlogits,
                                                              float* __restrict__ dx, float* __restrict__ dw,
                                                              float* __restrict__ db, int nbx, int nbw, XentBnLink lk,
                                                              float eps, const long long* __restrict__ tgt_b,
                                                              const float* __restrict__ lam_p, BceArgs ba) {
  __shared__ float sdy[kXentLinMax];
  const float k = BCE ? bce_k(gscale[0], B, O, ba.sum_classes) : gscale[0] / (float)B;
  const float on = 1.f - eps, off = eps / (float)O;  // (LS only)
  XentMixW mw{0.f, 0.f, 0.f};
  if (MIX) mw = xent_mix_w(lam_p[0], eps, O);
  else if (BCE) mw = xent_mix_w(1.f, eps, O);
  for (int r = threadIdx.x; r < B; r += 256) {
    const float* row = logits + (long long)r * O;
    if (BCE) {
      const long long t = tgt[r];
      long long tb = -1;
      if (MIX) tb = tgt_b[r];
      for (int o = 0; o < O; ++o) {
        const float d = bce_grad(row[o], bce_y(o == t, o == tb, mw, ba), k);
        sdy[r * O + o] = d;
        if (blockIdx.x == 0) dlogits[(long long)r * O + o] = d;
      }
      continue;
    }
    float v[SL_MAXO];
    float mx = -INFINITY;
#pragma unroll
    for (int o = 0; o < SL_MAXO; ++o) {
      v[o] = o < O ? row[o] : -INFINITY;
      mx = fmaxf(mx, v[o]);
    }
    float se = 0.f;
    if (LS || MIX) {
      // the sum in the order of xent_bwd_kernel's wave_sum (a xor butterfly over the lanes o < 16;
      // o >= O adds exact zeros): the smoothed gradient of the fused and of the unfused classifier
      // backward are then the same bits. (The plain sum below differs from that kernel's by an ulp.)
      static_assert(SL_MAXO == 16, "the butterfly below is written for 16 classes");
      float e[SL_MAXO];
#pragma unroll
      for (int o = 0; o < SL_MAXO; ++o) e[o] = o < O ? expf(v[o] - mx) : 0.f;
#pragma unroll
      for (int h = SL_MAXO / 2; h > 0; h >>= 1) {
#pragma unroll
        for (int o = 0; o < h; ++o) e[o] += e[o + h];
      }
      se = e[0];
    } else {
#pragma unroll
      for (int o = 0; o < SL_MAXO; ++o)
        if (o < O) se += expf(v[o] - mx);
    }
    const float inv = 1.f / se;
    const long long t = tgt[r];
    long long tb = -1;
    if (MIX) tb = tgt_b[r];
#pragma unroll
    for (int o = 0; o < SL_MAXO; ++o) {
      if (o >= O) break;
      const float d = MIX  ? xent_mix_grad(expf(v[o] - mx), inv, o == t, o == tb, mw, k)
                      : LS ? (expf(v[o] - mx) * inv - (o == t ? on : 0.f) - off) * k
                           : (expf(v[o] - mx) * inv - (o == t ? 1.f : 0.f)) * k;
      sdy[r * O + o] = d;
      if (blockIdx.x == 0) dlogits[(long long)r * O + o] = d;
    }
  }
  __syncthreads();
  if ((int)blockIdx.x >= nbx) {
    small_linear_bwd_body(sdy, x, w, B, I, O, nullptr, dw, db, 0, nbw, blockIdx.x - nbx);
    return;
  }
  __shared__ float red[3][16][17];
  const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int ncol = (I + 15) / 16;
  const int chunk = blockIdx.x / ncol;  // rows [32 chunk, 32 chunk + 32): the BN partial index
  const int i = (blockIdx.x - chunk * ncol) * 16 + col;
  const bool ok = i < I;
  const int rend = min(B, kXentLinRows * (chunk + 1));
  float wc[SL_MAXO];
#pragma unroll
  for (int o = 0; o < SL_MAXO; ++o) wc[o] = ok ? w[(long long)min(o, O - 1) * I + i] : 0.f;
  float a1 = 0.f, a2 = 0.f, a3 = 0.f;
  float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
  const bool link = lk.y != nullptr && ok;
  if (link) {
    mu = lk.stats[i];
    is = lk.stats[I + i];
    sc = lk.stats[2 * I + i];
    sh = lk.stats[3 * I + i];
  }
  for (int r = kXentLinRows * chunk + rl; r < rend && ok; r += 16) {
    float s = 0.f;
    for (int o = 0; o < O; ++o) s = fmaf(sdy[r * O + o], wc[o], s);
    dx[(long long)r * I + i] = s;
    if (link) {
      // the block's 2x2 pre-BN window of channel i (lk.H = lk.W = 2) or its single pixel
      const int np = lk.pool ? 4 : 1;
      float yv[4], z[4], d[4];
      for (int p = 0; p < np; ++p) {
        yv[p] = lk.y[((long long)r * np + p) * I + i];  // NHWC, pixels (0,0),(0,1),(1,0),(1,1)
        z[p] = fmaf(yv[p], sc, sh);
        if (lk.relu) z[p] = fmaxf(z[p], 0.f);
      }
      if (lk.pool) {
        int arg = 0;
        float m = z[0];
        if (z[1] > m) { m = z[1]; arg = 1; }
        if (z[2] > m) { m = z[2]; arg = 2; }
        if (z[3] > m) { m = z[3]; arg = 3; }
        const float gg = (!lk.relu || m > 0.f) ? s : 0.f;
        for (int p = 0; p < 4; ++p) d[p] = arg == p ? gg : 0.f;
      } else {
        d[0] = (!lk.relu || z[0] > 0.f) ? s : 0.f;
      }
      for (int p = 0; p < np; ++p) {
        const float xh = (yv[p] - mu) * is;
        a1 += d[p];
        a2 += d[p] * xh;
        a3 += xh;
      }
    }
  }
  if (lk.y == nullptr) return;  // (uniform over the block)
  red[0][rl][col] = a1;
  red[1][rl][col] = a2;
  red[2][rl][col] = a3;
  __syncthreads();
  if (rl < lk.ps && ok) {
    float t = 0.f;
    for (int q = 0; q < 16; ++q) t += red[rl][q][col];
    lk.part[((long long)chunk * I + i) * lk.ps + rl] = t;
  }
}

// global average pool over HW of NHWC -> [N][C]; and its backward (32-bit index decode by
// multiply-shift: the launchers check the sizes)
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const float* __restrict__ x, int N, int HW, int C,
                                                          float* __restrict__ y, FastDiv fd_C) {
  const int total = N * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int n = fdiv(i, fd_C);
    const int c = i - n * C;
    float s = 0.f;
    for (int k = 0; k < HW; ++k) s += x[((long long)n * HW + k) * C + c];
    y[i] = s / (float)HW;
  }
}
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ gy, int N, int HW, int C,
                                                          float* __restrict__ gx, FastDiv fd_C, FastDiv fd_HW) {
  const int total = N * HW * C;
  const float inv = 1.f / (float)HW;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int pix = fdiv(i, fd_C);
    const int c = i - pix * C;
    const int n = fdiv(pix, fd_HW);
    gx[i] = gy[n * C + c] * inv;
  }
}

// MaxPool2d(k, s, p) forward on NHWC with int32 argmax (flat h*W+w), and backward (scatter-add).
// Max-pool on NHWC, float4 along C. The argmax is kept as the window-local tap index (uint8,
// first max wins in (dh, dw) scan order like ATen), a quarter of an int32 index map. A window that
// holds a NaN returns NaN and the tap of its last NaN (ATen's val > max || isnan(val)).
// 32-bit indices with multiply-shift division (the launchers check the sizes): the 64-bit divisions
// the index decode took before were ~40 instructions each, four per element, in passes that are
// otherwise bandwidth-bound
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C,
                                                          int k, int s, int pd, int Ho, int Wo, float* __restrict__ y,
                                                          unsigned char* __restrict__ arg, FastDiv fd_C4, FastDiv fd_Wo,
                                                          FastDiv fd_Ho) {
  const int C4 = C >> 2;
  const int total = N * Ho * Wo * C4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int pix = fdiv(i, fd_C4);
    const int c4 = i - pix * C4;
    const int t = fdiv(pix, fd_Wo);
    const int wo = pix - t * Wo;
    const int n = fdiv(t, fd_Ho);
    const int ho = t - n * Ho;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int am[4] = {-1, -1, -1, -1};
    const float* base = x + (long long)n * H * W * C + 4 * c4;
    for (int dh = 0; dh < k; ++dh) {
      const int h = ho * s - pd + dh;
      if ((unsigned)h >= (unsigned)H) continue;
      for (int dw = 0; dw < k; ++dw) {
        const int w = wo * s - pd + dw;
        if ((unsigned)w >= (unsigned)W) continue;
        const float4 v = ld4(base + ((long long)h * W + w) * C);
        const float vv[4] = {v.x, v.y, v.z, v.w};
        const int tap = dh * k + dw;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (vv[e] > m[e] || am[e] < 0 || vv[e] != vv[e]) {  // a NaN always wins: the window's last one stays
            m[e] = vv[e];
            am[e] = tap;
          }
      }
    }
    st4(y + (long long)pix * C + 4 * c4, make_float4(m[0], m[1], m[2], m[3]));
    *reinterpret_cast<uchar4*>(arg + (long long)pix * C + 4 * c4) =
        make_uchar4((unsigned char)am[0], (unsigned char)am[1], (unsigned char)am[2], (unsigned char)am[3]);
  }
}

// Gather form of the backward (no atomics, no zero fill): every input element sums the gradients
// of the windows that cover it and whose argmax tap is this element.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ gy,
                                                          const unsigned char* __restrict__ arg, int N, int H, int W,
                                                          int C, int k, int s, int pd, int Ho, int Wo,
                                                          float* __restrict__ gx, FastDiv fd_C4, FastDiv fd_W,
                                                          FastDiv fd_H) {
  const int C4 = C >> 2;
  const int total = N * H * W * C4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int pix = fdiv(i, fd_C4);
    const int c4 = i - pix * C4;
    const int t = fdiv(pix, fd_W);
    const int w = pix - t * W;
    const int n = fdiv(t, fd_H);
    const int h = t - n * H;
    // windows ho with ho*s - pd <= h <= ho*s - pd + k - 1
    const int ho0 = max(0, (h + pd - k + s) / s), ho1 = min(Ho - 1, (h + pd) / s);
    const int wo0 = max(0, (w + pd - k + s) / s), wo1 = min(Wo - 1, (w + pd) / s);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ho = ho0; ho <= ho1; ++ho)
      for (int wo = wo0; wo <= wo1; ++wo) {
        const int tap = (h - (ho * s - pd)) * k + (w - (wo * s - pd));
        const long long o = (((long long)n * Ho + ho) * Wo + wo) * C + 4 * c4;
        const uchar4 a = *reinterpret_cast<const uchar4*>(arg + o);
        const float4 v = ld4(gy + o);
        if (a.x == tap) g[0] += v.x;
        if (a.y == tap) g[1] += v.y;
        if (a.z == tap) g[2] += v.z;
        if (a.w == tap) g[3] += v.w;
      }
    st4(gx + (long long)pix * C + 4 * c4, make_float4(g[0], g[1], g[2], g[3]));
  }
}

int grid_for(long long n) {
  long long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}



// sub-filter transpose for the sub-pixel data gradient: wt[ci][a][b][co] = w[co][kh0+2a][kw0+2b][ci]
__global__ __launch_bounds__(256) void wtrans_sub_kernel(const float* __restrict__ w, float* __restrict__ wt, int Co,
                                                         int KH, int KW, int Ci, int kh0, int kw0, int nkw) {
  __shared__ float tile[32][33];
  const int t = blockIdx.z;  // sub-tap a * nkw + b
  const int tap_in = (kh0 + 2 * (t / nkw)) * KW + kw0 + 2 * (t % nkw);
  const int T_in = KH * KW, T_out = gridDim.z;
  const int co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    const int co = co0 + j, ci = ci0 + tx;
    tile[j][tx] = (co < Co && ci < Ci) ? w[((long long)co * T_in + tap_in) * Ci + ci] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int ci = ci0 + j, co = co0 + tx;
    if (ci < Ci && co < Co) wt[((long long)ci * T_out + t) * Co + co] = tile[tx][j];
  }
}
}  // namespace

int sgd_grid(long long n) { return grid_for((n + 3) / 4); }

void xent_fwd_launch(const float* logits, const long long* tgt, int B, int C, float* loss, long long* correct,
                     float* sum_out, hipStream_t st, float eps, int topk, const long long* tgt_b, const float* lam) {
  if (!(eps >= 0.f && eps <= 1.f) || topk < 1) throw std::runtime_error("xent_fwd: label smoothing in [0, 1], topk >= 1");
  if ((tgt_b != nullptr) != (lam != nullptr)) throw std::runtime_error("xent_fwd: tgt_b and lam go together");
  // eps == 0 and topk == 1 take the plain instantiation: the arithmetic of a call without them
  const bool ls = eps != 0.f, tk = topk > 1;
  if (tgt_b) {
    if (correct || tk) throw std::runtime_error("xent_fwd: no correct count with a second target");
    auto kern = ls ? xent_fwd_kernel<true, false, true> : xent_fwd_kernel<false, false, true>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, st, logits, tgt, B, C, loss, correct, sum_out, eps, topk, tgt_b,
                       lam);
    return;
  }
  auto kern = ls ? (tk ? xent_fwd_kernel<true, true, false> : xent_fwd_kernel<true, false, false>)
                 : (tk ? xent_fwd_kernel<false, true, false> : xent_fwd_kernel<false, false, false>);
  hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, st, logits, tgt, B, C, loss, correct, sum_out, eps, topk, tgt_b,
                     lam);
}
void xent_bwd_launch(const float* logits, const long long* tgt, const float* gscale, int B, int C, float* dlogits,
                     hipStream_t st, float eps, const long long* tgt_b, const float* lam) {
  if (!(eps >= 0.f && eps <= 1.f)) throw std::runtime_error("xent_bwd: label smoothing in [0, 1]");
  if ((tgt_b != nullptr) != (lam != nullptr)) throw std::runtime_error("xent_bwd: tgt_b and lam go together");
  auto kern = tgt_b ? (eps != 0.f ? xent_bwd_kernel<true, true> : xent_bwd_kernel<false, true>)
                    : (eps != 0.f ? xent_bwd_kernel<true, false> : xent_bwd_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3((B + 3) / 4), dim3(256), 0, st, logits, tgt, gscale, B, C, dlogits, eps, tgt_b, lam);
}
namespace {
BceArgs bce_args(const char* op, float eps, const float* thr, bool sum_classes, const long long* tgt_b,
                 const float* lam) {
  const std::string o(op);
  if (!(eps >= 0.f && eps <= 1.f)) throw std::runtime_error(o + ": label smoothing in [0, 1]");
  if (thr && !(*thr >= 0.f && *thr < 1.f)) throw std::runtime_error(o + ": target threshold in [0, 1)");
  if ((tgt_b != nullptr) != (lam != nullptr)) throw std::runtime_error(o + ": tgt_b and lam go together");
  return BceArgs{thr ? *thr : 0.f, thr ? 1 : 0, sum_classes ? 1 : 0};
}
}  // namespace
void bce_fwd_launch(const float* logits, const long long* tgt, int B, int C, float* loss, hipStream_t st, float eps,
                    const float* thr, bool sum_classes, const long long* tgt_b, const float* lam) {
  const BceArgs ba = bce_args("bce_fwd", eps, thr, sum_classes, tgt_b, lam);
  auto kern = tgt_b ? bce_fwd_kernel<true> : bce_fwd_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, st, logits, tgt, B, C, loss, eps, ba, tgt_b, lam);
}
void bce_bwd_launch(const float* logits, const long long* tgt, const float* gscale, int B, int C, float* dlogits,
                    hipStream_t st, float eps, const float* thr, bool sum_classes, const long long* tgt_b,
                    const float* lam) {
  const BceArgs ba = bce_args("bce_bwd", eps, thr, sum_classes, tgt_b, lam);
  if (B <= 0) return;
  auto kern = tgt_b ? bce_bwd_kernel<true> : bce_bwd_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((B + 3) / 4), dim3(256), 0, st, logits, tgt, gscale, B, C, dlogits, eps, ba, tgt_b, lam);
}
void lr_sched_advance_launch(const SchedArgs& sched, const float* lr_ptr, float lr, hipStream_t st) {
  if (!sched.state || !sched.cfg) throw std::runtime_error("lr_sched_advance: state and cfg required");
  hipLaunchKernelGGL(lr_sched_advance_kernel, dim3(1), dim3(1), 0, st, sched, lr_ptr, lr);
}
void lr_sched_table_launch(const LrSchedCfg* cfg, const float* lr_ptr, float lr, long long first, long long n,
                           float* out, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lr_sched_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cfg, lr_ptr, lr, first,
                     n, out);
}
// The SGD kernels come in 16 instantiations each: CLIP x LARS x EMA x SCHED. SCHED is a template
// parameter like the others, so that the instantiations without it are the code they were before it
// existed (no LDS word, no barrier, no branch).
void sgd_launch(float* p, const float* g, float* buf, long long n, const float* lr_ptr, float lr, float momentum,
                float dampening, float wd, float grad_scale, bool nesterov, bool first, bool maximize,
                hipStream_t st, long long* counter, const ClipArgs& clip, const LarsArgs& lars, const EmaArgs& ema,
                const SchedArgs& sched) {
  const int flags = (nesterov ? 1 : 0) | (first ? 2 : 0) | (maximize ? 4 : 0) | (momentum != 0.f ? 8 : 0);
  if ((ema.e != nullptr) != (ema.coef != nullptr)) throw std::runtime_error("sgd: ema and ema_coef go together");
  if ((sched.state != nullptr) != (sched.cfg != nullptr)) throw std::runtime_error("sgd: sched state and cfg go together");
  if (lars.params && lars.nitems < 1) {
    if (sched.state && sched.advance) lr_sched_advance_launch(sched, lr_ptr, lr, st);  // a step all the same
    return;
  }
  // LARS: one workgroup per item of the work list, which tiles [0, n)
  const dim3 grid(lars.params ? lars.nitems : grid_for((n + 3) / 4));
#define CDP_SGD(CLIP, LARS, EMA, SCHED)                                                                               \
  hipLaunchKernelGGL((sgd_kernel<CLIP, LARS, EMA, SCHED>), grid, dim3(256), 0, st, p, g, buf, n, lr_ptr, lr, momentum, \
                     dampening, wd, grad_scale, flags, counter, clip, lars, ema, sched)
#define CDP_SGD_S(CLIP, LARS, EMA)                   \
  do {                                               \
    if (sched.state) CDP_SGD(CLIP, LARS, EMA, true); \
    else CDP_SGD(CLIP, LARS, EMA, false);            \
  } while (0)
#define CDP_SGD_E(CLIP, LARS)               \
  do {                                      \
    if (ema.e) CDP_SGD_S(CLIP, LARS, true); \
    else CDP_SGD_S(CLIP, LARS, false);      \
  } while (0)
  if (lars.params) {
    if (clip.part) CDP_SGD_E(true, true);
    else CDP_SGD_E(false, true);
  } else {
    if (clip.part) CDP_SGD_E(true, false);
    else CDP_SGD_E(false, false);
  }
#undef CDP_SGD_E
#undef CDP_SGD_S
#undef CDP_SGD
}
void sgd_prep_launch(float* p, const float* g, float* buf, const SgdPrepSeg* segs, int nseg, int nblk_w,
                     const SgdPrepChunk* chunks, int nchunk, float* wmax, const float* lr_ptr, float lr,
                     float momentum, float dampening, float wd, float grad_scale, bool nesterov, bool first,
                     bool maximize, hipStream_t st, long long* counter, const ClipArgs& clip, const LarsArgs& lars,
                     const EmaArgs& ema, const SchedArgs& sched) {
  const int flags = (nesterov ? 1 : 0) | (first ? 2 : 0) | (maximize ? 4 : 0) | (momentum != 0.f ? 8 : 0);
  if ((ema.e != nullptr) != (ema.coef != nullptr)) throw std::runtime_error("sgd: ema and ema_coef go together");
  if ((sched.state != nullptr) != (sched.cfg != nullptr)) throw std::runtime_error("sgd: sched state and cfg go together");
  if (nblk_w + nchunk <= 0) {
    if (sched.state && sched.advance) lr_sched_advance_launch(sched, lr_ptr, lr, st);  // a step all the same
    return;
  }
#define CDP_SGD_PREP_S(CLIP, LARS, EMA, SCHED)                                                                      \
  hipLaunchKernelGGL((sgd_prep_kernel<CLIP, LARS, EMA, SCHED>), dim3(nblk_w + nchunk), dim3(256), 0, st, p, g, buf, \
                     segs, nseg, nblk_w, chunks, wmax, lr_ptr, lr, momentum, dampening, wd, grad_scale, flags,      \
                     counter, clip, lars, ema, sched)
#define CDP_SGD_PREP_E(CLIP, LARS, EMA)                   \
  do {                                                    \
    if (sched.state) CDP_SGD_PREP_S(CLIP, LARS, EMA, true); \
    else CDP_SGD_PREP_S(CLIP, LARS, EMA, false);          \
  } while (0)
#define CDP_SGD_PREP(CLIP, LARS)                 \
  do {                                           \
    if (ema.e) CDP_SGD_PREP_E(CLIP, LARS, true); \
    else CDP_SGD_PREP_E(CLIP, LARS, false);      \
  } while (0)
  if (lars.params) {
    if (clip.part) CDP_SGD_PREP(true, true);
    else CDP_SGD_PREP(false, true);
  } else {
    if (clip.part) CDP_SGD_PREP(true, false);
    else CDP_SGD_PREP(false, false);
  }
#undef CDP_SGD_PREP
#undef CDP_SGD_PREP_E
#undef CDP_SGD_PREP_S
}
namespace {
bool erase_cfg_ok(const EraseCfg& e) {
  return e.prob >= 0.f && e.prob <= 1.f && e.scale_lo > 0.f && e.scale_lo <= e.scale_hi && e.scale_hi <= 1.f &&
         e.log_ratio_lo <= e.log_ratio_hi && e.mode >= kEraseConst && e.mode <= kErasePixel &&
         std::isfinite(e.value[0]) && std::isfinite(e.value[1]) && std::isfinite(e.value[2]);
}
const char* const kEraseCfgMsg =
    ": erase prob in [0, 1], 0 < scale_lo <= scale_hi <= 1, ratio_lo <= ratio_hi, mode const / rand / pixel, finite values";
}  // namespace
void augment_launch(const unsigned char* imgs, const long long* idx, long long idx_off, int B, int H, int W, int C,
                    const float* mean, const float* inv_std, int pad, bool flip, const long long* counter,
                    unsigned long long seed, float* out, hipStream_t st, long long nbatches,
                    const long long* labels, long long* labels_out, const MixCfg& cfg, float* mix,
                    long long* labels_b, const EraseCfg& ecfg, int* erase) {
  dim3 grid((H * W + 255) / 256, B);
  // both alphas 0: the instantiation without mixing, whose output does not depend on cfg
  const bool mixing = mix_enabled(cfg);
  if (mixing && (!mix || (labels_b && !labels)))
    throw std::runtime_error("augment: mixing needs the mix row (and labels for labels_b)");
  if (!(cfg.mixup_alpha >= 0.f && cfg.cutmix_alpha >= 0.f && cfg.prob >= 0.f && cfg.prob <= 1.f &&
        cfg.switch_prob >= 0.f && cfg.switch_prob <= 1.f))
    throw std::runtime_error("augment: mix alphas >= 0 and probabilities in [0, 1]");
  // prob 0: the instantiations without erasing, the kernels of a launch without these arguments
  const bool erasing = erase_enabled(ecfg);
  if (!erase_cfg_ok(ecfg)) throw std::runtime_error(std::string("augment") + kEraseCfgMsg);
  if (erasing && (!erase || C != 3))
    throw std::runtime_error("augment: erasing needs the erase rows and 3-channel images");
  auto kern = mixing ? (erasing ? augment_kernel<true, true> : augment_kernel<true, false>)
                     : (erasing ? augment_kernel<false, true> : augment_kernel<false, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, imgs, idx, idx_off, B, H, W, C, mean[0], mean[1], mean[2],
                     inv_std[0], inv_std[1], inv_std[2], pad, flip ? 1 : 0, counter, seed, out, nbatches, labels,
                     labels_out, cfg, mix, labels_b, ecfg, erase);
}
void mix_params_launch(unsigned long long seed, long long first, long long n, const MixCfg& cfg, int H, int W,
                       float* mix, hipStream_t st) {
  if (n <= 0) return;
  if (!(cfg.mixup_alpha >= 0.f && cfg.cutmix_alpha >= 0.f && cfg.prob >= 0.f && cfg.prob <= 1.f &&
        cfg.switch_prob >= 0.f && cfg.switch_prob <= 1.f) || H < 1 || W < 1)
    throw std::runtime_error("mix_params: mix alphas >= 0, probabilities in [0, 1], H, W >= 1");
  hipLaunchKernelGGL(mix_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, seed, first, n, cfg, H, W,
                     mix);
}
namespace {
bool rrc_cfg_ok(const RrcCfg& rc) {
  return rc.scale_lo > 0.f && rc.scale_lo <= rc.scale_hi && rc.scale_hi <= 1.f && rc.log_ratio_lo <= rc.log_ratio_hi;
}
}  // namespace
void augment_resize_launch(const unsigned char* imgs, const long long* idx, long long idx_off, int B, int H, int W,
                           int C, int OH, int OW, const float* mean, const float* inv_std, bool train,
                           const RrcCfg& rc, double center_frac, bool flip, const long long* counter,
                           unsigned long long seed, float* out, hipStream_t st, long long nbatches,
                           const long long* labels, long long* labels_out, int* crops, const MixCfg& cfg, float* mix,
                           long long* labels_b, const EraseCfg& ecfg, int* erase) {
  if (C != 3) throw std::runtime_error("augment_resize: 3-channel images only");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || OH < 1 || OW < 1 || H > 0x7fff || W > 0x7fff || OH > 0x7fff || OW > 0x7fff)
    throw std::runtime_error("augment_resize: 1 <= batch < 65536 and 1 <= H, W, out_h, out_w < 32768");
  if (!crops || (labels_out && !labels)) throw std::runtime_error("augment_resize: crops (and labels for labels_out) needed");
  if (!rrc_cfg_ok(rc) || !(center_frac > 0.0 && center_frac <= 1.0))
    throw std::runtime_error("augment_resize: 0 < scale_lo <= scale_hi <= 1, ratio_lo <= ratio_hi, 0 < center_frac <= 1");
  const bool mixing = mix_enabled(cfg);
  if (mixing && (!mix || (labels_b && !labels)))
    throw std::runtime_error("augment_resize: mixing needs the mix row (and labels for labels_b)");
  if (!(cfg.mixup_alpha >= 0.f && cfg.cutmix_alpha >= 0.f && cfg.prob >= 0.f && cfg.prob <= 1.f &&
        cfg.switch_prob >= 0.f && cfg.switch_prob <= 1.f))
    throw std::runtime_error("augment_resize: mix alphas >= 0 and probabilities in [0, 1]");
  // the eval window: the central (round(frac H), round(frac W)), ties to even as Python's round()
  const int eh = std::max(1, std::min(H, (int)std::nearbyint(center_frac * H)));
  const int ew = std::max(1, std::min(W, (int)std::nearbyint(center_frac * W)));
  // few, large workgroups per image: every thread keeps its 4 columns over about 4 rows, and small
  // batches still fill the chip
  const int nq = (OW + 3) / 4;
  const int rpp = 256 / std::min(nq, 256);
  const int passes = (OH + rpp - 1) / rpp;
  int gx = (passes + 3) / 4;
  if ((long long)gx * B < 512) gx = std::min(passes, (512 + B - 1) / B);
  const int vec = (OW % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  const bool erasing = erase_enabled(ecfg);
  if (!erase_cfg_ok(ecfg)) throw std::runtime_error(std::string("augment_resize") + kEraseCfgMsg);
  if (erasing && !erase) throw std::runtime_error("augment_resize: erasing needs the erase rows");
  auto kern = mixing ? (erasing ? augment_resize_kernel<true, true> : augment_resize_kernel<true, false>)
                     : (erasing ? augment_resize_kernel<false, true> : augment_resize_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(gx, B), dim3(256), 0, st, imgs, idx, idx_off, B, H, W, OH, OW, mean[0], mean[1],
                     mean[2], inv_std[0], inv_std[1], inv_std[2], train ? 1 : 0, rc, eh, ew, flip ? 1 : 0, counter,
                     seed, out, nbatches, labels, labels_out, crops, cfg, mix, labels_b, vec, ecfg, erase);
}
void erase_params_launch(unsigned long long seed, long long first, long long n, int B, const EraseCfg& ecfg, int H,
                         int W, int* rows, hipStream_t st) {
  if (n <= 0 || B <= 0) return;
  if (!erase_cfg_ok(ecfg) || H < 1 || W < 1 || H > 0x7fff || W > 0x7fff)
    throw std::runtime_error(std::string("erase_params: 1 <= H, W < 32768") + kEraseCfgMsg);
  const long long total = n * B;
  hipLaunchKernelGGL(erase_params_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, seed, first, total,
                     B, ecfg, H, W, rows);
}
void erase_noise_launch(unsigned long long seed, long long counter, int B, int H, int W, float* out, hipStream_t st) {
  if (B <= 0) return;
  if (B > 65535 || H < 1 || W < 1 || H > 0x7fff || W > 0x7fff)
    throw std::runtime_error("erase_noise: batch < 65536 and 1 <= H, W < 32768");
  const long long per3 = 3LL * H * W;
  hipLaunchKernelGGL(erase_noise_kernel, dim3(grid_for(per3 * B)), dim3(256), 0, st, seed,
                     (unsigned long long)counter, per3 * B, per3, out);
}
void rrc_params_launch(unsigned long long seed, long long first, long long n, int B, const RrcCfg& rc, int H, int W,
                       int* win, hipStream_t st) {
  if (n <= 0 || B <= 0) return;
  if (!rrc_cfg_ok(rc) || H < 1 || W < 1 || H > 0x7fff || W > 0x7fff)
    throw std::runtime_error("rrc_params: 0 < scale_lo <= scale_hi <= 1, ratio_lo <= ratio_hi, 1 <= H, W < 32768");
  const long long total = n * B;
  hipLaunchKernelGGL(rrc_params_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, seed, first, total, B,
                     rc, H, W, win);
}
void subpixel_zero_launch(float* dx, int N, int H, int W, int C, int mask, hipStream_t st) {
  if ((long long)N * H * W >= (1LL << 31) || (C & 3)) throw std::runtime_error("subpixel_zero: bad shape");
  const long long n4 = (long long)N * H * W * (C / 4);
  hipLaunchKernelGGL(subpixel_zero_kernel, dim3(grid_for(n4)), dim3(256), 0, st, dx, N, H, W, C / 4, mask,
                     make_fastdiv(C / 4), make_fastdiv(W));
}
// Zero-fill as a kernel (act-max slot chunks, ops.cpp alloc_slots): a kernel node of a captured
// graph is ordered like every other kernel of the step
__global__ __launch_bounds__(256) void fill_u32_kernel(unsigned* __restrict__ p, long long n, unsigned v) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = v;
}
__global__ __launch_bounds__(256) void fill_u32x4_kernel(uint4* __restrict__ p, long long n4, unsigned v) {
  const uint4 q = make_uint4(v, v, v, v);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
    p[i] = q;
}
void fill_u32_launch(unsigned* p, long long n, unsigned v, hipStream_t st) {
  if (n <= 0) return;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (n & 3) == 0) {  // 16-B stores (slot chunks: 256-B multiples)
    const long long n4 = n / 4, blocks = std::min<long long>(512, (n4 + 255) / 256);
    hipLaunchKernelGGL(fill_u32x4_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint4*>(p), n4, v);
    return;
  }
  const long long blocks = std::min<long long>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(fill_u32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, n, v);
}
// Device-to-device copy as a kernel (the root's own block of the grouped gather / scatter): inside a
// captured step a kernel node is ordered like the collectives around it (a captured memset node was
// measured to race, see fill_u32_kernel)
__global__ __launch_bounds__(256) void copy16_kernel(uint4* __restrict__ d, const uint4* __restrict__ s, long long n16) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x)
    d[i] = s[i];
}
__global__ __launch_bounds__(256) void copy1_kernel(unsigned char* __restrict__ d, const unsigned char* __restrict__ s,
                                                    long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    d[i] = s[i];
}
void copy_bytes_launch(void* dst, const void* src, long long bytes, hipStream_t st) {
  if (bytes <= 0) return;
  const bool wide = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src) | (uintptr_t)bytes) & 15) == 0;
  const long long n = wide ? bytes / 16 : bytes;
  const long long blocks = std::max<long long>(1, std::min<long long>(2048, (n + 255) / 256));
  if (wide)
    hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<uint4*>(dst),
                       static_cast<const uint4*>(src), n);
  else
    hipLaunchKernelGGL(copy1_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<unsigned char*>(dst),
                       static_cast<const unsigned char*>(src), n);
}
void counter_inc_launch(long long* c, hipStream_t st) {
  hipLaunchKernelGGL(counter_inc_kernel, dim3(1), dim3(1), 0, st, c);
}
void weight_prep_launch(const WeightPrepArgs& a, float* part, hipStream_t st) {
  hipLaunchKernelGGL(weight_prep_kernel, dim3(a.blk0[a.nseg]), dim3(256), 0, st, a, part);
}
void wtrans_launch(const float* w, float* wt, int Co, int T, int Ci, hipStream_t st) {
  dim3 grid((Ci + 31) / 32, (Co + 31) / 32, T);
  hipLaunchKernelGGL(wtrans_kernel, grid, dim3(256), 0, st, w, wt, Co, T, Ci);
}
void pad_c4_launch(const float* x, int N, long long HW, int C, float* out, ActMaxOut am, hipStream_t st) {
  const long long npix = (long long)N * HW;
  const int grid = (int)std::min<long long>(1024, std::max<long long>(1, (npix + 255) / 256));
  hipLaunchKernelGGL(pad_c4_kernel, dim3(grid), dim3(256), 0, st, x, N, HW, C, out, make_fastdiv((int)HW), am);
}
void stack_mean_launch(const float* const* srcs, int k, long long n, float* dst, hipStream_t st) {
  StackSrcs a{};
  for (int j = 0; j < k && j < kMaxStackSrcs; ++j) a.p[j] = srcs[j];
  hipLaunchKernelGGL(stack_mean_kernel, dim3(grid_for(n)), dim3(256), 0, st, a, k < kMaxStackSrcs ? k : kMaxStackSrcs, n,
                     dst);
}
// Test-only post-op (RcclComm::set_test_postop): every wave first idles ~delay_us with s_sleep
// (no memory traffic), then scales. Used to prove that consumers wait on the collective's event.
__global__ __launch_bounds__(256) void delay_scale_kernel(float* __restrict__ x, long long n, float a, int sleeps) {
  for (int i = 0; i < sleeps; ++i) __builtin_amdgcn_s_sleep(127);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    x[i] *= a;
}

// One thread writes the GPU's constant-rate wall clock (s_memrealtime, 100 MHz) into ts[idx]:
// a stream-ordered timestamp far cheaper than a timing event (which ends in a release barrier).
__global__ void timestamp_kernel(long long* ts, int idx) { ts[idx] = (long long)wall_clock64(); }

void timestamp_launch(long long* ts, int idx, hipStream_t st) {
  hipLaunchKernelGGL(timestamp_kernel, dim3(1), dim3(1), 0, st, ts, idx);
}

void delay_scale_launch(float* x, long long n, float a, double delay_us, hipStream_t st) {
  // s_sleep 127 ~ 127*64 cycles ~ 3.4 us at 2.4 GHz
  const int sleeps = (int)(delay_us / 3.4) + 1;
  if (a == 1.f) {
    // a pure delay (the modelled all-reduce time): 16 sleeping workgroups, about the CUs an RCCL
    // all-reduce's channels occupy, so the compute stream keeps the rest of the chip
    hipLaunchKernelGGL(delay_scale_kernel, dim3(16), dim3(64), 0, st, x, 0LL, a, sleeps);
    return;
  }
  hipLaunchKernelGGL(delay_scale_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, n, a, sleeps);
}
void scale_launch(float* x, long long n, float a, hipStream_t st) {
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, n, a);
}
void colsum_launch(const float* x, int R, int C, float* out, bool accumulate, hipStream_t st) {
  hipLaunchKernelGGL(colsum_kernel, dim3((C + 63) / 64), dim3(256), 0, st, x, R, C, out, accumulate ? 1 : 0);
}
void small_linear_fwd_launch(const float* x, const float* w, const float* b, int B, int I, int O, float* y,
                             hipStream_t st) {
  hipLaunchKernelGGL(small_linear_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, st, x, w, b, B, I, O, y);
}
void small_linear_bwd_launch(const float* dy, const float* x, const float* w, int B, int I, int O, float* dx, float* dw,
                             float* db, hipStream_t st) {
  const int nbx = dx ? (int)(((long long)B * I + 255) / 256) : 0;
  const int nbw = (I + 15) / 16;
  hipLaunchKernelGGL(small_linear_bwd_kernel, dim3(nbx + nbw + 1), dim3(256), 0, st, dy, x, w, B, I, O, dx, dw, db,
                     nbx, nbw);
}
void xent_linear_bwd_launch(const float* logits, const long long* tgt, const float* gscale, const float* x,
                            const float* w, int B, int I, int O, float* dlogits, float* dx, float* dw, float* db,
                            const XentBnLink& lk, hipStream_t st, float eps, const long long* tgt_b,
                            const float* lam, bool bce, const float* thr, bool sum_classes) {
  if (O > SL_MAXO || (long long)B * O > kXentLinMax) throw std::runtime_error("xent_linear_bwd: classifier too wide");
  if (lk.y && (!dx || lk.ps < 2 || lk.ps > 3)) throw std::runtime_error("xent_linear_bwd: BN link needs dX");
  if (!(eps >= 0.f && eps <= 1.f)) throw std::runtime_error("xent_linear_bwd: label smoothing in [0, 1]");
  const int nbx = dx ? ((I + 15) / 16) * xent_lin_chunks(B) : 0;
  const int nbw = (I + 15) / 16;
  if ((tgt_b != nullptr) != (lam != nullptr)) throw std::runtime_error("xent_linear_bwd: tgt_b and lam go together");
  if (!bce && (thr || sum_classes))
    throw std::runtime_error("xent_linear_bwd: target threshold and sum_classes belong to the BCE mode");
  BceArgs ba{0.f, 0, 0};
  if (bce) ba = bce_args("xent_linear_bwd", eps, thr, sum_classes, tgt_b, lam);
  auto kern = tgt_b ? (eps != 0.f ? xent_linear_bwd_kernel<true, true> : xent_linear_bwd_kernel<false, true>)
                    : (eps != 0.f ? xent_linear_bwd_kernel<true, false> : xent_linear_bwd_kernel<false, false>);
  if (bce) kern = tgt_b ? xent_linear_bwd_kernel<false, true, true> : xent_linear_bwd_kernel<false, false, true>;
  hipLaunchKernelGGL(kern, dim3(nbx + nbw + 1), dim3(256), 0, st, logits, tgt, gscale, x, w, B, I, O, dlogits, dx, dw,
                     db, nbx, nbw, lk, eps, tgt_b, lam, ba);
}
void avgpool_fwd_launch(const float* x, int N, int HW, int C, float* y, hipStream_t st) {
  if ((long long)N * HW * C >= (1LL << 31)) throw std::runtime_error("avgpool: tensor too large");
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(grid_for((long long)N * C)), dim3(256), 0, st, x, N, HW, C, y,
                     make_fastdiv(C));
}
void avgpool_bwd_launch(const float* gy, int N, int HW, int C, float* gx, hipStream_t st) {
  if ((long long)N * HW * C >= (1LL << 31)) throw std::runtime_error("avgpool: tensor too large");
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(grid_for((long long)N * HW * C)), dim3(256), 0, st, gy, N, HW, C, gx,
                     make_fastdiv(C), make_fastdiv(HW));
}
void maxpool_fwd_launch(const float* x, int N, int H, int W, int C, int k, int s, int p, int Ho, int Wo, float* y,
                        unsigned char* arg, hipStream_t st) {
  if ((long long)N * H * W * (C / 4) >= (1LL << 31)) throw std::runtime_error("maxpool: tensor too large");
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid_for((long long)N * Ho * Wo * (C / 4))), dim3(256), 0, st, x, N,
                     H, W, C, k, s, p, Ho, Wo, y, arg, make_fastdiv(C / 4), make_fastdiv(Wo), make_fastdiv(Ho));
}
void maxpool_bwd_launch(const float* gy, const unsigned char* arg, int N, int H, int W, int C, int k, int s, int p,
                        int Ho, int Wo, float* gx, hipStream_t st) {
  if ((long long)N * H * W * (C / 4) >= (1LL << 31)) throw std::runtime_error("maxpool: tensor too large");
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for((long long)N * H * W * (C / 4))), dim3(256), 0, st, gy, arg,
                     N, H, W, C, k, s, p, Ho, Wo, gx, make_fastdiv(C / 4), make_fastdiv(W), make_fastdiv(H));
}

void wtrans_sub_launch(const float* w, float* wt, int Co, int KH, int KW, int Ci, int kh0, int kw0, int nkh, int nkw,
                       hipStream_t st) {
  dim3 grid((Ci + 31) / 32, (Co + 31) / 32, nkh * nkw);
  hipLaunchKernelGGL(wtrans_sub_kernel, grid, dim3(256), 0, st, w, wt, Co, KH, KW, Ci, kh0, kw0, nkw);
}

}  // namespace cdp
