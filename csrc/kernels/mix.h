// Batch mixing (mixup, Zhang et al.; CutMix, Yun et al.) parameters, drawn on the device.
//
// One set of parameters per batch (timm's "batch" mode): mode, lam and the CutMix box are a pure
// function of (seed, step counter, cfg, H, W). Every workgroup of the augment kernel evaluates
// mix_draw itself from those inputs and gets the same bits, so mixing needs no launch of its own, no
// cross-block communication and no host-side draw: a replayed hipGraph sees a new mix every step.
//
// Random source: the counter-based hash of the augmentation (splitmix64), keyed by (seed, counter,
// a stream tag) and walked by a draw index. The crop / flip draws are keyed by (seed, counter, image)
// without the tag, so they are the same bits with mixing on or off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace cdp {

struct MixCfg {
  float mixup_alpha;   // Beta(alpha, alpha) of mixup; 0: mixup off
  float cutmix_alpha;  // Beta(alpha, alpha) of CutMix; 0: CutMix off
  float prob;          // probability that a batch is mixed at all
  float switch_prob;   // probability of CutMix when both are on
};
inline bool mix_enabled(const MixCfg& c) { return c.mixup_alpha > 0.f || c.cutmix_alpha > 0.f; }

constexpr int kMixNone = 0, kMixMixup = 1, kMixCutmix = 2;
constexpr int kMixRow = 8;  // floats of a published row: {mode, lam, lam_raw, y0, y1, x0, x1, 0}

struct MixParams {
  int mode;
  float lam;      // weight of the image itself (and of its label)
  float lam_raw;  // the Beta draw (CutMix: before the box was clipped to the image)
  int y0, y1, x0, x1;  // CutMix box [y0, y1) x [x0, x1) in output pixels
};

__host__ __device__ __forceinline__ unsigned long long mix_hash(unsigned long long x) {  // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct MixRng {
  unsigned long long key;
  unsigned k;
  // uniform in (0, 1): 23 hash bits + 1/2, exact in fp32, never 0 or 1
  __host__ __device__ __forceinline__ float uniform() {
    const unsigned long long r = mix_hash(key + (unsigned long long)(k++));
    return ((float)(unsigned)(r >> 41) + 0.5f) * (1.f / 8388608.f);
  }
  __host__ __device__ __forceinline__ float normal() {  // Box-Muller, one of the pair
    const float u1 = uniform(), u2 = uniform();
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
  }
};

// Gamma(a, 1), a > 0: Marsaglia-Tsang for a >= 1, Gamma(a + 1) U^(1/a) below. At most kMixTries
// proposals (each is accepted with probability > 0.95), then the distribution's bulk d: no kernel can
// spin here.
constexpr int kMixTries = 16;
__host__ __device__ __forceinline__ float mix_gamma(MixRng& g, float a) {
  const float boost = a < 1.f ? powf(g.uniform(), 1.f / a) : 1.f;
  const float d = (a < 1.f ? a + 1.f : a) - 1.f / 3.f;
  const float c = 1.f / sqrtf(9.f * d);
  float res = d;
  for (int i = 0; i < kMixTries; ++i) {  // (every lane of a workgroup takes the same trip count)
    const float x = g.normal();
    const float u = g.uniform();
    const float t = 1.f + c * x;
    const float v = t * t * t;
    if (v > 0.f && logf(u) < 0.5f * x * x + d - d * v + d * logf(v)) {
      res = d * v;
      break;
    }
  }
  return res * boost;
}

__host__ __device__ __forceinline__ int mix_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The stream tag keeps these draws apart from the crop / flip hash of every image index.
__host__ __device__ __forceinline__ MixParams mix_draw(unsigned long long seed, unsigned long long ctr,
                                                       const MixCfg& cfg, int H, int W) {
  MixRng g{mix_hash(mix_hash(seed ^ 0x6D69782D73747265ull) ^ mix_hash(ctr + 0x632D6D69782D3031ull)), 0u};
  MixParams p{kMixNone, 1.f, 1.f, 0, 0, 0, 0};
  const bool mu = cfg.mixup_alpha > 0.f, cm = cfg.cutmix_alpha > 0.f;
  const float u_on = g.uniform(), u_sw = g.uniform();
  if (!(mu || cm) || !(u_on < cfg.prob)) return p;
  const bool cut = cm && (!mu || u_sw < cfg.switch_prob);
  const float a = cut ? cfg.cutmix_alpha : cfg.mixup_alpha;
  const float g1 = mix_gamma(g, a), g2 = mix_gamma(g, a);
  const float s = g1 + g2;
  float lam = s > 0.f ? g1 / s : 0.5f;
  lam = lam < 0.f ? 0.f : (lam > 1.f ? 1.f : lam);
  p.lam_raw = lam;
  if (!cut) {
    p.mode = kMixMixup;
    p.lam = lam;
    return p;
  }
  // the published rand_bbox rule, the cut sizes in fp64 so that int() sees the exact product
  p.mode = kMixCutmix;
  const double r = sqrt(1.0 - (double)lam);
  const int cut_h = (int)((double)H * r), cut_w = (int)((double)W * r);
  const int cy = mix_clampi((int)(g.uniform() * (float)H), 0, H - 1);
  const int cx = mix_clampi((int)(g.uniform() * (float)W), 0, W - 1);
  p.y0 = mix_clampi(cy - cut_h / 2, 0, H);
  p.y1 = mix_clampi(cy + cut_h / 2, 0, H);
  p.x0 = mix_clampi(cx - cut_w / 2, 0, W);
  p.x1 = mix_clampi(cx + cut_w / 2, 0, W);
  p.lam = (float)(1.0 - (double)((long long)(p.y1 - p.y0) * (p.x1 - p.x0)) / ((double)H * (double)W));
  return p;
}

__host__ __device__ __forceinline__ void mix_publish(float* __restrict__ row, const MixParams& p) {
  row[0] = (float)p.mode;
  row[1] = p.lam;
  row[2] = p.lam_raw;
  row[3] = (float)p.y0;
  row[4] = (float)p.y1;
  row[5] = (float)p.x0;
  row[6] = (float)p.x1;
  row[7] = 0.f;
}

}  // namespace cdp
