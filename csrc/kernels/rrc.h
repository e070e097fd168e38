// RandomResizedCrop windows, drawn on the device.
//
// One window per image: {top, left, h, w} is a pure function of (seed, step counter, image slot b, cfg,
// H, W), by torchvision's published RandomResizedCrop.get_params rule. The resize kernel evaluates
// rrc_draw in one lane per workgroup from those inputs, so the crop needs no launch of its own and no
// host-side draw: a replayed hipGraph sees new windows every step. rrc_params_kernel (misc.hip)
// evaluates the same function for a schedule of counters.
//
// Random source: the counter-based hash of mix.h, keyed by (seed, counter, b) and a stream tag of its
// own. The flip bit stays the one of the augmentation's own hash (aug_image, misc.hip) and the mix
// draws stay mix_draw's, so both are the same bits with the resize on or off, and the windows are the
// same bits with mixing on or off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mix.h"

namespace cdp {

struct RrcCfg {
  float scale_lo, scale_hi;          // the window's share of the image area, U(scale_lo, scale_hi)
  float log_ratio_lo, log_ratio_hi;  // log of the aspect ratio w / h, U(log_ratio_lo, log_ratio_hi)
};
struct RrcWindow {
  int top, left, h, w;
};

constexpr int kRrcTries = 10;  // proposals before the central fallback: no kernel can spin here
constexpr int kCropRow = 5;    // ints of a published row: {top, left, h, w, flip}

// uniform on the integers [0, span]
__host__ __device__ __forceinline__ int rrc_offset(float u, int span) {
  const int v = (int)(u * (float)(span + 1));
  return v > span ? span : v;
}

// Every proposal takes four draws (area, aspect, top, left), used or not, so proposal i reads draws
// 4 i .. 4 i + 3. sqrt, exp and the rounding are in fp64 so that the rounding sees the exact product;
// rounding is to nearest, ties to even, as Python's round().
__host__ __device__ inline RrcWindow rrc_draw(unsigned long long seed, unsigned long long ctr, int b,
                                              const RrcCfg& cfg, int H, int W) {
  MixRng g{mix_hash(mix_hash(seed ^ 0x7272632D73747265ull) ^
                    mix_hash(mix_hash(ctr + 0x632D7272632D3031ull) + (unsigned long long)b)),
           0u};
  const double area = (double)H * (double)W;
#pragma unroll 1
  for (int i = 0; i < kRrcTries; ++i) {
    const float u_s = g.uniform(), u_r = g.uniform(), u_t = g.uniform(), u_l = g.uniform();
    const double target = area * ((double)cfg.scale_lo + ((double)cfg.scale_hi - (double)cfg.scale_lo) * (double)u_s);
    const double aspect =
        exp((double)cfg.log_ratio_lo + ((double)cfg.log_ratio_hi - (double)cfg.log_ratio_lo) * (double)u_r);
    const double wd = rint(sqrt(target * aspect)), hd = rint(sqrt(target / aspect));
    if (wd > 0.0 && wd <= (double)W && hd > 0.0 && hd <= (double)H) {
      const int w = (int)wd, h = (int)hd;
      return RrcWindow{rrc_offset(u_t, H - h), rrc_offset(u_l, W - w), h, w};
    }
  }
  // central fallback: the whole image, cut to the nearest allowed aspect ratio
  const double in_ratio = (double)W / (double)H;
  const double ratio_lo = exp((double)cfg.log_ratio_lo), ratio_hi = exp((double)cfg.log_ratio_hi);
  int w = W, h = H;
  if (in_ratio < ratio_lo) h = (int)rint((double)W / ratio_lo);
  else if (in_ratio > ratio_hi) w = (int)rint((double)H * ratio_hi);
  h = mix_clampi(h, 1, H);
  w = mix_clampi(w, 1, W);
  return RrcWindow{(H - h) / 2, (W - w) / 2, h, w};
}

}  // namespace cdp
