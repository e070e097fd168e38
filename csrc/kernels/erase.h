// RandomErasing (Zhong et al.) boxes and fill noise, drawn on the device.
//
// One box per image: {on, top, left, h, w} is a pure function of (seed, step counter, image slot b, cfg,
// H, W) with H x W the *output* size of the augment launch (the box lives in output pixels, after crop,
// resize and flip, on the normalised tensor: where torchvision and timm erase). The rule is
// torchvision's published RandomErasing.get_params: with probability prob the image is erased; then at
// most kEraseTries proposals of an area share U(scale) and an aspect ratio h / w log-uniform in ratio
// (RandomResizedCrop's aspect is w / h), accepted when h < H and w < W -- strict, as torchvision has
// them -- and placed uniformly. After kEraseTries rejections the image is not erased. One condition is
// our own: a proposal also needs h >= 1 and w >= 1. torchvision accepts a box that rounds to zero rows
// or columns and then erases nothing; here such a proposal is rejected and the next one is drawn, so a
// published row with on = 1 always names a box that holds pixels.
//
// The augment kernels evaluate erase_draw from those inputs, so erasing needs no launch of its own and
// no host-side draw: a replayed hipGraph sees new boxes every step. erase_params_kernel (misc.hip)
// evaluates the same function for a schedule of counters, erase_noise_kernel the fill noise of one.
//
// Random source: the counter-based hash of mix.h, keyed by (seed, counter, b) and a stream tag of its
// own (a second tag for the fill noise), so crops, flips, RandomResizedCrop windows and mix draws are
// the same bits with erasing on or off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mix.h"
#include "rrc.h"

namespace cdp {

constexpr int kEraseConst = 0;  // value[c], in normalised units
constexpr int kEraseRand = 1;   // one N(0, 1) value per channel per image: erase_noise at pixel (0, 0)
constexpr int kErasePixel = 2;  // one N(0, 1) value per element

struct EraseCfg {
  float prob = 0.f;                                             // probability that an image is erased; 0: off
  float scale_lo = 0.02f, scale_hi = 0.33f;                     // the box's share of the output area
  float log_ratio_lo = -1.2039728f, log_ratio_hi = 1.1939225f;  // log of the aspect ratio h / w: ln 0.3, ln 3.3
  int mode = kEraseConst;
  float value[3] = {0.f, 0.f, 0.f};
};
inline bool erase_enabled(const EraseCfg& c) { return c.prob > 0.f; }

struct EraseBox {
  int on, top, left, h, w;
};

constexpr int kEraseTries = 10;  // proposals before the image is left alone: no kernel can spin here
constexpr int kEraseRow = 5;     // ints of a published row: {on, top, left, h, w}, all 0 when on = 0

// Draw 0 is u_p; proposal i takes draws 1 + 4 i .. 4 + 4 i (area, aspect, top, left), used or not. sqrt,
// exp and the rounding are in fp64, to nearest, ties to even, as rrc_draw's.
__host__ __device__ inline EraseBox erase_draw(unsigned long long seed, unsigned long long ctr, int b,
                                               const EraseCfg& cfg, int H, int W) {
  MixRng g{mix_hash(mix_hash(seed ^ 0x65726173652D626Full) ^
                    mix_hash(mix_hash(ctr + 0x782D65726173652Dull) + (unsigned long long)b)),
           0u};
  const float u_p = g.uniform();
  if (!(u_p < cfg.prob)) return EraseBox{0, 0, 0, 0, 0};
  const double area = (double)H * (double)W;
#pragma unroll 1
  for (int i = 0; i < kEraseTries; ++i) {
    const float u_s = g.uniform(), u_r = g.uniform(), u_t = g.uniform(), u_l = g.uniform();
    const double target = area * ((double)cfg.scale_lo + ((double)cfg.scale_hi - (double)cfg.scale_lo) * (double)u_s);
    const double aspect =
        exp((double)cfg.log_ratio_lo + ((double)cfg.log_ratio_hi - (double)cfg.log_ratio_lo) * (double)u_r);
    const double hd = rint(sqrt(target * aspect)), wd = rint(sqrt(target / aspect));
    if (hd >= 1.0 && hd < (double)H && wd >= 1.0 && wd < (double)W) {
      const int h = (int)hd, w = (int)wd;
      return EraseBox{1, rrc_offset(u_t, H - h), rrc_offset(u_l, W - w), h, w};
    }
  }
  return EraseBox{0, 0, 0, 0, 0};
}

// The fill noise of image slot b: element e = (y OW + x) 3 + c is Box-Muller of the two uniforms
// hash(key + 2 e) and hash(key + 2 e + 1), the index in 64 bits (2 e passes 2^32 at large outputs, so
// this does not go through MixRng's 32-bit draw index). Only products and library calls: nothing is
// left to contract, so every caller on the device gets the same bits.
__host__ __device__ __forceinline__ unsigned long long erase_noise_key(unsigned long long seed, unsigned long long ctr,
                                                                       int b) {
  return mix_hash(mix_hash(seed ^ 0x65726173652D6E7Aull) ^
                  mix_hash(mix_hash(ctr + 0x6E6F6973652D3031ull) + (unsigned long long)b));
}
__host__ __device__ __forceinline__ float erase_uniform(unsigned long long r) {  // MixRng::uniform's map
  return ((float)(unsigned)(r >> 41) + 0.5f) * (1.f / 8388608.f);
}
__host__ __device__ __forceinline__ float erase_noise_at(unsigned long long key, long long e) {
  const float u1 = erase_uniform(mix_hash(key + 2ull * (unsigned long long)e));
  const float u2 = erase_uniform(mix_hash(key + 2ull * (unsigned long long)e + 1ull));
  return sqrtf(-2.f * logf(u1)) * cosf(6.2831853f * u2);
}
__host__ __device__ __forceinline__ float erase_noise(unsigned long long seed, unsigned long long ctr, int b,
                                                      long long e) {
  return erase_noise_at(erase_noise_key(seed, ctr, b), e);
}

// An image's box with what its fill needs: the noise key and, under const and rand, the three values.
struct EraseImg {
  EraseBox bx;
  unsigned long long key;
  float fill[3];
};
__host__ __device__ __forceinline__ EraseImg erase_image(unsigned long long seed, unsigned long long ctr, int b,
                                                         const EraseCfg& cfg, int H, int W) {
  EraseImg e;
  e.bx = erase_draw(seed, ctr, b, cfg, H, W);
  e.key = erase_noise_key(seed, ctr, b);
  for (int c = 0; c < 3; ++c) e.fill[c] = cfg.mode == kEraseRand ? erase_noise_at(e.key, c) : cfg.value[c];
  return e;
}
__host__ __device__ __forceinline__ bool erase_in(const EraseBox& bx, int y, int x) {
  return bx.on && (unsigned)(y - bx.top) < (unsigned)bx.h && (unsigned)(x - bx.left) < (unsigned)bx.w;
}
// channel c of erased output pixel number pix = y OW + x
__host__ __device__ __forceinline__ float erase_fill(const EraseImg& e, int mode, long long pix, int c) {
  return mode == kErasePixel ? erase_noise_at(e.key, pix * 3 + c) : e.fill[c];
}
__host__ __device__ __forceinline__ void erase_publish(int* __restrict__ row, const EraseBox& bx) {
  row[0] = bx.on;
  row[1] = bx.top;
  row[2] = bx.left;
  row[3] = bx.h;
  row[4] = bx.w;
}

}  // namespace cdp
