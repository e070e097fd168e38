// RandAugment (Cubuk et al.) draws, rows and parameter derivation.
//
// Every image gets num_ops operations. Operation k of image slot b is a pure function of (seed, step
// counter, b, k, cfg, H, W) with H x W the size of the staged uint8 image (after crop, resize and flip):
// an op drawn uniformly from cfg.names, a sign bit, and a level L = clamp(magnitude + mstd n, 0, 30),
// n ~ N(0, 1). It is published as one row of kRaRow ints
//   {op | sign << 8, level_q, p0 .. p5}     level_q = round(256 L)
// and everything a pixel depends on is an integer of that row: randaug_kernel (randaug.hip) and the
// Python twin (randaug.py) apply a row with integer arithmetic only and agree bitwise.
//
// From level_q the parameters are integer arithmetic too (round is to nearest, halves up; t = L / 30):
//   ShearX / ShearY        b resp. c = +-round(65536 * 0.3 t)  = +-round(256 level_q / 100)
//   TranslateX / Y         n = trunc(150 / 331 * W t) pixels   = 150 W level_q / (331 * 7680); tx = -+131072 n
//   Brightness .. Sharpness f8 = 256 +- round(256 * 0.9 t)      = 256 +- round(3 level_q / 100)
//   Posterize              bits = 8 - round(4 t)               = 8 - round(level_q / 1920); mask in p0, bits in p1
//   Solarize               thr = 256 - round(256 t)            = 256 - round(level_q / 30)
// Only Rotate needs floating point: theta = level_q / 7680 * pi / 6, a = d = rint(65536 cosf(theta)),
// b = -c = +-rint(65536 sinf(theta)). The level itself is Box-Muller in fp32 (MixRng's map).
//
// Random source: the counter-based hash of mix.h, keyed by (seed, counter, b) under a stream tag of its
// own and walked by the draw index 4 k + {0: op, 1: sign, 2 and 3: the level's two uniforms}. Crops,
// flips, RandomResizedCrop windows, mixes, erase boxes and noise are the same bits with RandAugment on
// or off. Op index and sign are integer arithmetic on the hash: ((r >> 32) * n_names) >> 32 and r >> 63.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mix.h"
#include "rrc.h"

namespace cdp {

constexpr int kRaIdentity = 0, kRaShearX = 1, kRaShearY = 2, kRaTranslateX = 3, kRaTranslateY = 4, kRaRotate = 5,
              kRaBrightness = 6, kRaColor = 7, kRaContrast = 8, kRaSharpness = 9, kRaPosterize = 10,
              kRaSolarize = 11, kRaAutoContrast = 12, kRaEqualize = 13, kRaNumKinds = 14;
constexpr int kRaRow = 8;        // ints of a published row
constexpr int kRaMaxOps = 8;     // operations per image
constexpr int kRaMaxNames = 32;  // entries of the list the ops are drawn from
constexpr int kRaNegBit = 256;   // set in row[0] when the sign bit was drawn negative

struct RandAugCfg {
  int num_ops = 0;  // operations per image; 0: off
  float magnitude = 9.f, mstd = 0.f;
  int n_names = 0;
  unsigned char names[kRaMaxNames] = {};  // op kinds, drawn from uniformly with replacement
  int fill[3] = {128, 128, 128};          // the geometric ops' value outside the image
};
inline bool randaug_cfg_ok(const RandAugCfg& c) {
  bool ok = c.num_ops >= 1 && c.num_ops <= kRaMaxOps && c.magnitude >= 0.f && c.magnitude <= 30.f && c.mstd >= 0.f &&
            c.mstd < INFINITY && c.n_names >= 1 && c.n_names <= kRaMaxNames;
  for (int i = 0; ok && i < c.n_names; ++i) ok = c.names[i] < kRaNumKinds;
  for (int i = 0; ok && i < 3; ++i) ok = c.fill[i] >= 0 && c.fill[i] <= 255;
  return ok;
}

struct RaRow {
  int v[kRaRow];
};

// round(num / den) to nearest, halves up, for num >= 0 and den > 0
__host__ __device__ __forceinline__ long long ra_round_div(long long num, long long den) {
  return (2 * num + den) / (2 * den);
}

// The row of op kind `op` with sign `neg` at level_q on an H x W image.
__host__ __device__ inline RaRow ra_derive(int op, int neg, int lq, int H, int W) {
  RaRow r;
  r.v[0] = op | (neg ? kRaNegBit : 0);
  r.v[1] = lq;
  for (int i = 2; i < kRaRow; ++i) r.v[i] = 0;
  const int sg = neg ? -1 : 1;
  if (op >= kRaShearX && op <= kRaRotate) {
    int a = 65536, b = 0, c = 0, d = 65536, tx = 0, ty = 0;
    if (op == kRaShearX) b = sg * (int)ra_round_div(256ll * lq, 100);
    if (op == kRaShearY) c = sg * (int)ra_round_div(256ll * lq, 100);
    if (op == kRaTranslateX) tx = -sg * 131072 * (int)(150ll * W * lq / (331ll * 7680ll));
    if (op == kRaTranslateY) ty = -sg * 131072 * (int)(150ll * H * lq / (331ll * 7680ll));
    if (op == kRaRotate) {
      const float th = (float)lq * (0.52359877559829887f / 7680.f);
      a = d = (int)rintf(65536.f * cosf(th));
      b = sg * (int)rintf(65536.f * sinf(th));
      c = -b;
    }
    r.v[2] = a;
    r.v[3] = b;
    r.v[4] = c;
    r.v[5] = d;
    r.v[6] = tx;
    r.v[7] = ty;
  } else if (op >= kRaBrightness && op <= kRaSharpness) {
    r.v[2] = 256 + sg * (int)ra_round_div(3ll * lq, 100);
  } else if (op == kRaPosterize) {
    const int bits = 8 - (int)ra_round_div(lq, 1920);
    r.v[2] = (0xFF << (8 - bits)) & 0xFF;
    r.v[3] = bits;
  } else if (op == kRaSolarize) {
    r.v[2] = 256 - (int)ra_round_div(lq, 30);
  }
  return r;
}

__host__ __device__ __forceinline__ unsigned long long ra_key(unsigned long long seed, unsigned long long ctr, int b) {
  return mix_hash(mix_hash(seed ^ 0x72616E646175672Dull) ^
                  mix_hash(mix_hash(ctr + 0x6F70732D72612D31ull) + (unsigned long long)b));
}
__host__ __device__ __forceinline__ float ra_uniform(unsigned long long r) {  // MixRng::uniform's map
  return ((float)(unsigned)(r >> 41) + 0.5f) * (1.f / 8388608.f);
}

// Operation k of image slot b at step counter ctr.
__host__ __device__ inline RaRow ra_draw(unsigned long long seed, unsigned long long ctr, int b, int k,
                                         const RandAugCfg& cfg, int H, int W) {
  const unsigned long long base = ra_key(seed, ctr, b) + 4ull * (unsigned long long)k;
  const unsigned long long r0 = mix_hash(base), r1 = mix_hash(base + 1ull);
  const int op = cfg.names[(int)(((r0 >> 32) * (unsigned long long)cfg.n_names) >> 32)];
  const int neg = (int)(r1 >> 63);
  float L = cfg.magnitude;
  if (cfg.mstd > 0.f) {
    const float u1 = ra_uniform(mix_hash(base + 2ull)), u2 = ra_uniform(mix_hash(base + 3ull));
    L = cfg.magnitude + cfg.mstd * (sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2));
  }
  L = L < 0.f ? 0.f : (L > 30.f ? 30.f : L);
  return ra_derive(op, neg, (int)rintf(256.f * L), H, W);
}

// The staging of randaug_launch: where the uint8 images come from and how they are cropped. resize = 0: the
// pad-shift crop and the flip of the augment launch (H x W output). resize = 1: the RandomResizedCrop window
// of rrc_draw resampled to OH x OW, then the flip; crops[b][kCropRow] receives {top, left, h, w, flip}.
struct RaStage {
  const unsigned char* imgs;
  const long long* idx;
  long long idx_off;
  int B, H, W, OH, OW;
  int resize;
  RrcCfg rc;
  int pad, flip;
  const long long* counter;
  unsigned long long seed;
  long long nbatches;
  const long long* labels;
  long long* labels_out;
  int* crops;
};

// One launch, one workgroup per image: stage image b as uint8 [OH, OW, 3] into buf_a[b], then apply its
// cfg.num_ops operations ping-pong between buf_a[b] and buf_b[b]; the result is in buf_a when num_ops is even
// and in buf_b when it is odd. rows[b][k][kRaRow] receives the rows. Asynchronous, allocates nothing.
void randaug_launch(const RaStage& s, const RandAugCfg& cfg, unsigned char* buf_a, unsigned char* buf_b, int* rows,
                    hipStream_t st);
// rows[i][b][k][kRaRow] = ra_draw at step counter first + i, i < n, for an H x W staged image
void randaug_params_launch(unsigned long long seed, long long first, long long n, int B, const RandAugCfg& cfg, int H,
                           int W, int* rows, hipStream_t st);

}  // namespace cdp
