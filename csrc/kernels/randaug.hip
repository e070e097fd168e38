// RandAugment in the device loader: one launch before the normalising augment launch (randaug.h).
//
// randaug_kernel runs one workgroup of up to 1024 threads per image, so every operation is uniform over the
// workgroup and the whole-image statistics (min / max, the gray mean, 3 x 256 histograms) are LDS
// reductions with LDS integer atomics. The workgroup
//   1. stages its image as uint8 [OH, OW, 3]: the gather through idx / idx_off / nbatches / counter of the
//      augment kernels, then either their pad-shift crop and flip (the same hash bits, padding 0), or the
//      RandomResizedCrop window of rrc_draw resampled with augment_resize_kernel's integer taps. There the
//      bilinear value is exact in integers: the tap weights are the rationals num / den the taps already
//      form, the value is (sum w_y w_x p + D / 2) / D with D = den_y den_x -- re-quantised to uint8, the PIL
//      order (augment_resize_kernel itself blends in fp32 and does not re-quantise);
//   2. applies the image's operations in order: reduce if the op needs statistics, barrier, apply from one
//      buffer into the other, barrier, swap.
// The two buffers are global memory that this workgroup writes and reads again inside the launch: they are
// plain pointers (no const, no __restrict__, no read-only loads), ordered by the workgroup barrier alone,
// and every barrier sits in workgroup-uniform control flow (the op of a row, never a pixel, decides).
// All pixel arithmetic is integer arithmetic on the published row.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "randaug.h"

namespace cdp {

namespace {

constexpr int kRaThreads = 1024;

// floor(num / den) for 0 <= num < 2^52 and 0 < den < 2^32 with a quotient below 2^20: the fp64 quotient is
// off by less than one, and the remainder says which way
__device__ __forceinline__ unsigned ra_div_u(unsigned long long num, unsigned long long den) {
  long long q = (long long)((double)num / (double)den);
  const long long r = (long long)num - q * (long long)den;
  if (r < 0) --q;
  else if (r >= (long long)den) ++q;
  return (unsigned)q;
}

struct RaTap {
  int i0, i1;
  unsigned w1, den;  // weight of i1 is w1 / den, of i0 (den - w1) / den
};
// rsz_tap's neighbours (misc.hip) with the weight kept as the rational it is
__device__ __forceinline__ RaTap ra_tap(int o, int n_in, int n_out) {
  const int n = (2 * o + 1) * n_in - n_out;  // < 2^31 for sizes < 32768
  const unsigned num = (unsigned)(n > 0 ? n : 0);
  const unsigned den = 2u * (unsigned)n_out;
  const unsigned i0 = num / den;
  RaTap t;
  t.i0 = min((int)i0, n_in - 1);
  t.i1 = min((int)i0 + 1, n_in - 1);
  t.w1 = num - i0 * den;
  t.den = den;
  return t;
}

__device__ __forceinline__ int ra_gray(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }
__device__ __forceinline__ int ra_blend(int f8, int v, int d) {
  const int o = (f8 * v + (256 - f8) * d + 128) >> 8;  // arithmetic shift: a floor
  return o < 0 ? 0 : (o > 255 ? 255 : o);
}

__global__ __launch_bounds__(kRaThreads) void randaug_kernel(RaStage s, RandAugCfg cfg, unsigned char* buf_a,
                                                            unsigned char* buf_b, int* __restrict__ rows) {
  __shared__ RaRow s_rows[kRaMaxOps];
  __shared__ int s_win[5];
  __shared__ unsigned s_hist[3 * 256];
  __shared__ int s_lut[3 * 256];
  __shared__ unsigned long long s_sum;
  __shared__ int s_lo[3], s_hi[3], s_mean;
  const int b = blockIdx.x;
  if (b >= s.B) return;  // (uniform over the workgroup)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int OH = s.OH, OW = s.OW, npix = OH * OW;
  const unsigned long long ctr = s.counter ? (unsigned long long)s.counter[0] : 0ull;
  const long long off =
      s.nbatches > 0 ? s.idx_off + (long long)(ctr % (unsigned long long)s.nbatches) * s.B : s.idx_off;
  const long long src_i = s.idx ? s.idx[off + b] : (off + b);
  // the crop / flip hash of the augment kernels (aug_image, misc.hip): the same bits
  const unsigned long long hr = mix_hash(s.seed ^ mix_hash(ctr * 0x100000001B3ull + (unsigned long long)b));
  const int fl = s.flip && ((hr >> 40) & 1) ? 1 : 0;
  if (tid == 0) {
    RrcWindow w{0, 0, s.H, s.W};
    if (s.resize) w = rrc_draw(s.seed, ctr, b, s.rc, s.H, s.W);
    s_win[0] = w.top;
    s_win[1] = w.left;
    s_win[2] = w.h;
    s_win[3] = w.w;
    s_win[4] = fl;
    if (s.labels_out) s.labels_out[b] = s.labels[src_i];
    if (s.resize && s.crops) {
      int* row = s.crops + (long long)b * kCropRow;
      row[0] = w.top;
      row[1] = w.left;
      row[2] = w.h;
      row[3] = w.w;
      row[4] = fl;
    }
    for (int k = 0; k < cfg.num_ops; ++k) {
      const RaRow r = ra_draw(s.seed, ctr, b, k, cfg, OH, OW);
      s_rows[k] = r;
      int* o = rows + ((long long)b * cfg.num_ops + k) * kRaRow;
      for (int j = 0; j < kRaRow; ++j) o[j] = r.v[j];
    }
  }
  __syncthreads();
  const long long base = (long long)b * npix * 3;
  unsigned char* src = buf_a + base;
  unsigned char* dst = buf_b + base;
  const unsigned char* img = s.imgs + src_i * (long long)s.H * s.W * 3;
  // ---- 1. stage
  if (!s.resize) {
    const int span = 2 * s.pad + 1;
    const int oy = s.pad ? (int)(hr % span) - s.pad : 0;
    const int ox = s.pad ? (int)((hr >> 16) % span) - s.pad : 0;
    for (int px = tid; px < npix; px += nt) {
      const int h = px / OW, w = px - h * OW;
      const int ww = fl ? (OW - 1 - w) : w;  // flip after the crop
      const int sh = h + oy, sw = ww + ox;
      const bool in = (unsigned)sh < (unsigned)s.H && (unsigned)sw < (unsigned)s.W;
      const unsigned char* sp = img + (long long)(in ? sh * s.W + sw : 0) * 3;
      for (int c = 0; c < 3; ++c) src[(long long)px * 3 + c] = in ? sp[c] : (unsigned char)0;
    }
  } else {
    const int top = s_win[0], left = s_win[1], wh = s_win[2], ww = s_win[3];
    const unsigned char* win = img + ((long long)top * s.W + left) * 3;
    for (int px = tid; px < npix; px += nt) {
      const int y = px / OW, x = px - y * OW;
      const RaTap ty = ra_tap(y, wh, OH);
      const RaTap tx = ra_tap(fl ? OW - 1 - x : x, ww, OW);  // flip after the resize
      const unsigned char* r0 = win + (long long)ty.i0 * s.W * 3;
      const unsigned char* r1 = win + (long long)ty.i1 * s.W * 3;
      const unsigned long long wy1 = ty.w1, wy0 = ty.den - ty.w1, wx1 = tx.w1, wx0 = tx.den - tx.w1;
      const unsigned long long D = (unsigned long long)ty.den * tx.den;  // < 2^32
      for (int c = 0; c < 3; ++c) {
        const unsigned long long t0 = wx0 * r0[tx.i0 * 3 + c] + wx1 * r0[tx.i1 * 3 + c];
        const unsigned long long t1 = wx0 * r1[tx.i0 * 3 + c] + wx1 * r1[tx.i1 * 3 + c];
        src[(long long)px * 3 + c] = (unsigned char)ra_div_u(wy0 * t0 + wy1 * t1 + D / 2, D);
      }
    }
  }
  __syncthreads();
  // ---- 2. the operations
  for (int k = 0; k < cfg.num_ops; ++k) {
    const RaRow row = s_rows[k];
    const int op = row.v[0] & 255;
    const bool stats = op == kRaContrast || op == kRaAutoContrast || op == kRaEqualize;
    if (stats) {
      for (int i = tid; i < 3 * 256; i += nt) s_hist[i] = 0u;
      if (tid == 0) s_sum = 0ull;
      if (tid < 3) {
        s_lo[tid] = 255;
        s_hi[tid] = 0;
      }
      __syncthreads();
      if (op == kRaContrast) {
        unsigned long long acc = 0ull;
        for (int px = tid; px < npix; px += nt) {
          const unsigned char* p = src + (long long)px * 3;
          acc += (unsigned long long)ra_gray(p[0], p[1], p[2]);
        }
        atomicAdd(&s_sum, acc);
      } else if (op == kRaAutoContrast) {
        int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
        for (int px = tid; px < npix; px += nt) {
          const unsigned char* p = src + (long long)px * 3;
          for (int c = 0; c < 3; ++c) {
            lo[c] = min(lo[c], (int)p[c]);
            hi[c] = max(hi[c], (int)p[c]);
          }
        }
        for (int c = 0; c < 3; ++c) {
          atomicMin(&s_lo[c], lo[c]);
          atomicMax(&s_hi[c], hi[c]);
        }
      } else {
        for (int px = tid; px < npix; px += nt) {
          const unsigned char* p = src + (long long)px * 3;
          for (int c = 0; c < 3; ++c) atomicAdd(&s_hist[c * 256 + p[c]], 1u);
        }
      }
      __syncthreads();
      if (op == kRaContrast && tid == 0) {
        s_mean = (int)((s_sum + (unsigned long long)(npix / 2)) / (unsigned long long)npix);
      }
      if (op == kRaEqualize && tid < 3) {
        // torchvision's integer rule, one channel per thread
        const unsigned* h = s_hist + tid * 256;
        int* lut = s_lut + tid * 256;
        int last = 0;
        for (int i = 0; i < 256; ++i)
          if (h[i]) last = i;
        const unsigned step = ((unsigned)npix - h[last]) / 255u;
        unsigned cum = 0u;
        for (int i = 0; i < 256; ++i) {
          const unsigned v = step ? (cum + step / 2u) / step : (unsigned)i;
          lut[i] = step && i == 0 ? 0 : (int)(v > 255u ? 255u : v);
          cum += h[i];
        }
      }
      __syncthreads();
    }
    if (op >= kRaShearX && op <= kRaRotate) {
      const long long a = row.v[2], bb = row.v[3], c_ = row.v[4], d = row.v[5], tx = row.v[6], ty = row.v[7];
      for (int px = tid; px < npix; px += nt) {
        const int y = px / OW, x = px - y * OW;
        const long long u = 2 * x + 1 - OW, v = 2 * y + 1 - OH;
        const long long sx = (a * u + bb * v + tx + 65536ll * OW) >> 17;
        const long long sy = (c_ * u + d * v + ty + 65536ll * OH) >> 17;
        const bool in = sx >= 0 && sx < OW && sy >= 0 && sy < OH;
        const unsigned char* p = src + (in ? (sy * OW + sx) : 0ll) * 3;
        for (int c = 0; c < 3; ++c) dst[(long long)px * 3 + c] = in ? p[c] : (unsigned char)cfg.fill[c];
      }
    } else if (op == kRaBrightness || op == kRaColor || op == kRaContrast) {
      const int f8 = row.v[2];
      const int mean = op == kRaContrast ? s_mean : 0;
      for (int px = tid; px < npix; px += nt) {
        const unsigned char* p = src + (long long)px * 3;
        const int r = p[0], g = p[1], bl = p[2];
        const int dd = op == kRaColor ? ra_gray(r, g, bl) : mean;
        unsigned char* o = dst + (long long)px * 3;
        o[0] = (unsigned char)ra_blend(f8, r, dd);
        o[1] = (unsigned char)ra_blend(f8, g, dd);
        o[2] = (unsigned char)ra_blend(f8, bl, dd);
      }
    } else if (op == kRaSharpness) {
      const int f8 = row.v[2];
      for (int px = tid; px < npix; px += nt) {
        const int y = px / OW, x = px - y * OW;
        const unsigned char* p = src + (long long)px * 3;
        unsigned char* o = dst + (long long)px * 3;
        const bool inner = y > 0 && y < OH - 1 && x > 0 && x < OW - 1;
        for (int c = 0; c < 3; ++c) {
          const int v = p[c];
          int out = v;  // border pixels keep their value
          if (inner) {
            int sum = 4 * v;  // the centre weighs 5
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx) sum += p[(dy * OW + dx) * 3 + c];
            out = ra_blend(f8, v, (sum + 6) / 13);
          }
          o[c] = (unsigned char)out;
        }
      }
    } else if (op == kRaAutoContrast) {
      for (int px = tid; px < npix; px += nt) {
        const unsigned char* p = src + (long long)px * 3;
        unsigned char* o = dst + (long long)px * 3;
        for (int c = 0; c < 3; ++c) {
          const int lo = s_lo[c], span = s_hi[c] - s_lo[c];
          const int v = p[c];
          o[c] = (unsigned char)(span > 0 ? ((v - lo) * 255 + span / 2) / span : v);
        }
      }
    } else if (op == kRaEqualize) {
      for (int px = tid; px < npix; px += nt) {
        const unsigned char* p = src + (long long)px * 3;
        unsigned char* o = dst + (long long)px * 3;
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)s_lut[c * 256 + p[c]];
      }
    } else {  // Identity, Posterize, Solarize: per element
      const int mask = op == kRaPosterize ? row.v[2] : 0xFF;
      const int thr = op == kRaSolarize ? row.v[2] : 256;
      for (int px = tid; px < npix; px += nt) {
        for (int c = 0; c < 3; ++c) {
          const int v = src[(long long)px * 3 + c] & mask;
          dst[(long long)px * 3 + c] = (unsigned char)(v >= thr ? 255 - v : v);
        }
      }
    }
    __syncthreads();  // dst is complete (and the statistics are free) before the next op reads it
    unsigned char* t = src;
    src = dst;
    dst = t;
  }
}

__global__ __launch_bounds__(256) void randaug_params_kernel(unsigned long long seed, long long first, long long total,
                                                            int B, RandAugCfg cfg, int H, int W,
                                                            int* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long img = i / cfg.num_ops;
  const RaRow r = ra_draw(seed, (unsigned long long)(first + img / B), (int)(img % B), (int)(i % cfg.num_ops), cfg, H, W);
  for (int j = 0; j < kRaRow; ++j) rows[i * kRaRow + j] = r.v[j];
}

}  // namespace

void randaug_launch(const RaStage& s, const RandAugCfg& cfg, unsigned char* buf_a, unsigned char* buf_b, int* rows,
                    hipStream_t st) {
  if (s.B < 1 || s.B > 65535 || s.H < 1 || s.W < 1 || s.H > 0x7fff || s.W > 0x7fff || s.OH < 1 || s.OW < 1 ||
      s.OH > 0x7fff || s.OW > 0x7fff)
    throw std::runtime_error("randaug: 1 <= batch < 65536 and 1 <= H, W, out_h, out_w < 32768");
  if (!randaug_cfg_ok(cfg))
    throw std::runtime_error("randaug: 1 <= num_ops <= 8, 0 <= magnitude <= 30, mstd >= 0, 1 .. 32 known ops and a "
                             "fill in 0 .. 255 required");
  if (!s.imgs || !buf_a || !buf_b || !rows || (s.labels_out && !s.labels) || (s.nbatches > 0 && !s.counter) ||
      s.nbatches < 0 || s.idx_off < 0)
    throw std::runtime_error("randaug: images, both buffers and rows needed (labels for labels_out, the counter for "
                             "counter-driven offsets)");
  if (s.resize) {
    if (!s.crops || !(s.rc.scale_lo > 0.f && s.rc.scale_lo <= s.rc.scale_hi && s.rc.scale_hi <= 1.f &&
                      s.rc.log_ratio_lo <= s.rc.log_ratio_hi))
      throw std::runtime_error("randaug: the resize needs crops and 0 < scale_lo <= scale_hi <= 1, ratio_lo <= ratio_hi");
  } else if (s.OH != s.H || s.OW != s.W || s.pad < 0 || s.pad > 0x7fff) {
    throw std::runtime_error("randaug: without the resize the output is H x W and 0 <= pad < 32768");
  }
  const int npix = s.OH * s.OW;
  const int threads = npix >= kRaThreads ? kRaThreads : ((npix + 63) / 64) * 64;
  hipLaunchKernelGGL(randaug_kernel, dim3((unsigned)s.B), dim3((unsigned)threads), 0, st, s, cfg, buf_a, buf_b, rows);
}

void randaug_params_launch(unsigned long long seed, long long first, long long n, int B, const RandAugCfg& cfg, int H,
                           int W, int* rows, hipStream_t st) {
  if (!randaug_cfg_ok(cfg) || n < 0 || B < 0 || B > 65535 || H < 1 || W < 1 || H > 0x7fff || W > 0x7fff)
    throw std::runtime_error("randaug_params: n >= 0, 0 <= B < 65536, 1 <= H, W < 32768 and a valid configuration");
  const long long total = n * B * cfg.num_ops;
  if (total == 0) return;
  hipLaunchKernelGGL(randaug_params_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, seed, first,
                     total, B, cfg, H, W, rows);
}

}  // namespace cdp
