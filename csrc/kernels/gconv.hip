// Direct grouped 3x3 convolution (pad 1, stride 1 or 2) in plain fp32 FMA: forward, data gradient and
// weight gradient of ResNeXt's Bottleneck conv2. NHWC activations, weight [Co][3][3][Cg_in] (channels_last
// [Co, Cg_in, 3, 3]); Cg_in and Cg_out multiples of 4, <= 64.
//
// Why direct and not the implicit GEMM: per group the product is pixels x 9 Cg x Cg, so at Cg = 4 a 32 x 32
// MFMA tile would be 7/8 padding, and the layer is bound by reading x and writing y once. Operands and
// accumulation are exact fp32 (one FMA chain of length 9 Cg_in per output, in a fixed order), so the kernels
// do not depend on the conv engine and two calls give the same bits. No atomics, no host synchronisation.
//
// How the work is split (all three kernels, 256 threads): the channel axis is cut into blocks of 64 / CGB
// whole groups, CGB = max(Cg_in, Cg_out) rounded up to 4, 8, 16, 32 or 64 (the template parameter), so a
// block is 64 padded channels = 16 quads whatever the group width; groups past G and channels past Cg are
// staged as zeros and never stored ("channel block not filled"). The row axis is the flattened (n, p, q)
// order of the implicit GEMM in tiles of R = 64 rows, so the BatchNorm partial contract (one (mean, M2) pair
// per channel and 64-row tile) holds unchanged.
//
// gconv_kernel<CGB, 0> (forward) / <CGB, 1> (data gradient): thread = (channel quad oq = t & 15, row slot
// t >> 4) owns one output quad for the 4 rows slot + 16 i. The reduction runs in chunks (kh, slice of
// SL = min(CGB, 32) reduce channels per group): per chunk the workgroup stages the rows' three kw taps of
// the block's channels in LDS with 16-byte loads (out-of-image taps, and for the stride-2 data gradient the
// taps of the wrong parity, are zeros: no sub-pixel classes, no zero-fill launch) and the chunk's weights as
// wl[kw][reduce channel][64 output channels] -- the forward transposes W on the way into LDS, the data
// gradient copies it (W's innermost axis is its output axis), so neither needs a W^T buffer. Per tap and
// reduce quad a thread then reads four float4 of w (contiguous over oq: conflict-free), and per row one
// float4 of x (broadcast to the group's threads) for 16 FMAs. Cg = 64 is sliced in two through LDS.
// Epilogue: bias, the tile goes through LDS once, the statistics are an exact two-pass per 16-row segment
// merged with Chan's formula, and y leaves as 16-byte row segments (plus the optional addend).
//   LDS: taps 64 x 3 x (64 + 4) floats = 51 KiB (CGB = 64: 32 + 4 wide, 27 KiB) + weights 3 x SL x 64
//   floats (3 / 6 / 12 / 24 / 24 KiB): 54 .. 75 KiB, i.e. two workgroups (8 waves) per CU, LDS-bound; the
//   kernels are latency-bound at that occupancy for Cg <= 8 (192 .. 384 FMAs per thread and chunk).
//
// gconv_wgrad_kernel<CGB>: the M = N P Q rows are cut into S chunks of whole 64-row tiles (gconv_wgrad_chunks:
// enough chunks for four workgroups per CU, never less than one tile each); grid = (S, channel blocks, 3 kh).
// A thread owns the (output quad, input quad) pair u of its block for one kh and all three kw -- 48
// accumulators -- and the 256 / (4 CGB) threads of a pair take every (256 / 4 CGB)-th row of a staged tile
// (dY rows 64 x 68 floats beside the forward's tap tile: 68 KiB, two workgroups per CU). They meet once in
// LDS in ascending lane order, the block's Cg_out x 3 Cg_in values go to slab [S][Co 9 Cg_in], and
// slab_sum_launch adds the S slabs in fixed order into the destination.
#include "common.h"
#include "kernels.h"

namespace cdp {
namespace {

constexpr int kR = kGconvRows;
constexpr int kYS = 68;  // row stride of a staged 64-channel tile (floats)

template <int CGB>
struct GTile {
  static constexpr int GPB = 64 / CGB;             // groups per channel block
  static constexpr int SL = CGB < 32 ? CGB : 32;   // reduce channels per group and chunk
  static constexpr int XS = GPB * SL + 4;          // tap row stride
  static constexpr int X_FLOATS = kR * 3 * XS > kR * kYS ? kR * 3 * XS : kR * kYS;
  static constexpr int W_FLOATS = 3 * SL * 64;
};

// rows m0 .. m0 + 63 of an [N][OH][OW] grid: source image base (pixels; -1 past M) and the tap origin.
// mode 0 (forward gather): source (oh s - 1 + kh, ow s - 1 + kw); mode 1 (data gradient): ((oh + 1 - kh) / s, ..)
__device__ __forceinline__ void row_setup(int* rowi, int m0, int M, int OH, int OW, int SHW, int mode, int stride) {
  const int t = threadIdx.x;
  if (t < kR) {
    const int m = m0 + t;
    int base = -1, a = 0, b = 0;
    if (m < M) {
      const int n = m / (OH * OW);
      const int rem = m - n * OH * OW;
      const int oh = rem / OW, ow = rem - oh * OW;
      base = n * SHW;
      a = mode == 0 ? oh * stride - 1 : oh + 1;
      b = mode == 0 ? ow * stride - 1 : ow + 1;
    }
    rowi[t] = base;
    rowi[kR + t] = a;
    rowi[2 * kR + t] = b;
  }
}

// the source pixel of row r's tap (kh, kw), -1 when it is padding (or, mode 1, of the wrong stride parity)
__device__ __forceinline__ int tap_pixel(const int* rowi, int r, int kh, int kw, int SH, int SW, int mode,
                                         int stride) {
  const int base = rowi[r];
  if (base < 0) return -1;
  int ih, iw;
  if (mode == 0) {
    ih = rowi[kR + r] + kh;
    iw = rowi[2 * kR + r] + kw;
    if (ih < 0 || iw < 0) return -1;
  } else {
    const int th = rowi[kR + r] - kh, tw = rowi[2 * kR + r] - kw;
    if (th < 0 || tw < 0 || ((th | tw) & (stride - 1))) return -1;  // stride is 1 or 2
    ih = th >> (stride - 1);
    iw = tw >> (stride - 1);
  }
  if (ih >= SH || iw >= SW) return -1;
  return base + ih * SW + iw;
}

// xl[r][kw][gl * SL + c] = src[pixel(r, kh, kw)][(g0 + gl) cs + c0 + c] for c < SL; zeros outside the image,
// past group G and past the group's cs channels
template <int GPB, int SL>
__device__ __forceinline__ void stage_taps(float* xl, const int* rowi, const float* __restrict__ src, int kh, int SH,
                                           int SW, int cs, int c0, int g0, int G, int mode, int stride) {
  constexpr int XQ = GPB * SL / 4, XS = GPB * SL + 4;
  const int Cs = G * cs;
  for (int e = threadIdx.x; e < kR * 3 * XQ; e += 256) {
    const int qd = e % XQ, rk = e / XQ;
    const int kw = rk % 3, r = rk / 3;
    const int gl = qd * 4 / SL, c = c0 + qd * 4 - gl * SL;
    float4 v = f4zero();
    const int pix = tap_pixel(rowi, r, kh, kw, SH, SW, mode, stride);
    if (pix >= 0 && g0 + gl < G && c < cs) v = ld4(src + (long long)pix * Cs + (g0 + gl) * cs + c);
    st4(xl + (r * 3 + kw) * XS + qd * 4, v);
  }
}

__device__ __forceinline__ void fma4(float4& a, float s, const float4& w) {
  a.x = fmaf(s, w.x, a.x);
  a.y = fmaf(s, w.y, a.y);
  a.z = fmaf(s, w.z, a.z);
  a.w = fmaf(s, w.w, a.w);
}

template <int CGB, int MODE>
__global__ __launch_bounds__(256) void gconv_kernel(GConvParams p) {
  using T = GTile<CGB>;
  constexpr int SL = T::SL, XS = T::XS;
  __shared__ __align__(16) float xl[T::X_FLOATS];
  __shared__ __align__(16) float wl[T::W_FLOATS];
  __shared__ int rowi[3 * kR];
  const int t = threadIdx.x;
  const int m0 = blockIdx.x * kR, g0 = blockIdx.y * T::GPB;
  const int cs = MODE == 0 ? p.cgi : p.cgo;  // per group: reduce channels of the source,
  const int cd = MODE == 0 ? p.cgo : p.cgi;  // channels of the destination
  const int Cd = p.G * cd;
  row_setup(rowi, m0, p.M, p.OH, p.OW, p.SH * p.SW, MODE, p.stride);
  __syncthreads();
  const int oq = t & 15, ps = t >> 4;
  const int gl = oq * 4 / CGB;
  float4 acc[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
  const int nsl = (cs + SL - 1) / SL;
  for (int kh = 0; kh < 3; ++kh)
    for (int sl = 0; sl < nsl; ++sl) {
      const int c0 = sl * SL;
      stage_taps<T::GPB, SL>(xl, rowi, p.src, kh, p.SH, p.SW, cs, c0, g0, p.G, MODE, p.stride);
      if (MODE == 0) {  // wl[kw][ci][col] = W[col's co][kh][kw][c0 + ci]: transposed on the way in
        for (int e = t; e < 3 * (SL / 4) * 64; e += 256) {
          const int col = e & 63, rest = e >> 6;
          const int rq = rest % (SL / 4), kw = rest / (SL / 4);
          const int g = g0 + col / CGB, c = col % CGB, ci = c0 + rq * 4;
          float4 v = f4zero();
          if (g < p.G && c < p.cgo && ci < p.cgi) v = ld4(p.w + ((long long)(g * p.cgo + c) * 9 + kh * 3 + kw) * p.cgi + ci);
          float* d = wl + (kw * SL + rq * 4) * 64 + col;
          d[0] = v.x;
          d[64] = v.y;
          d[128] = v.z;
          d[192] = v.w;
        }
      } else {  // wl[kw][co][col] = W[c0 + co][kh][kw][col's ci]: W's innermost axis is the output axis
        for (int e = t; e < 3 * SL * 16; e += 256) {
          const int q = e & 15, rest = e >> 4;
          const int cl = rest % SL, kw = rest / SL;
          const int g = g0 + q * 4 / CGB, ci = q * 4 % CGB, co = c0 + cl;
          float4 v = f4zero();
          if (g < p.G && ci < p.cgi && co < p.cgo) v = ld4(p.w + ((long long)(g * p.cgo + co) * 9 + kh * 3 + kw) * p.cgi + ci);
          st4(wl + (kw * SL + cl) * 64 + q * 4, v);
        }
      }
      __syncthreads();
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int rq = 0; rq < SL / 4; ++rq) {
          const float* wp = wl + (kw * SL + rq * 4) * 64 + oq * 4;
          const float4 w0 = ld4(wp), w1 = ld4(wp + 64), w2 = ld4(wp + 128), w3 = ld4(wp + 192);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float4 xv = ld4(xl + ((ps + 16 * i) * 3 + kw) * XS + gl * SL + rq * 4);
            fma4(acc[i], xv.x, w0);
            fma4(acc[i], xv.y, w1);
            fma4(acc[i], xv.z, w2);
            fma4(acc[i], xv.w, w3);
          }
        }
      __syncthreads();
    }
  // the tile goes through LDS: statistics by column, stores as 16-byte row segments
  const int gq = g0 + gl, cq = oq * 4 - gl * CGB;
  float4 bv = f4zero();
  if (p.bias && gq < p.G && cq < cd) bv = ld4(p.bias + gq * cd + cq);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float4 v = acc[i];
    v.x += bv.x;
    v.y += bv.y;
    v.z += bv.z;
    v.w += bv.w;
    st4(xl + (ps + 16 * i) * kYS + oq * 4, v);
  }
  __syncthreads();
  if (p.part) {  // (mean, M2) of every column over the tile's valid rows: two exact passes per 16-row segment
    const int col = t & 63, seg = t >> 6;
    const int nv = max(0, min(16, p.M - m0 - seg * 16));
    float s = 0.f;
    for (int r = 0; r < nv; ++r) s += xl[(seg * 16 + r) * kYS + col];
    const float mean_s = nv > 0 ? s / (float)nv : 0.f;
    float q = 0.f;
    for (int r = 0; r < nv; ++r) {
      const float d = xl[(seg * 16 + r) * kYS + col] - mean_s;
      q = fmaf(d, d, q);
    }
    wl[(seg * 64 + col) * 2] = mean_s;
    wl[(seg * 64 + col) * 2 + 1] = q;
    __syncthreads();
    const int g = g0 + col / CGB, c = col % CGB;
    if (seg == 0 && g < p.G && c < cd) {
      float cnt = (float)nv, mean = mean_s, m2 = q;
      for (int z = 1; z < 4; ++z) {
        const float nb = (float)max(0, min(16, p.M - m0 - z * 16));
        if (nb > 0.f) {
          const float mb = wl[(z * 64 + col) * 2], qb = wl[(z * 64 + col) * 2 + 1];
          const float tot = cnt + nb, delta = mb - mean;
          mean = fmaf(delta, nb / tot, mean);
          m2 += qb + delta * delta * (cnt * nb / tot);
          cnt = tot;
        }
      }
      float* dst = p.part + ((long long)blockIdx.x * Cd + g * cd + c) * 2;
      dst[0] = mean;
      dst[1] = m2;
    }
  }
  for (int e = t; e < kR * 16; e += 256) {
    const int q = e & 15, r = e >> 4;
    const int g = g0 + q * 4 / CGB, c = q * 4 % CGB;
    if (m0 + r < p.M && g < p.G && c < cd) {
      float4 v = ld4(xl + r * kYS + q * 4);
      const long long o = (long long)(m0 + r) * Cd + g * cd + c;
      if (p.addend) {  // may alias dst: read and written by this thread only
        const float4 a = ld4(p.addend + o);
        v.x += a.x;
        v.y += a.y;
        v.z += a.z;
        v.w += a.w;
      }
      st4(p.dst + o, v);
    }
  }
}

template <int CGB>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(GConvWgradParams p) {
  constexpr int GPB = 64 / CGB, U = 4 * CGB, RL = 256 / U;
  __shared__ __align__(16) float xl[kR * 3 * kYS];  // the tap tile; the lanes' meeting place at the end
  __shared__ __align__(16) float dyl[kR * kYS];
  __shared__ int rowi[3 * kR];
  static_assert(RL * 12 * U * 4 <= kR * 3 * kYS, "the lane reduction must fit the tap tile");
  const int t = threadIdx.x;
  const int u = t % U, rl = t / U;
  const int oq = u & 15, iq = u >> 4;
  const int gl = oq * 4 / CGB;
  const int kh = blockIdx.z, g0 = blockIdx.y * GPB;
  const int Co = p.G * p.cgo;
  const int ntiles = (p.M + kR - 1) / kR;
  const int tile0 = blockIdx.x * p.tiles_per_chunk, tile1 = min(tile0 + p.tiles_per_chunk, ntiles);
  float4 acc[3][4];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[kw][j] = f4zero();
  for (int tile = tile0; tile < tile1; ++tile) {
    const int m0 = tile * kR;
    row_setup(rowi, m0, p.M, p.P, p.Q, p.H * p.W, 0, p.stride);
    __syncthreads();
    stage_taps<GPB, CGB>(xl, rowi, p.x, kh, p.H, p.W, p.cgi, 0, g0, p.G, 0, p.stride);
    for (int e = t; e < kR * 16; e += 256) {
      const int q = e & 15, r = e >> 4;
      const int g = g0 + q * 4 / CGB, c = q * 4 % CGB;
      float4 v = f4zero();
      if (m0 + r < p.M && g < p.G && c < p.cgo) v = ld4(p.dy + (long long)(m0 + r) * Co + g * p.cgo + c);
      st4(dyl + r * kYS + q * 4, v);
    }
    __syncthreads();
    for (int r = rl; r < kR; r += RL) {  // rows past M are staged as zeros
      const float4 dv = ld4(dyl + r * kYS + oq * 4);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float4 xv = ld4(xl + (r * 3 + kw) * kYS + gl * CGB + iq * 4);
        fma4(acc[kw][0], dv.x, xv);
        fma4(acc[kw][1], dv.y, xv);
        fma4(acc[kw][2], dv.z, xv);
        fma4(acc[kw][3], dv.w, xv);
      }
    }
    __syncthreads();
  }
  // red[lane][v = kw * 4 + j][pair u]: summed over the lanes in ascending order
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int j = 0; j < 4; ++j) st4(xl + ((rl * 12 + kw * 4 + j) * U + u) * 4, acc[kw][j]);
  __syncthreads();
  const long long n = (long long)Co * 9 * p.cgi;
  for (int e = t; e < 12 * U; e += 256) {
    const int u2 = e % U, v = e / U;
    float4 s = ld4(xl + (v * U + u2) * 4);
    for (int z = 1; z < RL; ++z) {
      const float4 a = ld4(xl + ((z * 12 + v) * U + u2) * 4);
      s.x += a.x;
      s.y += a.y;
      s.z += a.z;
      s.w += a.w;
    }
    const int kw = v >> 2, j = v & 3;
    const int oq2 = u2 & 15, ci = (u2 >> 4) * 4;
    const int g = g0 + oq2 * 4 / CGB, co = oq2 * 4 % CGB + j;
    if (g < p.G && co < p.cgo && ci < p.cgi)
      st4(p.slab + (long long)blockIdx.x * n + ((long long)(g * p.cgo + co) * 9 + kh * 3 + kw) * p.cgi + ci, s);
  }
}

int bucket(int cgi, int cgo) {
  const int c = cgi > cgo ? cgi : cgo;
  return c <= 4 ? 4 : c <= 8 ? 8 : c <= 16 ? 16 : c <= 32 ? 32 : 64;
}

template <int MODE>
void launch_mode(const GConvParams& p, hipStream_t st) {
  const int cgb = bucket(p.cgi, p.cgo);
  const dim3 grid((unsigned)((p.M + kR - 1) / kR), (unsigned)((p.G + 64 / cgb - 1) / (64 / cgb)));
  switch (cgb) {
    case 4: hipLaunchKernelGGL((gconv_kernel<4, MODE>), grid, dim3(256), 0, st, p); break;
    case 8: hipLaunchKernelGGL((gconv_kernel<8, MODE>), grid, dim3(256), 0, st, p); break;
    case 16: hipLaunchKernelGGL((gconv_kernel<16, MODE>), grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL((gconv_kernel<32, MODE>), grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL((gconv_kernel<64, MODE>), grid, dim3(256), 0, st, p); break;
  }
}

}  // namespace

void gconv_fwd_launch(const GConvParams& p, hipStream_t st) { launch_mode<0>(p, st); }
void gconv_dgrad_launch(const GConvParams& p, hipStream_t st) { launch_mode<1>(p, st); }

// The split of the weight gradient's M rows: enough chunks that (chunks x channel blocks x 3 kh) is four
// workgroups per CU, in whole 64-row tiles and never more chunks than tiles. Returns {S, tiles per chunk}.
GConvChunks gconv_wgrad_chunks(long long M, int G, int cgi, int cgo, int cus) {
  const int gpb = 64 / bucket(cgi, cgo);
  const long long blocks = 3LL * ((G + gpb - 1) / gpb);
  const long long ntiles = (M + kR - 1) / kR;
  long long want = (4LL * cus + blocks - 1) / blocks;
  want = want < 1 ? 1 : want > ntiles ? ntiles : want;
  const long long tpc = (ntiles + want - 1) / want;
  return GConvChunks{(int)((ntiles + tpc - 1) / tpc), (int)tpc};
}

void gconv_wgrad_launch(const GConvWgradParams& p, int S, hipStream_t st) {
  const int cgb = bucket(p.cgi, p.cgo);
  const dim3 grid((unsigned)S, (unsigned)((p.G + 64 / cgb - 1) / (64 / cgb)), 3);
  switch (cgb) {
    case 4: hipLaunchKernelGGL(gconv_wgrad_kernel<4>, grid, dim3(256), 0, st, p); break;
    case 8: hipLaunchKernelGGL(gconv_wgrad_kernel<8>, grid, dim3(256), 0, st, p); break;
    case 16: hipLaunchKernelGGL(gconv_wgrad_kernel<16>, grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL(gconv_wgrad_kernel<32>, grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL(gconv_wgrad_kernel<64>, grid, dim3(256), 0, st, p); break;
  }
}

}  // namespace cdp
