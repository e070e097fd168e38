// Direct depthwise 3x3 convolution (groups == C == Co, pad 1, stride 1 or 2) in plain fp32 FMA: forward, data
// gradient and weight gradient of MobileNet's depthwise layers. NHWC activations, weight [C][9] (a [C, 1, 3, 3]
// tensor, contiguous or channels_last); C a multiple of 4.
//
// Why not gconv.hip at Cg = 1 and why no matrix instructions: a depthwise conv has no channel reduction, so the
// product has no K dimension to tile -- every output is 9 FMAs on its own channel and the layer is pure data
// movement (read x once, write y once). gconv pads a group to 4 channels and runs LDS-bound at two workgroups
// per CU; here nothing but the BatchNorm partials (and the weight gradient's final meeting) touches LDS. Operands
// and accumulation are exact fp32, every result is one FMA chain in a fixed order (the nine taps kh-major, padding
// taps as zeros), so the kernels do not depend on the conv engine and two calls give the same bits. No atomics, no
// host synchronisation, nothing a hipGraph cannot capture.
//
// How the work is split (all kernels, 256 threads): thread = (channel quad ql = t % CQ, row slot t / CQ) with
// CQ = 16 quads (64 channels) per workgroup for C >= 64 and 8 (32 channels) below, so the 32-channel first layer
// fills its lanes; quads past C load and store nothing ("channel block not filled"). A slot owns kL = 4
// consecutive rows of the flattened (n, p, q) order, a workgroup the 256 / CQ slots = R = 64 (CQ = 16) or 128
// (CQ = 8) consecutive rows of one tile, and R is the rows per BatchNorm partial (dwconv_rows). Row tiles go
// through xcd_remap, so the tiles that share input rows sit on one XCD and meet in its L2.
// The 9 weights of a thread's 4 channels are 36 contiguous floats of [C][9]: nine 16-byte loads, transposed in
// registers into nine float4 (one per tap) that live for the whole kernel. No W^T buffer, no LDS for weights.
//
// dwconv_slide_kernel (forward; the stride-1 data gradient with the taps flipped): a thread keeps a 3 x 3 window
// of float4 in registers and slides it along its 4 rows: a step to the next q loads one new column (3 float4,
// stride 1) or two (stride 2) and keeps the rest; the window is refilled where the run starts or wraps to q = 0.
// A thread so fetches 18 (27 at stride 2) float4 per 4 outputs instead of 36, each 16-byte load a full quad of a
// 256-byte (CQ = 16) row segment; the vertical reuse between image rows is the L1's and, through the tile order,
// the L2's. Padding taps are predicated loads that read as zero: no zero-filled copy of x. Epilogue: bias,
// optional addend, 16-byte stores. With statistics a thread makes the exact two-pass (mean, M2) of its own <= 4
// rows in registers, and the slots meet in LDS, merged in ascending order with Chan's formula by one thread per
// channel: the conv_igemm contract, [ceil(M / R)][C][2], the last part holding M - b R rows.
//   LDS: 256 x 2 float4 = 8 KiB (statistics only); 114 VGPRs, so registers set the occupancy: four workgroups
//   (16 waves) per CU. The stride-2 data gradient uses no LDS and 68 VGPRs: seven workgroups per CU.
//
// dwconv_dgrad_s2_kernel (stride-2 data gradient): same ownership over the input pixels. An input pixel (ih, iw)
// meets only the taps with kh = ih + 1, kw = iw + 1 (mod 2): 1, 2 or 4 of the 9, predicated per lane, and a
// wave skips the taps none of its lanes has (the lanes of a wave share the row parity and, step by step, the
// column parity). Only those are loaded and multiplied: no sub-pixel buffers, no zero-fill launch, no zeros fed
// through the FMAs. The chain runs kh-major over the taps that exist. Optional addend as in gconv2d_dgrad.
//
// dwconv_wgrad_kernel: dW[c][tap] = sum over rows of dY[row][c] x[tap(row)][c], 9 values per channel reduced over
// all M rows. The M rows are cut into S chunks of whole R-row tiles (dwconv_wgrad_chunks: enough chunks for four
// workgroups per CU, never less than one tile each); grid = (S, channel blocks). A thread walks its 4 rows of
// every tile of the chunk with the forward's sliding window and holds 9 float4 accumulators (tap x channel quad);
// the row slots meet once in LDS (256 x 9 float4 = 36 KiB, room for four workgroups per CU) in ascending slot order,
// the block writes its C_block x 9 values to slab [S][C 9], and slab_sum_launch adds the S slabs in fixed order.
// The build holds it in 207 VGPRs without scratch, so registers (two workgroups per CU), not LDS, set its
// occupancy; an occupancy bound of three or four waves per SIMD spills.
#include "common.h"
#include "kernels.h"

namespace cdp {
namespace {

constexpr int kL = 4;  // consecutive rows of a slot

__device__ __forceinline__ void fmaq(float4& a, const float4& x, const float4& w) {
  a.x = fmaf(x.x, w.x, a.x);
  a.y = fmaf(x.y, w.y, a.y);
  a.z = fmaf(x.z, w.z, a.z);
  a.w = fmaf(x.w, w.w, a.w);
}

__device__ __forceinline__ void addq(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// wt[k] = tap k of the four channels at w (36 contiguous floats of [C][9]); flip: tap 8 - k (the data gradient)
__device__ __forceinline__ void load_taps(float4 (&wt)[9], const float* __restrict__ w, bool on, bool flip) {
  float f[36];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float4 v = on ? ld4(w + 4 * i) : f4zero();
    f[4 * i] = v.x;
    f[4 * i + 1] = v.y;
    f[4 * i + 2] = v.z;
    f[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float4 a = make_float4(f[k], f[9 + k], f[18 + k], f[27 + k]);
    const float4 b = make_float4(f[8 - k], f[17 - k], f[26 - k], f[35 - k]);
    wt[k] = flip ? b : a;
  }
}

// one window column: src pixels (n, ih0 .. ih0 + 2, iw) of an [N][SH][SW][C] tensor, zeros outside the image
__device__ __forceinline__ void load_col(float4 (&col)[3], const float* __restrict__ src, bool on, int n, int ih0,
                                         int iw, int SH, int SW, int C, int c) {
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = ih0 + kh;
    col[kh] = f4zero();
    if (on && ih >= 0 && ih < SH && iw >= 0 && iw < SW) col[kh] = ld4(src + (long long)((n * SH + ih) * SW + iw) * C + c);
  }
}

// the window of output (n, oh, ow): refilled at the start of a run (first) and at ow == 0, slid otherwise
__device__ __forceinline__ void slide(float4 (&c0)[3], float4 (&c1)[3], float4 (&c2)[3], const float* __restrict__ src,
                                      bool on, bool first, int n, int oh, int ow, int stride, int SH, int SW, int C,
                                      int c) {
  const int ih0 = oh * stride - 1, iw0 = ow * stride - 1;
  if (first || ow == 0) {
    load_col(c0, src, on, n, ih0, iw0, SH, SW, C, c);
    load_col(c1, src, on, n, ih0, iw0 + 1, SH, SW, C, c);
  } else if (stride == 1) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      c0[kh] = c1[kh];
      c1[kh] = c2[kh];
    }
  } else {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) c0[kh] = c2[kh];
    load_col(c1, src, on, n, ih0, iw0 + 1, SH, SW, C, c);
  }
  load_col(c2, src, on, n, ih0, iw0 + 2, SH, SW, C, c);
}

struct RowPos {
  int n, oh, ow;
};
__device__ __forceinline__ RowPos row_pos(int m, int M, int OH, int OW) {
  RowPos r{0, 0, 0};
  if (m < M) {
    r.n = m / (OH * OW);
    const int rem = m - r.n * OH * OW;
    r.oh = rem / OW;
    r.ow = rem - r.oh * OW;
  }
  return r;
}
__device__ __forceinline__ void row_next(RowPos& r, int OH, int OW) {
  if (++r.ow == OW) {
    r.ow = 0;
    if (++r.oh == OH) {
      r.oh = 0;
      ++r.n;
    }
  }
}

template <int CQ>
__global__ __launch_bounds__(256) void dwconv_slide_kernel(DwConvParams p) {
  constexpr int SLOTS = 256 / CQ, R = SLOTS * kL, CW = CQ * 4;
  __shared__ __align__(16) float sm[SLOTS * CQ * 8];
  const int t = threadIdx.x, ql = t % CQ, slot = t / CQ;
  const int c = ((int)blockIdx.y * CQ + ql) * 4;
  const bool con = c < p.C;
  const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int m0 = tile * R, mb = m0 + slot * kL;
  float4 wt[9];
  load_taps(wt, p.w + (long long)c * 9, con, p.flip != 0);
  float4 bv = f4zero();
  if (p.bias && con) bv = ld4(p.bias + c);
  RowPos r = row_pos(mb, p.M, p.OH, p.OW);
  float4 out[kL], c0[3], c1[3], c2[3];
#pragma unroll
  for (int i = 0; i < kL; ++i) {
    const bool on = con && mb + i < p.M;
    slide(c0, c1, c2, p.src, on, i == 0, r.n, r.oh, r.ow, p.stride, p.SH, p.SW, p.C, c);
    float4 acc = f4zero();
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      fmaq(acc, c0[kh], wt[kh * 3]);
      fmaq(acc, c1[kh], wt[kh * 3 + 1]);
      fmaq(acc, c2[kh], wt[kh * 3 + 2]);
    }
    addq(acc, bv);
    out[i] = acc;
    if (on) {
      const long long o = (long long)(mb + i) * p.C + c;
      if (p.addend) addq(acc, ld4(p.addend + o));  // may alias dst: read and written by this thread only
      st4(p.dst + o, acc);
    }
    row_next(r, p.OH, p.OW);
  }
  if (p.part) {  // (mean, M2) of the slot's valid rows: two exact passes in registers; the slots meet in LDS
    const int nv = max(0, min(kL, p.M - mb));
    float4 s = f4zero();
#pragma unroll
    for (int i = 0; i < kL; ++i)
      if (i < nv) addq(s, out[i]);
    const float fn = (float)max(nv, 1);
    const float4 mean = make_float4(s.x / fn, s.y / fn, s.z / fn, s.w / fn);
    float4 q = f4zero();
#pragma unroll
    for (int i = 0; i < kL; ++i)
      if (i < nv) {
        const float4 d = make_float4(out[i].x - mean.x, out[i].y - mean.y, out[i].z - mean.z, out[i].w - mean.w);
        fmaq(q, d, d);
      }
    st4(sm + (slot * CQ + ql) * 8, mean);
    st4(sm + (slot * CQ + ql) * 8 + 4, q);
    __syncthreads();
    const int cc = (int)blockIdx.y * CW + t;
    if (t < CW && cc < p.C) {
      const float* col = sm + (t >> 2) * 8 + (t & 3);
      float cnt = (float)min(kL, p.M - m0), mean_c = col[0], m2 = col[4];  // slot 0 always holds a row
      for (int z = 1; z < SLOTS; ++z) {
        const float nb = (float)max(0, min(kL, p.M - m0 - z * kL));
        if (nb > 0.f) {
          const float mz = col[z * CQ * 8], qz = col[z * CQ * 8 + 4];
          const float tot = cnt + nb, delta = mz - mean_c;
          mean_c = fmaf(delta, nb / tot, mean_c);
          m2 += qz + delta * delta * (cnt * nb / tot);
          cnt = tot;
        }
      }
      float* dst = p.part + ((long long)tile * p.C + cc) * 2;
      dst[0] = mean_c;
      dst[1] = m2;
    }
  }
}

// src = dY [N][SH][SW][C] (SH, SW = P, Q), dst = dX rows (n, ih, iw) over OH, OW = H, W
template <int CQ>
__global__ __launch_bounds__(256) void dwconv_dgrad_s2_kernel(DwConvParams p) {
  constexpr int SLOTS = 256 / CQ, R = SLOTS * kL;
  const int t = threadIdx.x, ql = t % CQ, slot = t / CQ;
  const int c = ((int)blockIdx.y * CQ + ql) * 4;
  const bool con = c < p.C;
  const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int mb = tile * R + slot * kL;
  float4 wt[9];
  load_taps(wt, p.w + (long long)c * 9, con, false);
  RowPos r = row_pos(mb, p.M, p.OH, p.OW);
#pragma unroll
  for (int i = 0; i < kL; ++i) {
    const bool on = con && mb + i < p.M;
    float4 acc = f4zero();
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int th = r.oh + 1 - kh, tw = r.ow + 1 - kw;
        if (on && th >= 0 && tw >= 0 && !((th | tw) & 1) && (th >> 1) < p.SH && (tw >> 1) < p.SW)
          fmaq(acc, ld4(p.src + (long long)((r.n * p.SH + (th >> 1)) * p.SW + (tw >> 1)) * p.C + c), wt[kh * 3 + kw]);
      }
    if (on) {
      const long long o = (long long)(mb + i) * p.C + c;
      if (p.addend) addq(acc, ld4(p.addend + o));  // may alias dst: read and written by this thread only
      st4(p.dst + o, acc);
    }
    row_next(r, p.OH, p.OW);
  }
}

template <int CQ>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(DwConvWgradParams p) {
  constexpr int SLOTS = 256 / CQ, R = SLOTS * kL, CW = CQ * 4;
  __shared__ __align__(16) float red[SLOTS * 9 * CW];
  const int t = threadIdx.x, ql = t % CQ, slot = t / CQ;
  const int c = ((int)blockIdx.y * CQ + ql) * 4;
  const bool con = c < p.C;
  const int chunk = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int ntiles = (p.M + R - 1) / R;
  const int tile0 = chunk * p.tiles_per_chunk, tile1 = min(tile0 + p.tiles_per_chunk, ntiles);
  float4 acc[9], c0[3], c1[3], c2[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = f4zero();
  for (int tile = tile0; tile < tile1; ++tile) {
    const int mb = tile * R + slot * kL;
    RowPos r = row_pos(mb, p.M, p.P, p.Q);
#pragma unroll
    for (int i = 0; i < kL; ++i) {
      const bool on = con && mb + i < p.M;  // rows past M add dY = 0 times an all-zero window
      slide(c0, c1, c2, p.x, on, i == 0, r.n, r.oh, r.ow, p.stride, p.H, p.W, p.C, c);
      const float4 dv = on ? ld4(p.dy + (long long)(mb + i) * p.C + c) : f4zero();
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        fmaq(acc[kh * 3], dv, c0[kh]);
        fmaq(acc[kh * 3 + 1], dv, c1[kh]);
        fmaq(acc[kh * 3 + 2], dv, c2[kh]);
      }
      row_next(r, p.P, p.Q);
    }
  }
  // red[slot][tap][quad]: summed over the slots in ascending order
#pragma unroll
  for (int k = 0; k < 9; ++k) st4(red + ((slot * 9 + k) * CQ + ql) * 4, acc[k]);
  __syncthreads();
  for (int e = t; e < 9 * CW; e += 256) {
    const int col = e / 9, k = e - col * 9;
    const int cc = (int)blockIdx.y * CW + col;
    float s = red[k * CW + col];
    for (int z = 1; z < SLOTS; ++z) s += red[(z * 9 + k) * CW + col];
    if (cc < p.C) p.slab[(long long)chunk * p.C * 9 + (long long)cc * 9 + k] = s;
  }
}

int quads(int C) { return C >= 64 ? 16 : 8; }

dim3 row_grid(long long M, int C) {
  const int cq = quads(C), R = 256 / cq * kL;
  return dim3((unsigned)((M + R - 1) / R), (unsigned)((C / 4 + cq - 1) / cq));
}

}  // namespace

// rows of a workgroup's tile = rows per BatchNorm partial
int dwconv_rows(int C) { return 256 / quads(C) * kL; }

void dwconv_fwd_launch(const DwConvParams& p_, hipStream_t st) {
  DwConvParams p = p_;
  p.flip = 0;
  if (quads(p.C) == 16)
    hipLaunchKernelGGL(dwconv_slide_kernel<16>, row_grid(p.M, p.C), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(dwconv_slide_kernel<8>, row_grid(p.M, p.C), dim3(256), 0, st, p);
}

// stride 1: the forward's sliding window over dY with the taps flipped (flip); stride 2: the parity gather
void dwconv_dgrad_launch(const DwConvParams& p_, hipStream_t st) {
  DwConvParams p = p_;
  p.flip = 1;
  p.bias = nullptr;
  p.part = nullptr;
  const bool wide = quads(p.C) == 16;
  if (p.stride == 1) {
    if (wide)
      hipLaunchKernelGGL(dwconv_slide_kernel<16>, row_grid(p.M, p.C), dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL(dwconv_slide_kernel<8>, row_grid(p.M, p.C), dim3(256), 0, st, p);
  } else if (wide) {
    hipLaunchKernelGGL(dwconv_dgrad_s2_kernel<16>, row_grid(p.M, p.C), dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL(dwconv_dgrad_s2_kernel<8>, row_grid(p.M, p.C), dim3(256), 0, st, p);
  }
}

// The split of the weight gradient's M rows: enough chunks that (chunks x channel blocks) is four workgroups per
// CU, in whole tiles and never more chunks than tiles. Returns {S, tiles per chunk}.
GConvChunks dwconv_wgrad_chunks(long long M, int C, int cus) {
  const int cq = quads(C), R = 256 / cq * kL;
  const long long blocks = (C / 4 + cq - 1) / cq;
  const long long ntiles = (M + R - 1) / R;
  long long want = (4LL * cus + blocks - 1) / blocks;
  want = want < 1 ? 1 : want > ntiles ? ntiles : want;
  const long long tpc = (ntiles + want - 1) / want;
  return GConvChunks{(int)((ntiles + tpc - 1) / tpc), (int)tpc};
}

void dwconv_wgrad_launch(const DwConvWgradParams& p, int S, hipStream_t st) {
  const int cq = quads(p.C);
  const dim3 grid((unsigned)S, (unsigned)((p.C / 4 + cq - 1) / cq));
  if (cq == 16)
    hipLaunchKernelGGL(dwconv_wgrad_kernel<16>, grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(dwconv_wgrad_kernel<8>, grid, dim3(256), 0, st, p);
}

}  // namespace cdp
