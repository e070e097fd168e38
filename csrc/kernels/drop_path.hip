// Stochastic-depth scale tables (drop_path.h), gfx950.
#include <stdexcept>

#include "drop_path.h"
#include "kernels.h"

namespace cdp {
namespace {

// One training forward's table: out[i][b] = drop_path_scale(seed, counter[0], i, b, rates[i]), then
// counter[0] += 1. A single workgroup (nb * B is a few thousand elements at most): every thread reads
// the counter, the barrier keeps thread 0's store behind all of those reads, and thread 0 stores
// counter + 1 after its share of the table. No other workgroup exists, so nothing else has to arrive.
__global__ __launch_bounds__(256) void drop_path_draw_kernel(long long* counter, unsigned long long seed,
                                                            const float* __restrict__ rates, int nb, int B,
                                                            float* __restrict__ out) {
  const long long ctr = counter[0];
  __syncthreads();
  const int total = nb * B;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int blk = i / B, img = i - blk * B;
    out[i] = drop_path_scale(seed, (unsigned long long)ctr, blk, img, rates[blk]);
  }
  if (threadIdx.x == 0) counter[0] = ctr + 1;
}

// out[t][i][b] = drop_path_scale(seed, first + t, i, b, rates[i]) for t < n: the tables a model will
// draw at those steps. Reads no counter and moves none.
__global__ __launch_bounds__(256) void drop_path_table_kernel(unsigned long long seed, long long first, long long total,
                                                             const float* __restrict__ rates, int nb, int B,
                                                             float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long row = i / B;  // t * nb + block
  const long long t = row / nb;
  const int blk = (int)(row - t * nb), img = (int)(i - row * B);
  out[i] = drop_path_scale(seed, (unsigned long long)(first + t), blk, img, rates[blk]);
}

}  // namespace

void drop_path_draw_launch(long long* counter, unsigned long long seed, const float* rates, int nb, int B, float* out,
                           hipStream_t st) {
  if (nb < 0 || B < 0 || (long long)nb * B > (1LL << 24))
    throw std::runtime_error("drop_path_draw: 0 <= nb * B <= 2^24");
  // (an empty table still advances the counter: a step is a step)
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3(1), dim3(256), 0, st, counter, seed, rates, nb, B, out);
}

void drop_path_table_launch(unsigned long long seed, long long first, long long n, const float* rates, int nb, int B,
                            float* out, hipStream_t st) {
  if (n <= 0 || nb <= 0 || B <= 0) return;
  const long long total = n * nb * B;
  if (total > (1LL << 31) - 256) throw std::runtime_error("drop_path_table: n * nb * B < 2^31");
  hipLaunchKernelGGL(drop_path_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, seed, first,
                     total, rates, nb, B, out);
}

}  // namespace cdp
