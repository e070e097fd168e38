// Stochastic depth (Huang et al.; timm drop_path, torchvision StochasticDepth(mode="row")) scales,
// drawn on the device.
//
// One scale per (residual block, image): s = 0 with probability p (the block's branch is dropped for
// that image), else 1 / (1 - p). It is a pure function of (seed, step counter, block, image, p), so a
// table of any step can be written again from those inputs, and a replayed hipGraph that reads the
// counter from device memory drops different images at every replay. drop_path_draw_kernel
// (drop_path.hip) writes one step's [nb, B] table and advances the counter; drop_path_table_kernel
// evaluates the same function for a schedule of counters.
//
// Random source: the counter-based hash of mix.h, keyed by (seed, counter, block) under a stream tag
// of its own and walked by the image index, so the loader's crops, flips, windows, mixes and erase
// boxes are the same bits with drop path on or off.
#pragma once
#include <hip/hip_runtime.h>

#include "mix.h"

namespace cdp {

// u(seed, counter, block, image) in (0, 1): MixRng::uniform's bit rule at draw index `image`
__host__ __device__ __forceinline__ float drop_path_uniform(unsigned long long seed, unsigned long long ctr, int block,
                                                            int image) {
  MixRng g{mix_hash(mix_hash(seed ^ 0x64726F702D706174ull) ^
                    mix_hash(mix_hash(ctr + 0x682D73636C2D3031ull) + (unsigned long long)block)),
           (unsigned)image};
  return g.uniform();
}

// dropped when u < p (fp32 compare); a kept image's scale is 1.f / (1.f - p) in fp32
__host__ __device__ __forceinline__ float drop_path_scale(unsigned long long seed, unsigned long long ctr, int block,
                                                          int image, float p) {
  return drop_path_uniform(seed, ctr, block, image) < p ? 0.f : 1.f / (1.f - p);
}

}  // namespace cdp
