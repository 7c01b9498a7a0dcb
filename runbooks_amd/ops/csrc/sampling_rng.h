// Counter-based RNG and Gumbel noise shared by the sampling kernels
// (sampling.hip, sample_batch.hip). One definition each, so a token drawn
// by either kernel from the same (seed, row, col) sees the same noise.
#pragma once

#include "common.h"

namespace rb {

RB_DEV uint32_t hash_u32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// uniform in (0, 1]
RB_DEV float rng_uniform(uint64_t seed, uint32_t row, uint32_t col) {
  uint32_t h = hash_u32((uint32_t)seed ^ hash_u32(row * 0x9e3779b9U ^ hash_u32(col)));
  h ^= (uint32_t)(seed >> 32);
  h = hash_u32(h);
  return ((float)h + 1.0f) * (1.0f / 4294967296.0f);
}

// log(-log(u)) for u in (0, 1]; the Gumbel(0,1) sample is its negation
RB_DEV float neg_gumbel(float u) { return __logf(-__logf(u)); }

}  // namespace rb
