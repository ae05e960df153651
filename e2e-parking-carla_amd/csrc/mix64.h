// The splitmix64 finaliser behind every counter-based draw of the library: the step's random
// numbers (small.hip k_rng_draw) and the photometric augmentation of the frame decode
// (decode.hip).  mix64(0) == 0xE220A8397B1DCDAF.
#pragma once
#include <hip/hip_runtime.h>

namespace e2ep {

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace e2ep
