// torch.argmax's order over (value, index) candidates, shared by the token argmax
// (tokens.hip) and the per-pixel class argmax of the agent's post-processing (agent.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace e2ep {

// true where candidate (a, ai) ranks above (b, bi): the first index of the largest value
// wins; a NaN ranks above every number, and the first NaN wins.
__device__ __forceinline__ bool argmax_beats(float a, int ai, float b, int bi) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return an;
  if (an) return ai < bi;
  return a > b || (a == b && ai < bi);
}

}  // namespace e2ep
