// The order of fp32 scores as unsigned integers, one definition for every kernel that ranks or counts by score
// (rank.hip: the high word of its 64-bit (score, candidate) key; auc.hip: the key of a logit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The monotone 32-bit image of a score: a < b as floats iff key(a) < key(b).  NaN -> 0, below every number (every NaN the
// same key); -0 as +0 (one key, 0x80000000); -inf -> 0x007fffff, +inf -> 0xff800000.  0xffffffff is the image of no score.
__device__ __forceinline__ uint32_t mi_score_key32(float s) {
  uint32_t u = __float_as_uint(s);
  if (s != s) u = 0u;
  else if (s == 0.f) u = 0x80000000u;
  else u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return u;
}
