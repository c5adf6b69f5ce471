// The planes format (mi_planes_t): the operands of the MLP's matrix-pipe GEMMs.  The one definition of it;
// tests/test_hip_planes.py::host_planes restates it in numpy.
//
// A matrix [rows][K] is held as fp16 high + low parts of x * 2^s with ONE power-of-two exponent s PER ROW, chosen so
// that the row's abs-max lands in [2^14, 2^15):
//     x * 2^s = hi + lo,   hi = fp16(x * 2^s)  (RNE),  lo = fp16(x * 2^s - hi)
// In memory it is K-BLOCK MAJOR: for each block of 16 k, all rows back to back, a row's piece being 16 x hi then 16 x lo
// (PL_ROWB bytes); blocks are blk_stride bytes apart.
#pragma once
#include "common.h"

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int PL_ROWB = 64;           // bytes of a row's piece of one 16-k block: 16 x hi (at 0), then 16 x lo (at PL_LO)
constexpr int PL_LO = 32;

// 2^s as bits (-126 <= s <= 127)
__device__ __forceinline__ float pl_pow2(int s) { return __uint_as_float(static_cast<uint32_t>(127 + s) << 23); }

// exponent s with amax * 2^s in [2^14, 2^15), clamped so that 2^s and 2^-s are normal numbers
__device__ __forceinline__ int pl_exp_for(float amax) {
  const int e = static_cast<int>((__float_as_uint(amax) >> 23) & 0xffu);
  return max(-100, min(100, 141 - e));
}

// the same for the largest entry of an abs-max vector (MI_AMAX_SLOTS floats): a matrix-wide exponent
__device__ __forceinline__ int pl_scale_exp(const float* __restrict__ amax) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < MI_AMAX_SLOTS; ++j) m = fmaxf(m, amax[j]);
  return pl_exp_for(m);
}

// The planes of two scaled values u0, u1 (u = x * 2^s): hi and lo as packed fp16 pairs, u0 in the low half.
// KEEP_POSITIVE: a positive value stays positive in the high plane — the data gradient's relu / dropout mask reads
// "hi > 0" (only values below 2^-39 of the row maximum round to zero at all).  High half = max(high half, u > 0) as ONE
// packed unsigned maximum: a positive value rounds to +0 at worst, positive fp16 order like their bit patterns, and a
// negative half (sign bit set) is above 1 as an unsigned number, so it stays what it is.
template <bool KEEP_POSITIVE>
__device__ __forceinline__ void pl_split2(float u0, float u1, uint32_t& hi, uint32_t& lo) {
  const f32x2 uu = {u0, u1};
  h16x2 hh = __builtin_convertvector(uu, h16x2);                 // v_cvt_pk_f16_f32 (RNE)
  uint32_t hb = __builtin_bit_cast(uint32_t, hh);
  if constexpr (KEEP_POSITIVE) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const uint32_t nz = (u0 > 0.f ? 1u : 0u) | (u1 > 0.f ? 0x10000u : 0u);
    const u16x2 mxv = __builtin_elementwise_max(__builtin_bit_cast(u16x2, hb), __builtin_bit_cast(u16x2, nz));
    hb = __builtin_bit_cast(uint32_t, mxv);
    hh = __builtin_bit_cast(h16x2, hb);
  }
  const f32x2 rr = {u0 - static_cast<float>(hh[0]), u1 - static_cast<float>(hh[1])};
  hi = hb;
  lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(rr, h16x2));
}

// element j (0..15) of the row piece at p, of a row with exponent s, as fp32: (hi + lo) 2^-s
__device__ __forceinline__ float pl_decode(const char* p, int j, int s) {
  const _Float16* e = reinterpret_cast<const _Float16*>(p);
  return (static_cast<float>(e[j]) + static_cast<float>(e[PL_LO / 2 + j])) * pl_pow2(-s);
}

namespace mi {

// a planes buffer of `rows` rows: data and exponents given, data 16-byte aligned, blk_stride >= rows * PL_ROWB and a
// multiple of PL_ROWB
inline bool planes_ok(const mi_planes_t* p, int64_t rows) {
  return p && p->data && p->row_exp && aligned16(p->data) && p->blk_stride >= rows * PL_ROWB && (p->blk_stride & 63) == 0 &&
         rows >= 0;
}

}  // namespace mi
