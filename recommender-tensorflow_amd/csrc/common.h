// Shared host-side helpers for the C-ABI translation units (error text, argument checks,
// launch checks).  gfx950 only: wave = 64 lanes everywhere in this directory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include "../../include/mi355x_rec.h"

namespace mi {

constexpr int kWave = 64;

void set_error(const char* fmt, ...);
// the error text of a legal request that is not built; returns MI_ERR_UNSUPPORTED
int32_t unsupported(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// a group entry's refusal of its member i: the last error becomes "<entry>: member <i>: <the last error>"
void member_error(const char* entry, int i);
// a plan's member table from the host to the device, complete on return (who: the entry, for "<who>: copying the member
// table: ..." and MI_ERR_LAUNCH)
int32_t upload_table(void* device, const void* host, size_t bytes, mi_stream_t stream, const char* who);

inline hipStream_t as_stream(mi_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Tuning switches (MI_PL_TILE, MI_WGRAD_PL, MI_WGRAD_MIN_KSTEPS, MI_CATCHUP_BLOCKS, MI_SORT_FUSED, MI_SORT_BITS = the digit
// width of the fused per-field sort, 1..9, built-in 7; MI_SORT_NAP, MI_AUC_SORT_BITS = 1..9, built-in 9): read from the
// environment ONLY in the tools' build of the library (`make tuning` -> tools/probe/libmi355x_rec_tuning.so, -DMI_TUNING; the
// tools/*_bench.py scripts load that file).  The shipped libmi355x_rec.so has no environment switch: env_int is the
// built-in value.  Every switch tunes or chooses between shipped paths: a variant that lost its A/B is deleted, not kept
// behind one.
#ifdef MI_TUNING
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}
#else
constexpr int env_int(const char*, int dflt) { return dflt; }
#endif

// device-resident step state registered by mi_set_step_state (host_ids.cpp), or nullptr
const mi_step_state_t* step_state();

}  // namespace mi

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// *from to *to, word by word, by the kThreads threads of a workgroup: a member's arguments out of a group plan's device table
template <int kThreads, typename T>
__device__ __forceinline__ void mi_copy_words(T* to, const T* from) {
  static_assert(sizeof(T) % 4 == 0, "copied word by word");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(from);
  uint32_t* dst = reinterpret_cast<uint32_t*>(to);
  for (int i = threadIdx.x; i < static_cast<int>(sizeof(T) / sizeof(uint32_t)); i += kThreads) dst[i] = src[i];
}

template <int N> __device__ __forceinline__ void mi_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// A workgroup's abs-max mx (>= 0) into its slot of an abs-max vector (MI_AMAX_SLOTS floats, value = largest entry), by
// one thread: an atomic max on the bit pattern, spread over the slots, and only when the slot does not already hold a
// larger value — same-address atomics serialise at ~0.2 us each, and a kernel's first generation of workgroups ends together.
__device__ __forceinline__ void mi_amax_slot_max(float* vec, float mx) {
  unsigned int* slot = reinterpret_cast<unsigned int*>(vec) + (blockIdx.x & (MI_AMAX_SLOTS - 1));
  const unsigned int bits = __float_as_uint(mx);
  if (bits > *reinterpret_cast<volatile unsigned int*>(slot)) atomicMax(slot, bits);
}

// The same from every thread of the workgroup (it contains a barrier), each with its own mx.
__device__ __forceinline__ void mi_amax_publish(float* __restrict__ vec, float mx) {
  __shared__ float part[16];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w) mx = fmaxf(mx, part[w]);
    mi_amax_slot_max(vec, mx);
  }
}

// ---- the sigmoid cross-entropy head (binary_classification_head, deep_fm.py:118-125) ----------------------------------
// The unfused head (head.hip) and the fused tails (tail.hip, gemm_pl.hip's PL_TOP epilogue) are tested to give the same bits.
__device__ __forceinline__ float mi_sigmoid_stable(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// the loss of logit z for label y (0 or 1), unscaled: max(z, 0) - z y + log1p(exp(-|z|))
__device__ __forceinline__ float mi_sigmoid_ce_loss(float z, float y) { return fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z))); }
// its gradient d loss / d z, scaled
__device__ __forceinline__ float mi_sigmoid_ce_grad(float z, float y, float scale) { return (mi_sigmoid_stable(z) - y) * scale; }

// ---- activation of tf.layers.dense (deep_fm.py:22,100: params["activation"], default tf.nn.relu) -----------------------
// kind: 0 none, 1 relu, 2 sigmoid, 3 tanh; and its derivative expressed through the activation's OUTPUT y (what the forward
// stored).  The training step, predict_logits and top-K scoring all use these.
__device__ __forceinline__ float mi_act(int kind, float v) {
  switch (kind) {
    case 1: return fmaxf(v, 0.f);
    case 2: return 1.f / (1.f + __expf(-v));
    case 3: return tanhf(v);
    default: return v;
  }
}
__device__ __forceinline__ float mi_act_deriv_from_output(int kind, float y) {
  switch (kind) {
    case 1: return y > 0.f ? 1.f : 0.f;
    case 2: return y * (1.f - y);
    case 3: return 1.f - y * y;
    default: return 1.f;
  }
}

// ---- dropout mask (tf.layers.dropout, deep_fm.py:102-103): counter-based keep decisions, TWO per 32-bit hash --------
// Element (row, col) of a layer's output is kept iff its 16 bits of hash(row, col >> 1) — the low half for an even
// column, the high half for an odd one — are below keep_prob * 2^16.  The per-ROW key goes through a multiply-xorshift
// mixer (two v_mul_lo_u32, quarter rate on CDNA: paid once per row and lane); the per-PAIR mixer is a
// shift-add-xor chain in the manner of Thomas Wang's 32-bit integer hash, shifts, adds and xors only (round 2's mask paid 3.5 quarter-rate multiplies per
// ELEMENT: ~25 % of a GEMM epilogue).  tests/util.py replays the mask on the host, every kernel here uses these.
__device__ __forceinline__ uint32_t mi_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
constexpr uint32_t MI_DROP_PAIR_MUL = 0x85EBCA77U;
__device__ __forceinline__ uint32_t mi_drop_rowkey(uint64_t seed, uint32_t row) {
  const uint32_t s = static_cast<uint32_t>(seed) ^ (static_cast<uint32_t>(seed >> 32) * 0xC2B2AE35U);
  return mi_mix32((row * 0x9E3779B1U) ^ s);
}
// pair_term = (col >> 1) * MI_DROP_PAIR_MUL (callers with compile-time column offsets fold the multiply into constants)
__device__ __forceinline__ uint32_t mi_drop_pairhash(uint32_t rowkey, uint32_t pair_term) {
  // (every line below is one or two full-rate instructions — v_lshl_add_u32 / v_lshrrev + v_xor; no step is a sum of two
  // shifted copies, which hipcc would turn back into a quarter-rate v_mul_lo_u32)
  uint32_t x = rowkey + pair_term;
  x = ~x + (x << 15);
  x ^= x >> 12;
  x += x << 2;
  x ^= x >> 4;
  x += x << 3;
  x ^= x >> 11;
  x += x << 11;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t mi_drop_thresh16(float keep_prob) { return static_cast<uint32_t>(keep_prob * 65536.0f); }
__device__ __forceinline__ bool mi_drop_keep(uint32_t pairhash, uint32_t col, uint32_t thresh16) {
  return ((col & 1u) ? (pairhash >> 16) : (pairhash & 0xffffu)) < thresh16;
}
__device__ __forceinline__ bool mi_drop_keep_at(uint64_t seed, uint32_t row, uint32_t col, uint32_t thresh16) {
  return mi_drop_keep(mi_drop_pairhash(mi_drop_rowkey(seed, row), (col >> 1) * MI_DROP_PAIR_MUL), col, thresh16);
}

// ---- x / d for a divisor d known on the host (tf.nn.dropout: div(x, keep_prob)) ----------------------------------------
// Markstein's short division: with r = RN(1 / d) (computed on the host with IEEE division), q = RN(x r) is within an ulp of
// the quotient, the residual e = x - d q is exact in one fma, and RN(q + e r) is the correctly rounded x / d — the bits of
// the '/' operator — in 3 instructions instead of hipcc's ~12 (v_div_scale x2, v_rcp, 4 fma, v_div_fmas, v_div_fixup).
// Not taken on trust: mi_selftest_div compares the two on the device for EVERY fp32 x (tests: 0 mismatches for
// |x| >= 2^-100, where the residual of a quotient is still exactly representable; below that — values of 1e-30 — the last
// bit of the quotient can differ).  d = 1 gives x back exactly.
__device__ __forceinline__ float mi_div_const(float x, float d, float r) {
  const float q = x * r;
  const float e = fmaf(-d, q, x);
  return fmaf(e, r, q);
}

#define MI_REQUIRE(cond, ...)            \
  do {                                   \
    if (!(cond)) {                       \
      mi::set_error(__VA_ARGS__);        \
      return MI_ERR_INVALID;             \
    }                                    \
  } while (0)

#define MI_CHECK_LAUNCH(what)                                                   \
  do {                                                                          \
    hipError_t e__ = hipGetLastError();                                         \
    if (e__ != hipSuccess) {                                                    \
      mi::set_error("%s: launch failed: %s", what, hipGetErrorString(e__));     \
      return MI_ERR_LAUNCH;                                                     \
    }                                                                           \
  } while (0)

namespace mi {

// dynamic LDS above 64 KB has to be asked for, per kernel
template <typename K>
int32_t raise_lds(K* kernel, size_t lds, const char* who) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    MI_REQUIRE(e == hipSuccess, "%s: LDS of %zu bytes: %s", who, lds, hipGetErrorString(e));
  }
  return MI_OK;
}

}  // namespace mi
