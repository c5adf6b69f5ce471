// FarmHash Fingerprint64 (farmhashna::Hash64, Google, MIT licence), restated from the published algorithm, ONCE for the
// host entries (host_ids.cpp) and the device id transforms (ids.hip): TensorFlow 1.12 calls it for
// tf.feature_column.categorical_column_with_hash_bucket (trainers/ml_100k.py:19-35).  Every fetch lies inside
// [s, s + len): no byte outside the string's own range is read.  The fetches are unaligned: a memcpy, which hipcc
// turns into one load where the target takes unaligned addresses.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define MI_HD __host__ __device__

namespace mi {
namespace farm {

constexpr uint64_t k0 = 0xc3a5c85c97cb3127ULL;
constexpr uint64_t k1 = 0xb492b66fbe98f273ULL;
constexpr uint64_t k2 = 0x9ae16a3b2f90404fULL;

MI_HD inline uint64_t fetch64(const uint8_t* p) {
  uint64_t r;
  __builtin_memcpy(&r, p, 8);  // little-endian on the host (x86-64) and on the device
  return r;
}
MI_HD inline uint32_t fetch32(const uint8_t* p) {
  uint32_t r;
  __builtin_memcpy(&r, p, 4);
  return r;
}
MI_HD inline uint64_t rot(uint64_t v, int s) { return s == 0 ? v : ((v >> s) | (v << (64 - s))); }
MI_HD inline uint64_t shift_mix(uint64_t v) { return v ^ (v >> 47); }

MI_HD inline uint64_t hash_len16(uint64_t u, uint64_t v, uint64_t mul) {
  uint64_t a = (u ^ v) * mul;
  a ^= (a >> 47);
  uint64_t b = (v ^ a) * mul;
  b ^= (b >> 47);
  b *= mul;
  return b;
}

MI_HD inline uint64_t hash_0to16(const uint8_t* s, size_t len) {
  if (len >= 8) {
    uint64_t mul = k2 + len * 2;
    uint64_t a = fetch64(s) + k2;
    uint64_t b = fetch64(s + len - 8);
    uint64_t c = rot(b, 37) * mul + a;
    uint64_t d = (rot(a, 25) + b) * mul;
    return hash_len16(c, d, mul);
  }
  if (len >= 4) {
    uint64_t mul = k2 + len * 2;
    uint64_t a = fetch32(s);
    return hash_len16(len + (a << 3), fetch32(s + len - 4), mul);
  }
  if (len > 0) {
    uint8_t a = s[0], b = s[len >> 1], c = s[len - 1];
    uint32_t y = static_cast<uint32_t>(a) + (static_cast<uint32_t>(b) << 8);
    uint32_t z = static_cast<uint32_t>(len) + (static_cast<uint32_t>(c) << 2);
    return shift_mix(y * k2 ^ z * k0) * k2;
  }
  return k2;
}

MI_HD inline uint64_t hash_17to32(const uint8_t* s, size_t len) {
  uint64_t mul = k2 + len * 2;
  uint64_t a = fetch64(s) * k1;
  uint64_t b = fetch64(s + 8);
  uint64_t c = fetch64(s + len - 8) * mul;
  uint64_t d = fetch64(s + len - 16) * k2;
  return hash_len16(rot(a + b, 43) + rot(c, 30) + d, a + rot(b + k2, 18) + c, mul);
}

MI_HD inline uint64_t hash_33to64(const uint8_t* s, size_t len) {
  uint64_t mul = k2 + len * 2;
  uint64_t a = fetch64(s) * k2;
  uint64_t b = fetch64(s + 8);
  uint64_t c = fetch64(s + len - 8) * mul;
  uint64_t d = fetch64(s + len - 16) * k2;
  uint64_t y = rot(a + b, 43) + rot(c, 30) + d;
  uint64_t z = hash_len16(y, a + rot(b + k2, 18) + c, mul);
  uint64_t e = fetch64(s + 16) * mul;
  uint64_t f = fetch64(s + 24);
  uint64_t g = (y + fetch64(s + len - 32)) * mul;
  uint64_t h = (z + fetch64(s + len - 24)) * mul;
  return hash_len16(rot(e + f, 43) + rot(g, 30) + h, e + rot(f + a, 18) + g, mul);
}

struct u128 {
  uint64_t first, second;
};

MI_HD inline u128 weak32(uint64_t w, uint64_t x, uint64_t y, uint64_t z, uint64_t a, uint64_t b) {
  a += w;
  b = rot(b + a + z, 21);
  uint64_t c = a;
  a += x;
  a += y;
  b += rot(a, 44);
  return {a + z, b + c};
}
MI_HD inline u128 weak32(const uint8_t* s, uint64_t a, uint64_t b) {
  return weak32(fetch64(s), fetch64(s + 8), fetch64(s + 16), fetch64(s + 24), a, b);
}

MI_HD inline uint64_t hash64(const uint8_t* s, size_t len) {
  if (len <= 16) return hash_0to16(s, len);
  if (len <= 32) return hash_17to32(s, len);
  if (len <= 64) return hash_33to64(s, len);
  const uint64_t seed = 81;
  uint64_t x = seed;
  uint64_t y = seed * k1 + 113;
  uint64_t z = shift_mix(y * k2 + 113) * k2;
  u128 v{0, 0}, w{0, 0};
  x = x * k2 + fetch64(s);
  const uint8_t* end = s + ((len - 1) / 64) * 64;
  const uint8_t* last64 = end + ((len - 1) & 63) - 63;
  do {
    x = rot(x + y + v.first + fetch64(s + 8), 37) * k1;
    y = rot(y + v.second + fetch64(s + 48), 42) * k1;
    x ^= w.second;
    y += v.first + fetch64(s + 40);
    z = rot(z + w.first, 33) * k1;
    v = weak32(s, v.second * k1, x + w.first);
    w = weak32(s + 32, z + w.second, y + fetch64(s + 16));
    uint64_t t = z;
    z = x;
    x = t;
    s += 64;
  } while (s != end);
  uint64_t mul = k1 + ((z & 0xff) << 1);
  s = last64;
  w.first += ((len - 1) & 63);
  v.first += w.first;
  w.first += v.first;
  x = rot(x + y + v.first + fetch64(s + 8), 37) * mul;
  y = rot(y + v.second + fetch64(s + 48), 42) * mul;
  x ^= w.second * 9;
  y += v.first * 9 + fetch64(s + 40);
  z = rot(z + w.first, 33) * mul;
  v = weak32(s, v.second * mul, x + w.first);
  w = weak32(s + 32, z + w.second, y + fetch64(s + 16));
  uint64_t t = z;
  z = x;
  x = t;
  return hash_len16(hash_len16(v.first, w.first, mul) + shift_mix(y) * k0 + z,
                    hash_len16(v.second, w.second, mul) + x, mul);
}

}  // namespace farm
}  // namespace mi
