// Host-side entry points: library info, error text, and the categorical id transforms of
// trainers/ml_100k.py:19-35 (hash_bucket / bucketized columns).  Integer work only.
//
// Fingerprint64 is FarmHash's farmhashna::Hash64 (Google, MIT licence), restated in farmhash.h (shared
// with the device transforms of ids.hip) from the published algorithm: TensorFlow 1.12 (un-vendored dependency, environment.yml:10) calls it for
// tf.feature_column.categorical_column_with_hash_bucket.  The reference holds no vector for it;
// tests/test_fingerprint.py pins the 1-3 byte branch on TF's own string_to_hash_bucket test
// values and cross-checks every branch against the independent Python restatement in oracle/.
#include <string.h>

#include <string>

#include "common.h"
#include "farmhash.h"

static const mi_step_state_t* g_step_state = nullptr;

namespace mi {

const mi_step_state_t* step_state() { return g_step_state; }

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int32_t unsupported(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return MI_ERR_UNSUPPORTED;
}

void member_error(const char* entry, int i) {
  char why[sizeof(g_err)];
  snprintf(why, sizeof(why), "%s", g_err);
  set_error("%s: member %d: %s", entry, i, why);
}

int32_t upload_table(void* device, const void* host, size_t bytes, mi_stream_t stream, const char* who) {
  hipError_t e = hipMemcpyAsync(device, host, bytes, hipMemcpyHostToDevice, as_stream(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));           // (the caller frees the host table)
  if (e == hipSuccess) return MI_OK;
  set_error("%s: copying the member table: %s", who, hipGetErrorString(e));
  return MI_ERR_LAUNCH;
}

}  // namespace mi

extern "C" {

int32_t mi_set_step_state(const mi_step_state_t* device_state) {
  g_step_state = device_state;
  return MI_OK;
}

int32_t mi_abi_version(void) { return 21; }

const char* mi_last_error(void) { return mi::g_err; }

const char* mi_build_info(void) {
  static char info[128];
  snprintf(info, sizeof(info), "libmi355x_rec gfx950 HIP %d.%d.%d", HIP_VERSION_MAJOR,
           HIP_VERSION_MINOR, HIP_VERSION_PATCH);
  return info;
}

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) — the checksum of TensorFlow's tensor-bundle checkpoint files
// (block trailers of the .index table, one per tensor in the .data shards; conf_utils.py:6-10 configures the Estimator
// that writes them).  Slicing-by-8 tables, built on first use; `crc` is the running value (0 to start), unmasked.
uint32_t mi_crc32c(const void* data, size_t len, uint32_t crc) {
  static uint32_t T[8][256];
  static bool ready = false;
  if (!ready) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
      T[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xffu];
    ready = true;
  }
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint32_t c = ~crc;
  while (len && (reinterpret_cast<uintptr_t>(p) & 7u)) { c = (c >> 8) ^ T[0][(c ^ *p++) & 0xffu]; --len; }
  while (len >= 8) {
    uint64_t w;
    memcpy(&w, p, 8);
    w ^= c;
    c = T[7][w & 0xff] ^ T[6][(w >> 8) & 0xff] ^ T[5][(w >> 16) & 0xff] ^ T[4][(w >> 24) & 0xff] ^
        T[3][(w >> 32) & 0xff] ^ T[2][(w >> 40) & 0xff] ^ T[1][(w >> 48) & 0xff] ^ T[0][(w >> 56) & 0xff];
    p += 8; len -= 8;
  }
  while (len--) c = (c >> 8) ^ T[0][(c ^ *p++) & 0xffu];
  return ~c;
}

uint64_t mi_fingerprint64(const void* data, size_t len) {
  return mi::farm::hash64(static_cast<const uint8_t*>(data), len);
}

int32_t mi_hash_bucket_i64(const int64_t* values, int64_t n, int64_t num_buckets,
                           int32_t* out_ids) {
  MI_REQUIRE(n >= 0 && num_buckets > 0 && num_buckets <= INT32_MAX, "hash_bucket_i64: n=%lld buckets=%lld",
             (long long)n, (long long)num_buckets);
  MI_REQUIRE(n == 0 || (values && out_ids), "hash_bucket_i64: null buffer");
  char buf[32];
  for (int64_t i = 0; i < n; ++i) {
    // tf.as_string on an integer tensor: plain decimal, '-' for negatives
    int len = snprintf(buf, sizeof(buf), "%lld", (long long)values[i]);
    out_ids[i] = static_cast<int32_t>(mi_fingerprint64(buf, (size_t)len) % (uint64_t)num_buckets);
  }
  return MI_OK;
}

int32_t mi_hash_bucket_bytes(const uint8_t* bytes, const int64_t* offsets, int64_t n,
                             int64_t num_buckets, int32_t* out_ids) {
  MI_REQUIRE(n >= 0 && num_buckets > 0 && num_buckets <= INT32_MAX, "hash_bucket_bytes: n=%lld buckets=%lld",
             (long long)n, (long long)num_buckets);
  MI_REQUIRE(n == 0 || (offsets && out_ids), "hash_bucket_bytes: null buffer");
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo = offsets[i], hi = offsets[i + 1];
    MI_REQUIRE(hi >= lo && lo >= 0, "hash_bucket_bytes: offsets not monotone at %lld", (long long)i);
    out_ids[i] = static_cast<int32_t>(mi_fingerprint64(bytes + lo, (size_t)(hi - lo)) %
                                      (uint64_t)num_buckets);
  }
  return MI_OK;
}

int32_t mi_bucketize_f32(const float* values, int64_t n, const float* boundaries,
                         int32_t num_boundaries, int32_t* out_ids) {
  MI_REQUIRE(n >= 0 && num_boundaries >= 0, "bucketize: n=%lld nb=%d", (long long)n, num_boundaries);
  MI_REQUIRE(n == 0 || (values && out_ids), "bucketize: null buffer");
  for (int32_t j = 1; j < num_boundaries; ++j)
    MI_REQUIRE(boundaries[j] > boundaries[j - 1], "bucketize: boundaries must be strictly increasing");
  for (int64_t i = 0; i < n; ++i) {
    // std::upper_bound: number of boundaries <= x
    int32_t lo = 0, hi = num_boundaries;
    const float x = values[i];
    while (lo < hi) {
      int32_t mid = (lo + hi) >> 1;
      if (boundaries[mid] <= x) lo = mid + 1; else hi = mid;
    }
    out_ids[i] = lo;
  }
  return MI_OK;
}

}  // extern "C"
