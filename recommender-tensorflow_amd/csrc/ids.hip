// The categorical id transforms on the device: F raw feature columns of B values become the id matrix [B, ld] in ONE
// launch (mi_ids_transform), and the raw fingerprints of a column of strings (mi_fingerprint64_device).  The device form
// of host_ids.cpp's entries, which stand for the column constructors of trainers/ml_100k.py:19-35 (hash_bucket, bucketized,
// vocabulary_list, identity).  Integer work only, held to equality with the host definitions.
//
// Shape of the kernel: grid (ceil(B / 256), F).  The column is blockIdx.y, so its descriptor — an element of the table that
// travels in the kernel's arguments — is read with scalar loads and the switch on its kind is uniform: no lane of a
// workgroup takes another branch.  One lane transforms one value.  The decimal text of an integer (at most 20 characters)
// is built and hashed in three packed 64-bit words, never in a byte array indexed at run time (which would live in
// scratch memory); strings are hashed where they lie, every fetch inside the string's own range (farmhash.h).
#include "common.h"
#include "farmhash.h"

namespace {

constexpr int kThreads = 256;

struct IdsArgs {
  mi_ids_column_t col[MI_IDS_MAX_COLUMNS];
  int32_t* ids;
  int32_t* status;
  int64_t B, ld;
};
static_assert(sizeof(IdsArgs) <= 4096, "the column table has to fit the kernel's arguments");

// ---- an integer's decimal text in packed words: character p is byte p & 7 of word p >> 3 -------------------------------
struct Text {
  uint64_t w0, w1, w2;
  int len;
};

MI_HD inline void push_front(Text& t, uint32_t ch) {
  t.w2 = (t.w2 << 8) | (t.w1 >> 56);
  t.w1 = (t.w1 << 8) | (t.w0 >> 56);
  t.w0 = (t.w0 << 8) | ch;
  ++t.len;
}

// what "%lld" prints: the digits from the last to the first, each pushed in front of the text so far, then the sign
MI_HD inline Text decimal_text(int64_t v) {
  Text t{0, 0, 0, 0};
  const bool neg = v < 0;
  uint64_t m = neg ? 0ull - static_cast<uint64_t>(v) : static_cast<uint64_t>(v);
  while (m >> 32) {                                  // (a 64-bit division by 10 is a dozen instructions: only while needed)
    const uint64_t q = m / 10u;
    push_front(t, '0' + static_cast<uint32_t>(m - q * 10u));
    m = q;
  }
  uint32_t s = static_cast<uint32_t>(m);
  do {
    const uint32_t q = s / 10u;
    push_front(t, '0' + (s - q * 10u));
    s = q;
  } while (s);
  if (neg) push_front(t, '-');
  return t;
}

// the 8 bytes from character `off` on (off in [0, 16]); bytes past the text read as what the words hold there
MI_HD inline uint64_t text_fetch64(const Text& t, int off) {
  const int q = off >> 3, r = (off & 7) * 8;
  const uint64_t lo = q == 0 ? t.w0 : (q == 1 ? t.w1 : t.w2);
  const uint64_t hi = q == 0 ? t.w1 : (q == 1 ? t.w2 : 0ull);
  return r ? ((lo >> r) | (hi << (64 - r))) : lo;
}

// farmhashna::Hash64 of a text of 1 to 20 characters: the branches of farmhash.h's hash_0to16 and hash_17to32
MI_HD inline uint64_t text_fingerprint(const Text& t) {
  using namespace mi::farm;
  const uint64_t len = static_cast<uint64_t>(t.len);
  if (t.len > 16) {
    const uint64_t mul = k2 + len * 2;
    const uint64_t a = t.w0 * k1;
    const uint64_t b = t.w1;
    const uint64_t c = text_fetch64(t, t.len - 8) * mul;
    const uint64_t d = text_fetch64(t, t.len - 16) * k2;
    return hash_len16(rot(a + b, 43) + rot(c, 30) + d, a + rot(b + k2, 18) + c, mul);
  }
  if (t.len >= 8) {
    const uint64_t mul = k2 + len * 2;
    const uint64_t a = t.w0 + k2;
    const uint64_t b = text_fetch64(t, t.len - 8);
    const uint64_t c = rot(b, 37) * mul + a;
    const uint64_t d = (rot(a, 25) + b) * mul;
    return hash_len16(c, d, mul);
  }
  if (t.len >= 4) {
    const uint64_t mul = k2 + len * 2;
    const uint64_t a = t.w0 & 0xffffffffull;
    const uint64_t b = (t.w0 >> ((t.len - 4) * 8)) & 0xffffffffull;
    return hash_len16(len + (a << 3), b, mul);
  }
  const uint32_t a = static_cast<uint32_t>(t.w0 & 0xff);
  const uint32_t b = static_cast<uint32_t>((t.w0 >> ((t.len >> 1) * 8)) & 0xff);
  const uint32_t c = static_cast<uint32_t>((t.w0 >> ((t.len - 1) * 8)) & 0xff);
  const uint32_t y = a + (b << 8);
  const uint32_t z = static_cast<uint32_t>(t.len) + (c << 2);
  return shift_mix(y * k2 ^ z * k0) * k2;
}

// h mod n for n in [1, 2^31 - 1]: the compiler's 64-bit integer remainder — exact for every h
MI_HD inline int64_t bucket_of(uint64_t h, int32_t n) { return static_cast<int64_t>(h % static_cast<uint64_t>(n)); }

MI_HD inline bool same_bytes(const uint8_t* a, const uint8_t* b, int64_t n) {
  int64_t i = 0;
  for (; i + 8 <= n; i += 8)
    if (mi::farm::fetch64(a + i) != mi::farm::fetch64(b + i)) return false;
  for (; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// the id of one string of a vocabulary_list column, or -1 ... default_value as the host gives them
MI_HD inline int64_t vocabulary_id(const mi_ids_column_t& c, const uint8_t* s, int64_t len) {
  const int32_t n = c.n_table;
  const uint64_t* fp = static_cast<const uint64_t*>(c.table);
  const int64_t* start = reinterpret_cast<const int64_t*>(fp + n);
  const int32_t* index = reinterpret_cast<const int32_t*>(start + n + 1);
  const uint8_t* text = reinterpret_cast<const uint8_t*>(index + n + (n & 1));
  const uint64_t h = mi::farm::hash64(s, static_cast<size_t>(len));
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (fp[mid] < h) lo = mid + 1; else hi = mid;
  }
  for (; lo < n && fp[lo] == h; ++lo) {
    const int64_t a = start[lo];
    if (start[lo + 1] - a == len && same_bytes(text + a, s, len)) return index[lo];
  }
  return c.num_oov > 0 ? n + bucket_of(h, c.num_oov) : c.default_value;
}

MI_HD inline int64_t identity_id(const mi_ids_column_t& c, int64_t v) {
  return (v >= 0 && v < c.num_buckets) ? v : c.default_value;
}

__global__ __launch_bounds__(kThreads) void ids_transform_k(const IdsArgs a) {
  const int f = blockIdx.y;
  const mi_ids_column_t& c = a.col[f];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= a.B) return;
  int64_t id = -1;
  switch (c.kind) {
    case MI_IDS_HASH_I64:
      id = bucket_of(text_fingerprint(decimal_text(static_cast<const int64_t*>(c.values)[i])), c.num_buckets);
      break;
    case MI_IDS_HASH_I32:
      id = bucket_of(text_fingerprint(decimal_text(static_cast<const int32_t*>(c.values)[i])), c.num_buckets);
      break;
    case MI_IDS_HASH_BYTES:
    case MI_IDS_VOCAB_BYTES: {
      const int64_t lo = c.offsets[i], hi = c.offsets[i + 1];
      if (lo >= 0 && hi >= lo) {
        const uint8_t* s = static_cast<const uint8_t*>(c.values) + lo;
        id = c.kind == MI_IDS_HASH_BYTES ? bucket_of(mi::farm::hash64(s, static_cast<size_t>(hi - lo)), c.num_buckets)
                                         : vocabulary_id(c, s, hi - lo);
      }
      break;
    }
    case MI_IDS_BUCKETIZE_F32: {
      // std::upper_bound, the host's loop: the number of boundaries <= x (a NaN compares false: 0)
      const float* bd = static_cast<const float*>(c.table);
      const float x = static_cast<const float*>(c.values)[i];
      int32_t lo = 0, hi = c.n_table;
      while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (bd[mid] <= x) lo = mid + 1; else hi = mid;
      }
      id = lo;
      break;
    }
    case MI_IDS_IDENTITY_I64:
      id = identity_id(c, static_cast<const int64_t*>(c.values)[i]);
      break;
    case MI_IDS_IDENTITY_I32:
      id = identity_id(c, static_cast<const int32_t*>(c.values)[i]);
      break;
    default:
      break;
  }
  if (id < 0 || id >= c.num_buckets) {
    // a bad value: the kernels downstream index the table unchecked, so row 0 is stored and the host is told
    id = 0;
    atomicAdd(a.status + 2 * f, 1);
    atomicMax(a.status + 2 * f + 1, static_cast<int32_t>(INT32_MAX - i));
  }
  a.ids[i * a.ld + f] = static_cast<int32_t>(id);
}

__global__ __launch_bounds__(kThreads) void fingerprint64_k(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                            int64_t n, uint64_t* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t lo = offsets[i], hi = offsets[i + 1];
  const bool ok = lo >= 0 && hi >= lo;
  out[i] = mi::farm::hash64(bytes + (ok ? lo : 0), static_cast<size_t>(ok ? hi - lo : 0));
}

int32_t check_column(const mi_ids_column_t& c, int f) {
  const bool bytes_kind = c.kind == MI_IDS_HASH_BYTES || c.kind == MI_IDS_VOCAB_BYTES;
  MI_REQUIRE(c.kind >= MI_IDS_HASH_I64 && c.kind <= MI_IDS_IDENTITY_I32, "ids_transform: column %d: unknown kind %d", f, c.kind);
  MI_REQUIRE(c.values != nullptr, "ids_transform: column %d: null values", f);
  MI_REQUIRE(!bytes_kind || c.offsets != nullptr, "ids_transform: column %d: null offsets", f);
  MI_REQUIRE(c.num_buckets >= 1 && c.num_buckets <= INT32_MAX, "ids_transform: column %d: num_buckets=%d (1 to 2^31 - 1)", f,
             c.num_buckets);
  MI_REQUIRE(c.n_table >= 0, "ids_transform: column %d: n_table=%d", f, c.n_table);
  if (c.kind == MI_IDS_BUCKETIZE_F32) {
    MI_REQUIRE(c.n_table == 0 || (c.table && c.table_host), "ids_transform: column %d: null boundaries", f);
    MI_REQUIRE(c.n_table < c.num_buckets, "ids_transform: column %d: %d boundaries make %d buckets, num_buckets=%d", f, c.n_table,
               c.n_table + 1, c.num_buckets);
    for (int32_t j = 1; j < c.n_table; ++j)
      MI_REQUIRE(c.table_host[j] > c.table_host[j - 1], "ids_transform: column %d: boundaries must be strictly increasing", f);
  }
  if (c.kind == MI_IDS_VOCAB_BYTES) {
    MI_REQUIRE(c.n_table >= 1 && c.table, "ids_transform: column %d: no vocabulary table (n_table=%d)", f, c.n_table);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(c.table) & 7u) == 0, "ids_transform: column %d: vocabulary table not 8-byte aligned", f);
    MI_REQUIRE(c.num_oov >= 0 && static_cast<int64_t>(c.n_table) + c.num_oov <= c.num_buckets,
               "ids_transform: column %d: %d entries + %d oov buckets, num_buckets=%d", f, c.n_table, c.num_oov, c.num_buckets);
  }
  return MI_OK;
}

}  // namespace

extern "C" {

int32_t mi_ids_transform(const mi_ids_column_t* columns, int32_t F, int64_t B, int32_t* ids, int64_t ld, int32_t* status,
                         mi_stream_t stream) {
  MI_REQUIRE(columns && ids && status, "ids_transform: null buffer");
  MI_REQUIRE(F >= 1 && F <= MI_IDS_MAX_COLUMNS, "ids_transform: F=%d columns (1 to %d in one call)", F, MI_IDS_MAX_COLUMNS);
  MI_REQUIRE(B >= 1 && B <= INT32_MAX, "ids_transform: B=%lld", (long long)B);
  MI_REQUIRE(ld >= F, "ids_transform: ld=%lld < F=%d", (long long)ld, F);
  IdsArgs a{};
  for (int32_t f = 0; f < F; ++f) {
    const int32_t rc = check_column(columns[f], f);
    if (rc != MI_OK) return rc;
    a.col[f] = columns[f];
  }
  a.ids = ids; a.status = status; a.B = B; a.ld = ld;
  ids_transform_k<<<dim3(static_cast<unsigned>(mi::ceil_div(B, kThreads)), static_cast<unsigned>(F)), dim3(kThreads), 0,
                    mi::as_stream(stream)>>>(a);
  MI_CHECK_LAUNCH("ids_transform_k");
  return MI_OK;
}

int32_t mi_fingerprint64_device(const uint8_t* bytes, const int64_t* offsets, int64_t n, uint64_t* out, mi_stream_t stream) {
  MI_REQUIRE(n >= 1 && n <= INT32_MAX, "fingerprint64_device: n=%lld", (long long)n);
  MI_REQUIRE(offsets && out, "fingerprint64_device: null buffer");
  fingerprint64_k<<<dim3(static_cast<unsigned>(mi::ceil_div(n, kThreads))), dim3(kThreads), 0, mi::as_stream(stream)>>>(bytes, offsets,
                                                                                                                        n, out);
  MI_CHECK_LAUNCH("fingerprint64_k");
  return MI_OK;
}

}  // extern "C"
