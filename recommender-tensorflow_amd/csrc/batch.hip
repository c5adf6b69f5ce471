// One training batch out of a dataset that lives on the device (mi_batch_gather, include/mi355x_rec.h): the rows an index
// stream names — ids int32 [B, F], numeric features float [B, n_num], labels uint8 [B] — are copied out of the resident
// arrays in ONE launch.  The layer above it is mi355x_rec/dataset.py.
//
// Shape of the kernel: a workgroup takes tiles of kRows consecutive OUTPUT rows.  A tile of a dense [B, w] output is one
// contiguous run of kRows * w dwords, and lane t of the workgroup stores dwords t, t + 256, t + 512, ... of it: every store
// instruction of a wave covers 256 contiguous bytes, and the loads of one output row are one contiguous segment of its
// source row.  The (row, column) of a lane's dword is never divided out per element: the lane divides its own number once
// a tile (32 bits, the lane number is below 256) and then steps by (256 / w, 256 % w), which the host worked out.  A bad
// index never becomes an address: its row is read from row 0 and stored as zeros.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 32;          // output rows a tile
constexpr int kUnroll = 4;         // dwords a lane has in flight
constexpr int kMaxBlocks = 2048;   // a grid of at most this many workgroups strides over the tiles

struct BatchArgs {
  const int32_t* ids_all;
  const float* x_all;
  const uint8_t* y_all;
  const int32_t* order;
  int32_t* ids;
  float* x;
  uint8_t* y;
  int32_t* status;
  int64_t ld_ids, ld_x, N, B;
  uint32_t F, n_num;
  uint32_t ids_dq, ids_dr, x_dq, x_dr;   // kThreads / width and kThreads % width of the two planes
};

// rows `order[0 .. rows)` of src [N, ld] into the dense tile dst [rows, w]; kCount: this plane reports the bad indices.
// A lane's dwords are taken kUnroll at a time — their positions first, then every index, then every value, then the stores —
// so that a tile costs two round trips to memory a group and not two a dword (the kernel is a chain of dependent loads:
// order[r], then the row).  Every load is unconditional and in range: a position past the tile reads order[0], a bad
// index row 0; only the stores are predicated.
template <bool kCount, typename T>
__device__ __forceinline__ void gather_tile(const T* __restrict__ src, int64_t ld, uint32_t w, uint32_t dq, uint32_t dr,
                                            const int32_t* __restrict__ order, int64_t N, uint32_t rows, int64_t row0,
                                            T* __restrict__ dst, int32_t* status) {
  uint32_t r = threadIdx.x / w, c = threadIdx.x - r * w;
  while (r < rows) {
    uint32_t rr[kUnroll], cc[kUnroll];
    int32_t idx[kUnroll];
    T v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      rr[u] = r;
      cc[u] = c;
      r += dq;
      c += dr;
      if (c >= w) {
        c -= w;
        ++r;
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) idx[u] = order[rr[u] < rows ? rr[u] : 0];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const bool ok = idx[u] >= 0 && idx[u] < N;
      v[u] = src[static_cast<int64_t>(ok ? idx[u] : 0) * ld + cc[u]];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (rr[u] >= rows) continue;
      const bool ok = idx[u] >= 0 && idx[u] < N;
      dst[static_cast<int64_t>(rr[u]) * w + cc[u]] = ok ? v[u] : T(0);
      if (kCount && !ok && cc[u] == 0) {
        atomicAdd(status, 1);
        atomicMax(status + 1, static_cast<int32_t>(INT32_MAX - (row0 + rr[u])));
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void batch_gather_k(const BatchArgs a) {
  const int64_t tiles = (a.B + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    const uint32_t rows = static_cast<uint32_t>(a.B - row0 < kRows ? a.B - row0 : kRows);
    const int32_t* order = a.order + row0;
    gather_tile<true>(a.ids_all, a.ld_ids, a.F, a.ids_dq, a.ids_dr, order, a.N, rows, row0, a.ids + row0 * a.F, a.status);
    if (a.n_num)
      gather_tile<false>(a.x_all, a.ld_x, a.n_num, a.x_dq, a.x_dr, order, a.N, rows, row0, a.x + row0 * a.n_num, nullptr);
    if (a.y && threadIdx.x < rows) {
      const int32_t idx = order[threadIdx.x];
      const bool ok = idx >= 0 && idx < a.N;
      const uint8_t v = a.y_all[ok ? idx : 0];
      a.y[row0 + threadIdx.x] = ok ? v : uint8_t(0);
    }
  }
}

}  // namespace

extern "C" {

int32_t mi_batch_gather(const int32_t* ids_all, int64_t ld_ids, const float* x_all, int64_t ld_x, const uint8_t* y_all, int64_t N,
                        const int32_t* order, int64_t B, int32_t F, int32_t n_num, int32_t* ids, float* x, uint8_t* y,
                        int32_t* status, mi_stream_t stream) {
  MI_REQUIRE(ids_all != nullptr, "batch_gather: null ids_all");
  MI_REQUIRE(order != nullptr, "batch_gather: null order");
  MI_REQUIRE(ids != nullptr, "batch_gather: null ids");
  MI_REQUIRE(status != nullptr, "batch_gather: null status");
  MI_REQUIRE(N >= 1 && N <= INT32_MAX, "batch_gather: N=%lld (1 to 2^31 - 1)", (long long)N);
  MI_REQUIRE(B >= 1 && B <= INT32_MAX, "batch_gather: B=%lld (1 to 2^31 - 1)", (long long)B);
  MI_REQUIRE(F >= 1 && F <= MI_IDS_MAX_COLUMNS, "batch_gather: F=%d (1 to %d)", F, MI_IDS_MAX_COLUMNS);
  MI_REQUIRE(ld_ids >= F, "batch_gather: ld_ids=%lld < F=%d", (long long)ld_ids, F);
  MI_REQUIRE(n_num >= 0, "batch_gather: n_num=%d", n_num);
  if (n_num > 0) {
    MI_REQUIRE(x_all != nullptr, "batch_gather: null x_all with n_num=%d", n_num);
    MI_REQUIRE(x != nullptr, "batch_gather: null x with n_num=%d", n_num);
    MI_REQUIRE(ld_x >= n_num, "batch_gather: ld_x=%lld < n_num=%d", (long long)ld_x, n_num);
  }
  MI_REQUIRE((y_all == nullptr) == (y == nullptr), "batch_gather: %s is null and %s is not (labels: both or neither)",
             y_all ? "y" : "y_all", y_all ? "y_all" : "y");
  BatchArgs a{};
  a.ids_all = ids_all; a.x_all = x_all; a.y_all = y_all; a.order = order;
  a.ids = ids; a.x = x; a.y = y; a.status = status;
  a.ld_ids = ld_ids; a.ld_x = ld_x; a.N = N; a.B = B;
  a.F = static_cast<uint32_t>(F); a.n_num = static_cast<uint32_t>(n_num);
  a.ids_dq = kThreads / a.F; a.ids_dr = kThreads % a.F;
  if (n_num > 0) { a.x_dq = kThreads / a.n_num; a.x_dr = kThreads % a.n_num; }
  const int64_t tiles = mi::ceil_div(B, kRows);
  batch_gather_k<<<dim3(static_cast<unsigned>(tiles < kMaxBlocks ? tiles : kMaxBlocks)), dim3(kThreads), 0,
                   mi::as_stream(stream)>>>(a);
  MI_CHECK_LAUNCH("batch_gather_k");
  return MI_OK;
}

}  // extern "C"
