// The pieces every stable LSD radix sort of this directory is made of, each written once: sort.hip (int32 key + value: the
// rows sort, the two per-field forms) and auc_sort.hip (64-bit words) hold the kernels and decide what a tile reads, where
// its offsets come from and where a ranked key goes; how a tile counts, scans, ranks and compacts is here.  Device helpers
// and small key sources only: no kernel, no entry point.
//
// A tile is kTile = 4,096 keys of one 256-thread workgroup.  Counting kernels read it block-strided (round r: keys
// r * 256 + t); scattering kernels give wave w the keys [w * 1,024, (w + 1) * 1,024) (round r: 64 consecutive keys), so the
// tile order is wave order, then round order, then lane order — what makes the scatter stable.
#pragma once
#include <type_traits>

#include "common.h"

namespace radix {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kItems = 16;                 // keys per thread per tile
constexpr int kTile = kBlock * kItems;     // 4096
constexpr int kMaxBits = 9;                // digit width limit: 512 bins x 4 waves of running slots = 8 KB of LDS
constexpr int kMaxBins = 1 << kMaxBits;

// ---- LDS words of one wave, scans, sums ------------------------------------------------------------------------------------
// A wave's running slots (ranked_scatter) are LDS words that lanes of the SAME wave read and write in turn, with only
// wave barriers in between.  They go through wavefront-scope relaxed atomics on the LDS array itself: the compiler may then
// neither keep a slot in a register across the barrier nor reorder the accesses, and the address space stays known (ds_read /
// ds_write).  A volatile POINTER to the array loses the address space and compiles to flat loads / stores with sc0 sc1.
__device__ __forceinline__ int32_t lds_ld(int32_t* p) {
  return __hip_atomic_load((__attribute__((address_space(3))) int32_t*)(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void lds_st(int32_t* p, int32_t v) {
  __hip_atomic_store((__attribute__((address_space(3))) int32_t*)(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

// the sum of v over a 256-thread workgroup, in every thread (one barrier; red[kWaves] is free again after the next one)
__device__ __forceinline__ int block_sum(int v, int32_t* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// One workgroup of BLOCK threads scans a row of `count` values in chunks of BLOCK: store(i, the sum of load(j) for j < i
// plus carry, load(i)); returns carry + the row's sum.  Two barriers per chunk.
template <int BLOCK, typename I, typename Load, typename Store>
__device__ __forceinline__ int block_excl_scan_chunked(I count, int carry, Load&& load, Store&& store) {
  constexpr int NW = BLOCK / 64;
  __shared__ int32_t wsum[NW];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  for (I c0 = 0; c0 < count; c0 += BLOCK) {
    const I i = c0 + t;
    const int v = (i < count) ? load(i) : 0;
    const int incl = wave_incl_scan(v, lane);
    __syncthreads();                     // previous chunk's wsum fully consumed
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int pre = carry, tot = 0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      if (ww < w) pre += wsum[ww];
      tot += wsum[ww];
    }
    if (i < count) store(i, pre + incl - v, v);
    carry += tot;
  }
  return carry;
}

// N exclusive scans at once over the nbins <= kMaxBins digits, by the whole workgroup: thread t owns `per` consecutive
// digits.  get(b, c) fills the N counts of digit b, put(b, j, pre) receives their N exclusive sums (j: the digit's index
// among the thread's own).  One barrier inside; wsum[N * kWaves] is scratch; what put() writes needs the caller's barrier.
__device__ __forceinline__ int digits_per_thread(int nbins) { return nbins > kBlock ? nbins / kBlock : 1; }
template <int N, typename Get, typename Put>
__device__ __forceinline__ void digit_excl_scan(int nbins, int32_t* wsum, Get&& get, Put&& put) {
  constexpr int P = kMaxBins / kBlock;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int per = digits_per_thread(nbins);
  int c[P][N], pre[N];
#pragma unroll
  for (int k = 0; k < N; ++k) pre[k] = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int b = t * per + j;
#pragma unroll
    for (int k = 0; k < N; ++k) c[j][k] = 0;
    if (j < per && b < nbins) get(b, c[j]);
#pragma unroll
    for (int k = 0; k < N; ++k) pre[k] += c[j][k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int incl = wave_incl_scan(pre[k], lane);
    if (lane == 63) wsum[k * kWaves + w] = incl;
    pre[k] = incl - pre[k];
  }
  __syncthreads();
  for (int ww = 0; ww < w; ++ww)
#pragma unroll
    for (int k = 0; k < N; ++k) pre[k] += wsum[k * kWaves + ww];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int b = t * per + j;
    if (j < per && b < nbins) put(b, j, pre);
#pragma unroll
    for (int k = 0; k < N; ++k) pre[k] += c[j][k];
  }
}

// ---- keys ------------------------------------------------------------------------------------------------------------------
// A key source gives a tile its keys: at(i) is the key of position i.  Digits are taken from the key's unsigned image —
// uint32_t for the int32 sorts, uint64_t for auc_sort.hip's words (whose sources are defined there, with the word format).
template <typename K>
__device__ __forceinline__ unsigned int digit_of(K key, int shift, unsigned int mask) {
  return static_cast<unsigned int>(static_cast<std::make_unsigned_t<K>>(key) >> shift) & mask;
}

struct ArrayKeys {                         // a plain int32 array
  const int32_t* __restrict__ keys;
  __device__ __forceinline__ int32_t at(int64_t i) const { return keys[i]; }
};

// The digit histogram of tile blockIdx.x (LDS atomics) -> hist[(seg * nbins + digit) * tps + tis], where tile = seg * tps +
// tis (segments: one per field, tps tiles each, sorted independently; one segment: tps = the number of tiles); with
// bin_total, the segment's totals too: bin_total[seg * nbins + digit], by global integer atomics on zeroed words.
// Positions >= n do not exist.  (hist_fields_k of sort.hip, whose tiles are whole and whose key depends on the segment, is
// written out: see there.)
template <typename Src>
__device__ __forceinline__ void tile_digit_hist(const Src& src, int64_t n, int shift, int nbins, int tps, int32_t* __restrict__ hist,
                                                int32_t* __restrict__ bin_total) {
  __shared__ unsigned int h[kMaxBins];
  for (int b = threadIdx.x; b < nbins; b += kBlock) h[b] = 0;
  __syncthreads();
  const int seg = blockIdx.x / tps, tis = blockIdx.x - seg * tps;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile;
  const unsigned int mask = nbins - 1;
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[digit_of(src.at(i), shift, mask)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += kBlock) {
    const unsigned int c = h[b];
    hist[(static_cast<int64_t>(seg) * nbins + b) * tps + tis] = static_cast<int32_t>(c);
    if (bin_total && c) atomicAdd(&bin_total[seg * nbins + b], static_cast<int32_t>(c));
  }
}

// ---- the stable scatter of a tile ---------------------------------------------------------------------------------------------
// counts[w][b] = how many keys of wave w have digit b (the waves' private LDS histograms, complete: the caller's barrier)
// -> running[w][b] = this wave's first slot of digit b: offs(b), the tile's first slot of the digit, plus the counts of the
// waves before it (each lane: digits lane, lane + 64, ...).  counts may be running itself.  One barrier inside — after it
// nothing reads counts or what offs reads any more — and running[w] is visible to the wave on return.
template <typename Offs>
__device__ __forceinline__ void wave_first_slots(const int32_t (*counts)[kMaxBins], int32_t (*running)[kMaxBins], int nbins, Offs&& offs) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t first[kMaxBins / 64];
#pragma unroll
  for (int q = 0; q < kMaxBins / 64; ++q) {
    const int b = q * 64 + lane;
    int32_t f = 0;
    if (b < nbins) {
      f = offs(b);
      for (int ww = 0; ww < w; ++ww) f += counts[ww][b];
    }
    first[q] = f;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kMaxBins / 64; ++q)
    if (q * 64 + lane < nbins) running[w][q * 64 + lane] = first[q];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A wave scatters its 16 rounds alone: per round a lane finds its PEERS — the lanes of the wave whose key has the same
// digit, by one ballot per digit bit — and its rank among them (the peers in lower lanes); the key's slot is the digit's
// running slot run[d] + rank, handed to sink(slot, r); the peers' leader (rank 0) then moves the running slot past them
// all.  Between the read and the leader's write stands a wave barrier — every peer has read the slot before its leader
// moves it — and another before the next round reads.  run = this wave's slots (wave_first_slots), through lds_ld / lds_st.
// BOUNDED: the key of round r exists iff pos0 + r * 64 < n (pos0: the lane's position in round 0); lanes without one
// take no part.  REEXTRACT: the compiler may not carry the 16 digits over from the loop that counted them, it extracts
// them again from the keys (16 registers fewer where the count loop is close enough for it to try).
template <bool BOUNDED, bool REEXTRACT = false, typename K, typename Sink>
__device__ __forceinline__ void ranked_scatter(K (&key)[kItems], int shift, int nbits, int32_t* run, int64_t pos0, int64_t n, Sink&& sink) {
  const int lane = threadIdx.x & 63;
  const unsigned int mask = (1u << nbits) - 1;
  const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const bool valid = !BOUNDED || pos0 + r * 64 < n;
    if (REEXTRACT) asm volatile("" : "+v"(key[r]));
    const unsigned int d = digit_of(key[r], shift, mask);
    unsigned long long peers = BOUNDED ? __ballot(valid) : ~0ull;
    for (int b = 0; b < nbits; ++b) {
      const unsigned long long m = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? m : ~m;
    }
    const int rank = __popcll(peers & lt_mask);
    int32_t dst = 0;
    if (valid) dst = lds_ld(run + d) + rank;
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      if (rank == 0) lds_st(run + d, dst + __popcll(peers));
      sink(dst, r);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- compaction: the first entry of every distinct row ------------------------------------------------------------------------
// (seg_len > 0: positions that start a segment — a field — start a row whatever the keys say)
__device__ __forceinline__ bool is_head(const int32_t* __restrict__ keys, int64_t i, int64_t seg_len) {
  return i == 0 || keys[i] != keys[i - 1] || (seg_len > 0 && i % seg_len == 0);
}

// the number of positions of tile blockIdx.x that start a new row, in every thread (block_sum's barrier and red)
__device__ __forceinline__ int count_heads(const int32_t* __restrict__ keys, int64_t n, int64_t seg_len, int32_t* red) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile;
  int c = 0;
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kBlock + threadIdx.x;
    if (i < n && is_head(keys, i, seg_len)) ++c;
  }
  return block_sum(c, red);
}

// The compaction of tile blockIdx.x, given `run` = the heads of the tiles before it: sorted_entry = the values; per head,
// in order, uniq_rows (seg_len > 0: the key is a field's local id, field_off makes it the global row) and seg_start; with
// slot_of_entry, the segment of every entry.  The last tile closes the lists: num_uniq, seg_start[num_uniq] = n.
// BOUNDED = false: a per-field sort's tile — every position exists and seg_len > 0 — which does not pay for either check.
template <bool BOUNDED>
__device__ __forceinline__ void compact_tile(const int32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int run,
                                             int32_t* __restrict__ sorted_entry, int32_t* __restrict__ uniq_rows,
                                             int32_t* __restrict__ seg_start, int32_t* __restrict__ num_uniq, int64_t seg_len,
                                             const int64_t* __restrict__ field_off, int32_t* __restrict__ slot_of_entry) {
  __shared__ int32_t wc[kWaves];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile;
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kBlock + t;
    const bool valid = !BOUNDED || i < n;
    int32_t key = 0;
    bool head = false;
    if (valid) {
      key = keys[i];
      head = is_head(keys, i, seg_len);
      sorted_entry[i] = vals[i];
    }
    const unsigned long long hb = __ballot(head);
    __syncthreads();                       // previous round's wc consumed
    if (lane == 0) wc[w] = __popcll(hb);
    __syncthreads();
    int idx = 0;
    if (head || slot_of_entry) {
      idx = run + __popcll(hb & lt_mask);
      for (int ww = 0; ww < w; ++ww) idx += wc[ww];
    }
    if (head) {
      uniq_rows[idx] = (!BOUNDED || seg_len > 0) ? static_cast<int32_t>(field_off[i / seg_len] + key) : key;
      seg_start[idx] = static_cast<int32_t>(i);
    }
    // (the segment a position belongs to: the heads up to and including its own, minus one — what mi_segment_slots finds by
    // binary search, 112 us at 1.7 M entries, for the price of one scattered 4-byte store here)
    if (slot_of_entry && valid) slot_of_entry[vals[i]] = head ? idx : idx - 1;
    run += wc[0] + wc[1] + wc[2] + wc[3];
  }
  if (blockIdx.x == gridDim.x - 1 && t == 0) {
    num_uniq[0] = run;
    seg_start[run] = static_cast<int32_t>(n);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// `bits` key bits in digits of equal width, at most max_bits (itself held to 1..kMaxBits) wide
struct Digits {
  int passes, nbits;
};
inline Digits plan_digits(int bits, int max_bits) {
  max_bits = max_bits < 1 ? 1 : (max_bits > kMaxBits ? kMaxBits : max_bits);
  const int passes = (bits + max_bits - 1) / max_bits;
  return Digits{passes, (bits + passes - 1) / passes};
}
// the bits that tell `count` values apart: ceil(log2 count), at most cap
inline int bits_for(int64_t count, int cap) {
  int bits = 0;
  while (bits < cap && (static_cast<int64_t>(1) << bits) < count) ++bits;
  return bits;
}

}  // namespace radix
