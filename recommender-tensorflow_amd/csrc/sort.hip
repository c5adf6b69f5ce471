// Stable LSD radix sort of (row, entry index) pairs + duplicate compaction.
//
// Device analogue of TF's `unique` + `unsorted_segment_sum` (_deduplicate_indexed_slices) that
// runs before every sparse optimizer apply, reached from optimizer.minimize
// (trainers/model_utils.py:69-72 / head at trainers/deep_fm.py:119-125).
// Integer work, bit exact: equal rows keep their entry order, so the later segment sum adds
// duplicates in ascending example order like TF's CPU kernel.
//
// This file owns the int32 key + value sorts: their kernels (what a tile reads, where its offsets come from, where a ranked
// key goes), their workspace and their entries.  How a tile counts its digits, scans, ranks its keys with ballots and
// compacts the row heads is written once, in radix.h, for these and for auc_sort.hip's 64-bit words.
//
// mi_sort_unique_rows: digits of up to 9 bits (26 M rows = 25 bits -> 3 passes).  Per pass:
//   hist_k      per-tile digit histogram (LDS atomics) + per-digit totals (global integer atomics)
//   bin_scan_k  one workgroup per digit: base = sum of the lower digits' totals, then an
//               exclusive scan of that digit's per-tile counts (wave shuffles, carried in chunks)
//   scatter_k   stable scatter: lanes find their equal-digit peers in the wave with ballots; a wave owns
//               a contiguous quarter of the tile and keeps its own running slot per digit in LDS
// then head_count_k / scan_small_k / compact_k mark the first entry of every distinct row (coalesced reads,
// ballot ranks) and emit uniq_rows / seg_start / sorted_entry.
// mi_sort_unique_fields: the same result for ids [B][F] of F fields whose rows are disjoint ranges — every field's
// B local ids sorted on their own (segments), 20 bits instead of 25 at config 3: 3 passes of 7 bits.  Two forms, same
// outputs: beside = 0, one launch per pass whose tiles wait for each other (pass_fused_k / compact_fused_k), and the
// short launches that run beside the catch-up, where nothing may wait — per pass hist_fields_k + scatter_runs_k, then
// head_count_k + compact_fields_k (9 launches at config 3, 113 us alone; the 14 of hist_k / bin_scan_k / scatter_k
// they replace: 145).  There a (key, value) travels as one 8-byte pair, pass 0 reads ids [B][F] in place, a tile
// derives its own offsets from the raw counts (no bin_scan_k), stages its pairs in LDS in digit order and writes
// them out in runs, and the compaction adds up the head counts before it itself (no scan_small_k):
// profiles/sort_beside_scatter.md.
#include "radix.h"

namespace {

using namespace radix;

constexpr int kMaxPasses = 4;
constexpr int kFusedMaxTps = 256;          // tiles per field up to which a field's tiles wait for each other inside one launch

// (our own kernel instead of hipMemsetAsync: a plain kernel node when the step is captured into a hipGraph — a
// LINEAR captured step with memset nodes faulted at replay on this ROCm, the same step with a forked side stream
// did not — and no runtime fill-kernel in between ours)
__global__ __launch_bounds__(256) void zero_i32_k(int32_t* __restrict__ p, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) p[i] = 0;
}
inline void zero_i32(int32_t* p, int64_t n, hipStream_t st) {
  const int64_t b = (n + 255) / 256;
  zero_i32_k<<<dim3(static_cast<unsigned>(b < 64 ? b : 64)), dim3(256), 0, st>>>(p, n);
}

// Segments (mi_sort_unique_fields: one per field, tps tiles each, sorted independently): tile = seg * tps + tis,
// hist[(seg * nbins + digit) * tps + tis], bin_total[seg * nbins + digit].  One segment: tps = ntiles.
__global__ __launch_bounds__(kBlock) void hist_k(const int32_t* __restrict__ keys, int64_t n, int shift,
                                                 int nbins, int tps, int32_t* __restrict__ hist,
                                                 int32_t* __restrict__ bin_total) {
  tile_digit_hist(ArrayKeys{keys}, n, shift, nbins, tps, hist, bin_total);
}

// hist_k of the catch-up's staleness key, computed on the way (the key of mi_catchup_gap_keys: steps to replay,
// clamped to 62; 63 for the slots past num_uniq) and kept for the scatter.  (Not tile_digit_hist: the 16 keys are two
// dependent loads each, all issued before the first store, and the 64 bins are one per thread of a wave.  The kernel on the
// shared body was neither built nor timed.)
__global__ __launch_bounds__(kBlock) void gap_hist_k(const int32_t* __restrict__ uniq_rows, const int32_t* __restrict__ num_uniq,
                                                     const int32_t* __restrict__ last_step, int64_t n, int step_to, int st,
                                                     const mi_step_state_t* __restrict__ ss, int32_t* __restrict__ keys,
                                                     int ntiles, int32_t* __restrict__ hist, int32_t* __restrict__ bin_total) {
  __shared__ unsigned int h[64];
  if (ss) step_to = ss->step - 1;
  if (threadIdx.x < 64) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile;
  const int64_t U = *num_uniq;
  int32_t key[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kBlock + threadIdx.x;
    key[r] = 63;
    if (i < U) {
      const int ls = last_step[static_cast<int64_t>(uniq_rows[i]) * st];
      key[r] = (ls > 0 && ls < step_to) ? min(step_to - ls, 62) : 0;
    }
  }
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kBlock + threadIdx.x;
    if (i < n) { keys[i] = key[r]; atomicAdd(&h[key[r]], 1u); }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const unsigned int c = h[threadIdx.x];
    hist[static_cast<int64_t>(threadIdx.x) * ntiles + blockIdx.x] = static_cast<int32_t>(c);
    if (c) atomicAdd(&bin_total[threadIdx.x], static_cast<int32_t>(c));
  }
}

// block (seg, b): hist[seg, b, 0..tps) -> global offsets (exclusive scan + base of digit b inside segment seg,
// which starts at seg * seg_len)
__global__ __launch_bounds__(kBlock) void bin_scan_k(int32_t* __restrict__ hist, int ntiles, int nbins,
                                                     const int32_t* __restrict__ bin_total, int64_t seg_len) {
  __shared__ int32_t red[kWaves];
  const int seg = blockIdx.x / nbins, b = blockIdx.x - seg * nbins;
  bin_total += seg * nbins;
  int part = 0;
  for (int j = threadIdx.x; j < b; j += kBlock) part += bin_total[j];
  const int base = block_sum(part, red) + static_cast<int>(seg * seg_len);
  int32_t* row = hist + (static_cast<int64_t>(seg) * nbins + b) * ntiles;
  block_excl_scan_chunked<kBlock>(ntiles, base, [&](int i) { return row[i]; }, [&](int i, int excl, int) { row[i] = excl; });
}

// Two block barriers in total: the waves first count their digits (private LDS histograms), every wave then derives its
// own running offsets (tile offset of the digit + the counts of the waves before it) and scatters its 16 rounds alone.
// (vals_in == NULL: the value of position i is i — or, with fm_B > 0, the entry b * fm_F + f of the field-major
// position i = f * fm_B + b.)
__global__ __launch_bounds__(kBlock) void scatter_k(const int32_t* __restrict__ keys_in,
                                                    const int32_t* __restrict__ vals_in, int64_t n,
                                                    int shift, int nbits, int tps,
                                                    const int32_t* __restrict__ offs,
                                                    int32_t* __restrict__ keys_out,
                                                    int32_t* __restrict__ vals_out, int64_t fm_B = 0, int fm_F = 0) {
  __shared__ int32_t running[kWaves][kMaxBins];    // per wave: digit counts, then the next output slot of each digit
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nbins = 1 << nbits;
  const int seg = blockIdx.x / tps, tis = blockIdx.x - seg * tps;
  for (int b = t; b < kWaves * kMaxBins; b += kBlock) (&running[0][0])[b] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile + w * (64 * kItems) + lane;
  int32_t key[kItems], val[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * 64;
    const bool valid = i < n;
    key[r] = valid ? keys_in[i] : 0;
    val[r] = valid ? (vals_in ? vals_in[i] : (fm_B ? static_cast<int32_t>((i % fm_B) * fm_F + i / fm_B) : static_cast<int32_t>(i))) : 0;
    if (valid) atomicAdd(&running[w][digit_of(key[r], shift, nbins - 1)], 1);
  }
  __syncthreads();
  wave_first_slots(running, running, nbins, [&](int b) { return offs[(static_cast<int64_t>(seg) * nbins + b) * tps + tis]; });
  ranked_scatter<true>(key, shift, nbits, running[w], base, n, [&](int32_t dst, int r) {
    keys_out[dst] = key[r];
    vals_out[dst] = val[r];
  });
}

// heads[tile] = number of positions in the tile that start a new row
__global__ __launch_bounds__(kBlock) void head_count_k(const int32_t* __restrict__ keys, int64_t n,
                                                       int32_t* __restrict__ tile_heads, int64_t seg_len = 0) {
  __shared__ int32_t red[kWaves];
  const int c = count_heads(keys, n, seg_len, red);
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = c;
}

// exclusive scan of `count` int32 values by ONE block (count = number of tiles: small).  256 threads, not 1,024: a
// 16-wave workgroup needs four free wave slots on every SIMD of ONE CU at the same moment, and beside the sparse apply or
// the resident catch-up workgroups it waited for that for 0.17 ms on average (0.5 ms at worst: rocprofv3 trace of the
// row-sharded step, profiles/r05_sharded_one_rank.md) — for 5 us of work.
constexpr int kScanSmallBlock = 256;
__global__ __launch_bounds__(kScanSmallBlock) void scan_small_k(int32_t* __restrict__ data, int64_t count) {
  block_excl_scan_chunked<kScanSmallBlock>(count, 0, [&](int64_t i) { return data[i]; }, [&](int64_t i, int excl, int) { data[i] = excl; });
}

// tile_base = the heads of the tiles before each (scan_small_k of head_count_k's counts)
__global__ __launch_bounds__(kBlock) void compact_k(const int32_t* __restrict__ keys,
                                                    const int32_t* __restrict__ vals, int64_t n,
                                                    const int32_t* __restrict__ tile_base,
                                                    int32_t* __restrict__ sorted_entry,
                                                    int32_t* __restrict__ uniq_rows,
                                                    int32_t* __restrict__ seg_start,
                                                    int32_t* __restrict__ num_uniq, int64_t seg_len = 0,
                                                    const int64_t* __restrict__ field_off = nullptr,
                                                    int32_t* __restrict__ slot_of_entry = nullptr) {
  compact_tile<true>(keys, vals, n, tile_base[blockIdx.x], sorted_entry, uniq_rows, seg_start, num_uniq, seg_len, field_off, slot_of_entry);
}

constexpr int kFieldsMax = 64;

// ---- The short launches of mi_sort_unique_fields (beside the catch-up: no workgroup waits for another) ------------------
// Between the passes a (key, value) is ONE 8-byte pair; pass 0 reads ids [B][F] in place: the key of field-major position
// i = seg * B + b is ids[b * F + seg], its value the entry b * F + seg, so no field-major copy of the ids is made.
__device__ __forceinline__ int32_t fields_key(const int2* __restrict__ pairs_in, const int32_t* __restrict__ ids, int64_t i,
                                              int seg, int64_t B, int F) {
  return ids ? ids[(i - static_cast<int64_t>(seg) * B) * F + seg] : pairs_in[i].x;
}

// hist_k of a field's tile (B is a multiple of kTile: every position exists).  Written out, not on radix.h's
// tile_digit_hist: on it, with a key source that took the segment, the kernel ran 7.70 to 7.74 us against 7.60 to 7.68
// for this text (three earlier forms of the source: 7.72 to 7.88), above its own run-to-run range of 0.08 us
// (profiles/sort_one_body.md).
__global__ __launch_bounds__(kBlock) void hist_fields_k(const int2* __restrict__ pairs_in, const int32_t* __restrict__ ids, int64_t B,
                                                        int F, int shift, int nbins, int tps, int32_t* __restrict__ hist,
                                                        int32_t* __restrict__ bin_total) {
  __shared__ unsigned int h[kMaxBins];
  for (int b = threadIdx.x; b < nbins; b += kBlock) h[b] = 0;
  __syncthreads();
  const int seg = blockIdx.x / tps, tis = blockIdx.x - seg * tps;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile;
  const unsigned int mask = nbins - 1;
#pragma unroll
  for (int r = 0; r < kItems; ++r)
    atomicAdd(&h[digit_of(fields_key(pairs_in, ids, base + r * kBlock + threadIdx.x, seg, B, F), shift, mask)], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += kBlock) {
    const unsigned int c = h[b];
    hist[(static_cast<int64_t>(seg) * nbins + b) * tps + tis] = static_cast<int32_t>(c);
    if (c) atomicAdd(&bin_total[seg * nbins + b], static_cast<int32_t>(c));
  }
}

// A tile finds its own output offsets where that read is small beside the tile's own 64 KB of pairs: per digit, the field's
// total (exclusive scan over the digits) + the counts of the field's tiles before this one, straight from hist_k's raw
// counts — nbins * tps ints at most (2,176 at config 3, L2-resident).  Up to kSelfOffsMaxInts = a quarter of the tile's
// own traffic; above it bin_scan_k turns hist into offsets first, as for the other callers.
constexpr int kSelfOffsMaxInts = 4096;

// scatter_k for a field's tile, writing RUNS: the tile is first staged in LDS in digit order — stable: a key's place is
// the tile-local start of its digit + the counts of the waves before its own + its wave's running count + its ballot rank
// — and then written out in staged order, so consecutive lanes write consecutive slots of one bin (runs of ~32 pairs at
// config 3: a wave's store touches a few lines, not 64).  The worst case — all 4,096 keys in one bin — is one run.
// self_offs: hist holds the raw per-tile counts (see above), else the offsets bin_scan_k made of them.
// keys_out != NULL (the last pass): keys and values go to two arrays, what head_count_k / compact_k read.
// LDS: 32 KB of pairs + 8 KB of running slots: four workgroups per CU.  Before the staging the pairs' space holds the
// waves' digit counts and the scans' scratch, after it the first wave's slots hold (global offset - tile-local start) per digit.
template <bool IDS>
__global__ __launch_bounds__(kBlock) void scatter_runs_k(const int2* __restrict__ pairs_in, const int32_t* __restrict__ ids, int64_t B,
                                                         int F, int shift, int nbits, int tps, const int32_t* __restrict__ hist,
                                                         const int32_t* __restrict__ bin_total, int self_offs,
                                                         int2* __restrict__ pairs_out, int32_t* __restrict__ keys_out,
                                                         int32_t* __restrict__ vals_out) {
  __shared__ int2 staged[kTile];
  __shared__ int32_t running[kWaves][kMaxBins];    // per wave: the next staged slot of each digit
  int32_t* before = reinterpret_cast<int32_t*>(staged);      // [nbins] counts of the field's earlier tiles
  int32_t* tstart = before + kMaxBins;                       // [nbins] tile-local start of a digit
  int32_t (*cnt)[kMaxBins] = reinterpret_cast<int32_t (*)[kMaxBins]>(tstart + kMaxBins);   // [4][nbins] per wave: digit counts
  int32_t* wsum = &cnt[kWaves][0];                                                         // [2][4] the waves' sums of the two scans
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nbins = 1 << nbits;
  const int seg = blockIdx.x / tps, tis = blockIdx.x - seg * tps;
  for (int b = t; b < kWaves * kMaxBins; b += kBlock) (&cnt[0][0])[b] = 0;
  for (int b = t; b < nbins; b += kBlock) before[b] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile + w * (64 * kItems);
  // (pass 0: the value is the entry itself, made again where it is stored — 16 registers fewer)
  const int32_t e0 = static_cast<int32_t>((base - static_cast<int64_t>(seg) * B + lane) * F + seg);
  int32_t key[kItems], val[IDS ? 1 : kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    if (IDS) {
      key[r] = ids[e0 + r * 64 * F];
    } else {
      const int2 kv = pairs_in[base + r * 64 + lane];
      key[r] = kv.x;
      val[r] = kv.y;
    }
    atomicAdd(&cnt[w][digit_of(key[r], shift, nbins - 1)], 1);
  }
  const int32_t* fh = hist + static_cast<int64_t>(seg) * nbins * tps;      // the field's counts [digit][tile]
  if (self_offs)
    for (int i = t; i < nbins * tps; i += kBlock) {
      const int b = i / tps;
      if (i - b * tps < tis) atomicAdd(&before[b], fh[i]);
    }
  __syncthreads();
  // two exclusive scans over the digits: the tile's own counts -> tile-local starts; the field's totals -> the digit's base
  // in the field (which starts at seg * B)
  const int per = digits_per_thread(nbins);
  int32_t delta[kMaxBins / kBlock] = {};
  digit_excl_scan<2>(
      nbins, wsum,
      [&](int b, int (&c)[2]) {
        c[0] = cnt[0][b] + cnt[1][b] + cnt[2][b] + cnt[3][b];
        if (self_offs) c[1] = bin_total[seg * nbins + b];
      },
      [&](int b, int j, const int (&pre)[2]) {
        const int32_t gofs = self_offs ? pre[1] + static_cast<int>(static_cast<int64_t>(seg) * B) + before[b] : fh[static_cast<int64_t>(b) * tps + tis];
        delta[j] = gofs - pre[0];
        tstart[b] = pre[0];
      });
  __syncthreads();
  // counts -> this wave's first staged slot per digit.  (radix.h's wave_first_slots written out as a loop: counts and slots
  // are two arrays here, so nothing is held in registers across a barrier; with the shared body, unrolled over the 8 x 64
  // digits, the kernel was 28 % longer and ran 21.75 us instead of 21.58 (pass 0: 24.27 instead of 24.07) in a kernel
  // trace of tools/sort_bench.py fields, parent and change alternating three times, the parent's own range 0.08.)
  for (int b = lane; b < nbins; b += 64) {
    int32_t f = tstart[b];
    for (int ww = 0; ww < w; ++ww) f += cnt[ww][b];
    running[w][b] = f;
  }
  __syncthreads();                              // the scratch is read by everyone: the staging may overwrite it
  ranked_scatter<false, true>(key, shift, nbits, running[w], 0, 0,
                              [&](int32_t dst, int r) { staged[dst] = make_int2(key[r], IDS ? e0 + r * 64 * F : val[r]); });
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kMaxBins / kBlock; ++j)
    if (j < per && t * per + j < nbins) running[0][t * per + j] = delta[j];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int s = r * kBlock + t;
    const int2 kv = staged[s];
    const int32_t dst = running[0][digit_of(kv.x, shift, nbins - 1)] + s;
    if (keys_out) {
      keys_out[dst] = kv.x;
      vals_out[dst] = kv.y;
    } else {
      pairs_out[dst] = kv;
    }
  }
}

// compact_k without scan_small_k's launch: a tile adds up the head counts of the tiles before it itself (up to
// kFoldHeadsMaxTiles ints, a quarter of the 64 KB it reads and writes anyway).
constexpr int kFoldHeadsMaxTiles = 4096;
__global__ __launch_bounds__(kBlock) void compact_fields_k(const int32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                                                           const int32_t* __restrict__ tile_heads, int32_t* __restrict__ sorted_entry,
                                                           int32_t* __restrict__ uniq_rows, int32_t* __restrict__ seg_start,
                                                           int32_t* __restrict__ num_uniq, int64_t seg_len,
                                                           const int64_t* __restrict__ field_off) {
  __shared__ int32_t red[kWaves];
  int part = 0;
  for (int j = threadIdx.x; j < static_cast<int>(blockIdx.x); j += kBlock) part += tile_heads[j];
  compact_tile<false>(keys, vals, n, block_sum(part, red), sorted_entry, uniq_rows, seg_start, num_uniq, seg_len, field_off, nullptr);
}


// ---- One launch per radix pass, one for the compaction (mi_sort_unique_fields) --------------------------
// hist_k + bin_scan_k + scatter_k of a pass as ONE kernel: a tile counts its digits, PUBLISHES the counts, waits until the
// other tiles of its field have published theirs (tps <= kFusedMaxTps workgroups, consecutive block ids: dispatched together),
// derives its own offsets from them and scatters.  14 dependent launches of ~12 us each (most of them a few workgroups or
// ONE) become 4-5.  Cross-workgroup traffic goes through agent-scope atomics (the L2s of the 8 XCDs are not coherent for
// plain loads inside a launch): relaxed stores of the counts, a release increment of the field's arrival counter, an
// acquire spin on it, relaxed loads of the counts.  The spin is bounded (every wave reaches its exit: a tile that never
// sees its field complete raises *err and goes on with what it has — garbage that tests catch — instead of hanging the GPU).
__device__ __forceinline__ void st_agent(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
constexpr int kSpinMax = 1 << 22;          // x s_sleep 8 (~0.25 us): about a second

// pass 0 reads ids [B][F] itself (key = the local id of (b, seg), value = the entry b * F + seg): no field-major copy
__global__ __launch_bounds__(kBlock) void pass_fused_k(const int32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in,
                                                       const int32_t* __restrict__ ids, int64_t B, int F, int shift, int nbits,
                                                       int tps, int32_t* __restrict__ thist, int32_t* __restrict__ ready,
                                                       int32_t* __restrict__ err, int32_t* __restrict__ keys_out,
                                                       int32_t* __restrict__ vals_out, int nap) {
  __shared__ int32_t running[kWaves][kMaxBins];    // per wave: digit counts, then the next output slot of each digit
  __shared__ int32_t offsT[kMaxBins];              // this tile's first slot per digit
  __shared__ int32_t totS[kMaxBins];               // the field's total per digit
  __shared__ int32_t wsum[kWaves];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nbins = 1 << nbits;
  const int seg = blockIdx.x / tps, tis = blockIdx.x - seg * tps;
  for (int b = t; b < kWaves * kMaxBins; b += kBlock) (&running[0][0])[b] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile + w * (64 * kItems);
  int32_t key[kItems], val[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * 64 + lane;         // (B is a multiple of kTile: every position exists)
    if (ids) {
      const int64_t e = (i - static_cast<int64_t>(seg) * B) * F + seg;
      key[r] = ids[e];
      val[r] = static_cast<int32_t>(e);
    } else {
      key[r] = keys_in[i];
      val[r] = vals_in[i];
    }
    atomicAdd(&running[w][digit_of(key[r], shift, nbins - 1)], 1);
  }
  __syncthreads();
  for (int b = t; b < nbins; b += kBlock)
    st_agent(thist + static_cast<int64_t>(blockIdx.x) * nbins + b, running[0][b] + running[1][b] + running[2][b] + running[3][b]);
  // (the counts went out as write-through stores: once they are acknowledged — vmcnt 0 in every wave, then the barrier —
  // a RELAXED increment publishes them.  A release increment would write back this XCD's whole L2, an acquire load in the
  // spin invalidate it on every turn: 160-190 us per sort instead of 150 for the 14 launches this replaces.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    __hip_atomic_fetch_add(ready + seg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int spins = 0;
    while (ld_agent(ready + seg) < tps) {
      if (nap >= 2) __builtin_amdgcn_s_sleep(100); else if (nap == 1) __builtin_amdgcn_s_sleep(32); else __builtin_amdgcn_s_sleep(4);
      if (++spins > kSpinMax) { atomicExch(err, 1); break; }
    }
  }
  __syncthreads();
  // per digit: the field's total and the part of it that lies in the tiles before this one (L2-bypassing loads, kept in
  // flight eight at a time: one after the other they cost a memory latency each)
  for (int b = t; b < nbins; b += kBlock) {
    const int32_t* col = thist + static_cast<int64_t>(seg) * tps * nbins + b;
    int total = 0, before = 0;
    for (int t0 = 0; t0 < tps; t0 += 8) {
      int v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (t0 + j < tps) ? ld_agent(col + static_cast<int64_t>(t0 + j) * nbins) : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        total += v[j];
        before += (t0 + j < tis) ? v[j] : 0;
      }
    }
    totS[b] = total;
    offsT[b] = before;
  }
  __syncthreads();
  // the digit's base in the field (which starts at seg * B): the exclusive scan of the totals over the digits
  digit_excl_scan<1>(
      nbins, wsum, [&](int b, int (&c)[1]) { c[0] = totS[b]; },
      [&](int b, int, const int (&pre)[1]) { offsT[b] += pre[0] + static_cast<int>(static_cast<int64_t>(seg) * B); });
  __syncthreads();
  wave_first_slots(running, running, nbins, [&](int b) { return offsT[b]; });
  ranked_scatter<false>(key, shift, nbits, running[w], 0, 0, [&](int32_t dst, int r) {
    keys_out[dst] = key[r];
    vals_out[dst] = val[r];
  });
}

// head_count_k + scan_small_k + compact_k as one launch: a tile publishes its number of row heads (+ 1: 0 = not there yet)
// and waits for the tiles BEFORE it only — lower block ids, dispatched earlier — to know where its rows start.
__global__ __launch_bounds__(kBlock) void compact_fused_k(const int32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                                                          int32_t* __restrict__ hcf, int32_t* __restrict__ err,
                                                          int32_t* __restrict__ sorted_entry, int32_t* __restrict__ uniq_rows,
                                                          int32_t* __restrict__ seg_start, int32_t* __restrict__ num_uniq,
                                                          int64_t seg_len, const int64_t* __restrict__ field_off) {
  __shared__ int32_t red[kWaves];
  const int mine = count_heads(keys, n, seg_len, red);
  if (threadIdx.x == 0) st_agent(hcf + blockIdx.x, mine + 1);
  int part = 0;
  for (int j = threadIdx.x; j < static_cast<int>(blockIdx.x); j += kBlock) {
    int v, spins = 0;
    while ((v = ld_agent(hcf + j)) == 0) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > kSpinMax) { atomicExch(err, 1); v = 1; break; }
    }
    part += v - 1;
  }
  __syncthreads();                         // red[] read by everyone
  compact_tile<true>(keys, vals, n, block_sum(part, red), sorted_entry, uniq_rows, seg_start, num_uniq, seg_len, field_off, nullptr);
}

// The workspace: two key and two value buffers (the per-field short launches use each pair of them as one pair buffer),
// hist, the tiles' head counts, bin_total per pass (and field), the fused passes' sync words.
// kReservedBytes: unused.  The region held the rows sort's total, which the last tile of the compaction knows itself; it stays
// so that mi_sort_unique_workspace_bytes and mi_sort_unique_fields_workspace_bytes return what callers already allocate.
constexpr int64_t kReservedBytes = 256;
struct Layout {
  int64_t ntiles, keysA, keysB, valsA, valsB, hist, heads, bin_total, sync, sync_words, bytes;
};

Layout layout_for(int64_t n, int nseg = 1) {
  Layout L;
  L.ntiles = mi::ceil_div(n > 0 ? n : 1, kTile);
  int64_t o = 0;
  const int64_t nb = align_up(n * 4, 256);
  L.keysA = o; o += nb;
  L.keysB = o; o += nb;
  L.valsA = o; o += nb;
  L.valsB = o; o += nb;
  L.hist = o; o += align_up(L.ntiles * kMaxBins * 4, 256);
  L.heads = o; o += align_up(L.ntiles * 4, 256);
  L.bin_total = o; o += static_cast<int64_t>(kMaxPasses) * (nseg > 1 ? nseg : 1) * kMaxBins * 4;
  o += kReservedBytes;
  // the fused passes' sync words (mi_sort_unique_fields): [pass][field] arrival counters, one published head count per
  // tile, one error word — zeroed by the entry's first launch
  L.sync_words = static_cast<int64_t>(kMaxPasses) * (nseg > 1 ? nseg : 1) + L.ntiles + 1;
  L.sync = o; o += align_up(L.sync_words * 4, 256);
  L.bytes = o;
  return L;
}

struct Buffers {
  int32_t *kbuf[2], *vbuf[2], *hist, *heads, *bin_total, *sync;
  int ntiles;
};
Buffers carve(void* workspace, const Layout& L) {
  char* ws = static_cast<char*>(workspace);
  auto at = [&](int64_t o) { return reinterpret_cast<int32_t*>(ws + o); };
  return Buffers{{at(L.keysA), at(L.keysB)}, {at(L.valsA), at(L.valsB)}, at(L.hist), at(L.heads), at(L.bin_total), at(L.sync),
                 static_cast<int>(L.ntiles)};
}

// the digits of an int32 key below `count`
Digits plan_rows(int64_t count, int max_bits) {
  const int bits = bits_for(count, 31);
  return plan_digits(bits > 1 ? bits : 1, max_bits);
}

}  // namespace

// ---- n <= kSmallN: the whole sort + unique in ONE workgroup (the launch-bound small-batch step: B = 32 x 26 fields
// = 832 keys would otherwise take a dozen launches).
namespace {
constexpr int kSmallN = 1024;
__global__ __launch_bounds__(kBlock) void sort_small_k(const int32_t* __restrict__ keys, int n, int32_t* __restrict__ sorted_entry,
                                                       int32_t* __restrict__ uniq_rows, int32_t* __restrict__ seg_start,
                                                       int32_t* __restrict__ num_uniq, int32_t* __restrict__ slot_of_entry = nullptr) {
  // bitonic sort of (key << 10 | index) in LDS: the index makes equal keys keep their order (stable), padding sorts
  // last.  (The first version ranked every key against every other: 87 us of the 280-us B = 32 step.)
  __shared__ unsigned long long a[kSmallN];
  __shared__ int32_t sk[kSmallN], head[kSmallN];
  const int t = threadIdx.x;
  int np2 = 64;
  while (np2 < n) np2 <<= 1;
  for (int i = t; i < np2; i += kBlock)
    a[i] = i < n ? (static_cast<unsigned long long>(static_cast<uint32_t>(keys[i])) << 10) | static_cast<unsigned>(i) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < np2; i += kBlock) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long x = a[i], y = a[p];
          if ((x > y) == ((i & k) == 0)) { a[i] = y; a[p] = x; }
        }
      }
      __syncthreads();
    }
  for (int i = t; i < n; i += kBlock) {
    sk[i] = static_cast<int32_t>(a[i] >> 10);
    sorted_entry[i] = static_cast<int32_t>(a[i] & 1023u);
  }
  if (!uniq_rows) return;
  __syncthreads();
  // head flags -> exclusive scan (4 passes of 256) -> compaction
  const int U = block_excl_scan_chunked<kBlock>(
      n, 0, [&](int i) { return (i == 0 || sk[i] != sk[i - 1]) ? 1 : 0; },
      [&](int i, int excl, int v) {
        head[i] = v ? excl : -1;
        if (slot_of_entry) slot_of_entry[a[i] & 1023u] = excl + v - 1;      // (heads up to and including i, minus one)
      });
  __syncthreads();
  for (int i = t; i < n; i += kBlock)
    if (head[i] >= 0) { uniq_rows[head[i]] = sk[i]; seg_start[head[i]] = i; }
  if (t == 0) { seg_start[U] = n; *num_uniq = U; }
}
}  // namespace

extern "C" {

size_t mi_sort_unique_workspace_bytes(int64_t n) { return static_cast<size_t>(layout_for(n).bytes); }

static int32_t sort_unique_rows_impl(const int32_t* rows, int64_t n, int64_t num_rows_total,
                                     int32_t* sorted_entry, int32_t* uniq_rows, int32_t* seg_start,
                                     int32_t* num_uniq, int32_t* slot_of_entry, void* workspace, size_t workspace_bytes,
                                     mi_stream_t stream) {
  MI_REQUIRE(n > 0 && n < (int64_t)INT32_MAX - kTile, "sort_unique_rows: n=%lld", (long long)n);
  MI_REQUIRE(num_rows_total > 0 && num_rows_total <= (int64_t)INT32_MAX, "sort_unique_rows: num_rows_total=%lld",
             (long long)num_rows_total);
  MI_REQUIRE(rows && sorted_entry && workspace, "sort_unique_rows: null buffer");
  const bool perm_only = uniq_rows == nullptr;       // just the stable sort permutation, no unique / segment pass
  MI_REQUIRE(perm_only || (seg_start && num_uniq), "sort_unique_rows: uniq_rows needs seg_start and num_uniq");
  MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "sort_unique_rows: workspace must be 256-byte aligned");
  const Layout L = layout_for(n);
  if (workspace_bytes < static_cast<size_t>(L.bytes)) {
    mi::set_error("sort_unique_rows: workspace %zu < %lld", workspace_bytes, (long long)L.bytes);
    return MI_ERR_WORKSPACE;
  }
  hipStream_t st = mi::as_stream(stream);
  if (n <= kSmallN) {
    sort_small_k<<<dim3(1), dim3(kBlock), 0, st>>>(rows, static_cast<int>(n), sorted_entry, uniq_rows, seg_start, num_uniq, slot_of_entry);
    MI_CHECK_LAUNCH("sort_unique_rows(small)");
    return MI_OK;
  }
  const Buffers W = carve(workspace, L);
  const int ntiles = W.ntiles;
  const Digits D = plan_rows(num_rows_total, kMaxBits);
  const int nbins = 1 << D.nbits;

  zero_i32(W.bin_total, kMaxPasses * kMaxBins, st);
  MI_CHECK_LAUNCH("sort_unique_rows(zero)");
  const int32_t* kin = rows;
  const int32_t* vin = nullptr;  // pass 0: value = position
  for (int p = 0; p < D.passes; ++p) {
    int32_t* kout = W.kbuf[p & 1];
    int32_t* vout = (perm_only && p == D.passes - 1) ? sorted_entry : W.vbuf[p & 1];
    int32_t* bt = W.bin_total + p * kMaxBins;
    hist_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kin, n, D.nbits * p, nbins, ntiles, W.hist, bt);
    MI_CHECK_LAUNCH("sort_unique_rows(hist)");
    bin_scan_k<<<dim3(nbins), dim3(kBlock), 0, st>>>(W.hist, ntiles, nbins, bt, 0);
    MI_CHECK_LAUNCH("sort_unique_rows(scan)");
    scatter_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kin, vin, n, D.nbits * p, D.nbits, ntiles, W.hist, kout, vout);
    MI_CHECK_LAUNCH("sort_unique_rows(scatter)");
    kin = kout;
    vin = vout;
  }
  if (perm_only) return MI_OK;
  head_count_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kin, n, W.heads);
  MI_CHECK_LAUNCH("sort_unique_rows(heads)");
  scan_small_k<<<dim3(1), dim3(kScanSmallBlock), 0, st>>>(W.heads, ntiles);
  MI_CHECK_LAUNCH("sort_unique_rows(scan heads)");
  compact_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kin, vin, n, W.heads, sorted_entry, uniq_rows, seg_start, num_uniq, 0, nullptr,
                                                   slot_of_entry);
  MI_CHECK_LAUNCH("sort_unique_rows(compact)");
  return MI_OK;
}

int32_t mi_sort_unique_rows(const int32_t* rows, int64_t n, int64_t num_rows_total, int32_t* sorted_entry, int32_t* uniq_rows,
                            int32_t* seg_start, int32_t* num_uniq, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return sort_unique_rows_impl(rows, n, num_rows_total, sorted_entry, uniq_rows, seg_start, num_uniq, nullptr, workspace, workspace_bytes, stream);
}

int32_t mi_sort_unique_rows_slots(const int32_t* rows, int64_t n, int64_t num_rows_total, int32_t* sorted_entry, int32_t* uniq_rows,
                                  int32_t* seg_start, int32_t* num_uniq, int32_t* slot_of_entry, void* workspace,
                                  size_t workspace_bytes, mi_stream_t stream) {
  MI_REQUIRE(slot_of_entry && uniq_rows, "sort_unique_rows_slots: null buffer");
  return sort_unique_rows_impl(rows, n, num_rows_total, sorted_entry, uniq_rows, seg_start, num_uniq, slot_of_entry, workspace, workspace_bytes, stream);
}


int32_t mi_catchup_rows_by_gap(const int32_t* uniq_rows, const int32_t* num_uniq, const int32_t* last_step, int64_t n_max,
                               int32_t step_to, int32_t lin_stride, int32_t* rows_out, void* workspace,
                               size_t workspace_bytes, mi_stream_t stream) {
  MI_REQUIRE(n_max >= 0 && n_max < (int64_t)INT32_MAX - kTile && step_to >= 0 && lin_stride >= 1,
             "catchup_rows_by_gap: n_max=%lld", (long long)n_max);
  if (n_max == 0) return MI_OK;
  MI_REQUIRE(uniq_rows && num_uniq && last_step && rows_out && workspace, "catchup_rows_by_gap: null buffer");
  MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "catchup_rows_by_gap: workspace must be 256-byte aligned");
  const Layout L = layout_for(n_max);
  if (workspace_bytes < static_cast<size_t>(L.bytes)) {
    mi::set_error("catchup_rows_by_gap: workspace %zu < %lld", workspace_bytes, (long long)L.bytes);
    return MI_ERR_WORKSPACE;
  }
  hipStream_t st = mi::as_stream(stream);
  const Buffers W = carve(workspace, L);
  int32_t* keys = W.kbuf[0];
  int32_t* keys_sorted = W.kbuf[1];
  const int ntiles = W.ntiles;
  zero_i32(W.bin_total, 64, st);
  MI_CHECK_LAUNCH("catchup_rows_by_gap(zero)");
  gap_hist_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(uniq_rows, num_uniq, last_step, n_max, step_to, lin_stride, mi::step_state(),
                                                    keys, ntiles, W.hist, W.bin_total);
  MI_CHECK_LAUNCH("catchup_rows_by_gap(keys + hist)");
  bin_scan_k<<<dim3(64), dim3(kBlock), 0, st>>>(W.hist, ntiles, 64, W.bin_total, 0);
  MI_CHECK_LAUNCH("catchup_rows_by_gap(scan)");
  scatter_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(keys, uniq_rows, n_max, 0, 6, ntiles, W.hist, keys_sorted, rows_out);
  MI_CHECK_LAUNCH("catchup_rows_by_gap(scatter)");
  return MI_OK;
}


size_t mi_sort_unique_fields_workspace_bytes(int64_t B, int32_t F) {
  return static_cast<size_t>(layout_for(B * (F > 0 ? F : 1), F).bytes);
}

int32_t mi_sort_unique_fields(const int32_t* ids, const int64_t* field_off, int64_t B, int32_t F, int64_t max_vocab,
                              int32_t* sorted_entry, int32_t* uniq_rows, int32_t* seg_start, int32_t* num_uniq,
                              void* workspace, size_t workspace_bytes, int32_t beside, mi_stream_t stream) {
  const int64_t n = B * F;
  MI_REQUIRE(B > 0 && F > 0 && F <= kFieldsMax && B % kTile == 0 && n < (int64_t)INT32_MAX - kTile,
             "sort_unique_fields: B=%lld (a multiple of %d) F=%d (<= %d)", (long long)B, kTile, F, kFieldsMax);
  MI_REQUIRE(max_vocab > 0 && max_vocab <= (int64_t)1 << 30, "sort_unique_fields: max_vocab=%lld", (long long)max_vocab);
  MI_REQUIRE(ids && field_off && sorted_entry && uniq_rows && seg_start && num_uniq && workspace, "sort_unique_fields: null buffer");
  MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "sort_unique_fields: workspace must be 256-byte aligned");
  const Layout L = layout_for(n, F);
  if (workspace_bytes < static_cast<size_t>(L.bytes)) {
    mi::set_error("sort_unique_fields: workspace %zu < %lld", workspace_bytes, (long long)L.bytes);
    return MI_ERR_WORKSPACE;
  }
  hipStream_t st = mi::as_stream(stream);
  const Buffers W = carve(workspace, L);
  const int ntiles = W.ntiles, tps = static_cast<int>(B / kTile);

  if (tps <= kFusedMaxTps && !beside && mi::env_int("MI_SORT_FUSED", 1) != 0) {
    // one launch per pass + one for the compaction (pass_fused_k / compact_fused_k above).  Digits of 7 bits: 20-bit ids = 3
    // passes, 130 us at config 3 against 149 for 2 passes of 10 bits (1,024 bins per 4,096-key tile scatter 16-byte runs)
    // Above 28 bits 7-bit digits would take a fifth pass, for which there is neither a bin_total nor a ready word: the digits
    // widen until kMaxPasses hold the key (max_vocab <= 2^30: 4 passes of 8 bits; pass_fused_k holds kMaxBins bins).
    int max_bits = mi::env_int("MI_SORT_BITS", 7);
    Digits D = plan_rows(max_vocab, max_bits);
    while (D.passes > kMaxPasses && max_bits < kMaxBits) D = plan_rows(max_vocab, ++max_bits);
    MI_REQUIRE(D.passes <= kMaxPasses, "sort_unique_fields: %d passes", D.passes);
    int32_t* ready = W.sync;                                       // [pass][field]
    int32_t* hcf = W.sync + static_cast<int64_t>(kMaxPasses) * F;  // [tile]
    int32_t* err = hcf + ntiles;
    zero_i32(W.sync, L.sync_words, st);
    MI_CHECK_LAUNCH("sort_unique_fields(zero)");
    const int32_t* kin = nullptr;
    const int32_t* vin = nullptr;
    const int nap = mi::env_int("MI_SORT_NAP", 1);
    for (int p = 0; p < D.passes; ++p) {
      int32_t* kout = W.kbuf[p & 1];
      int32_t* vout = W.vbuf[p & 1];
      pass_fused_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kin, vin, p == 0 ? ids : nullptr, B, F, D.nbits * p, D.nbits, tps, W.hist,
                                                          ready + static_cast<int64_t>(p) * F, err, kout, vout, nap);
      MI_CHECK_LAUNCH("sort_unique_fields(pass)");
      kin = kout;
      vin = vout;
    }
    compact_fused_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kin, vin, n, hcf, err, sorted_entry, uniq_rows, seg_start, num_uniq, B, field_off);
    MI_CHECK_LAUNCH("sort_unique_fields(compact)");
    return MI_OK;
  }
  // the short launches (hist_fields_k / scatter_runs_k / compact_fields_k above): 3 passes at config 3 = zero + 3 x (hist +
  // scatter) + head count + compact = 9.  The two pair buffers are the key buffers and the value buffers, each pair of
  // them contiguous; the last pass writes keys and values apart into the pair buffer it does not read.
  const Digits D = plan_rows(max_vocab, kMaxBits);
  const int nbins = 1 << D.nbits;
  zero_i32(W.bin_total, static_cast<int64_t>(kMaxPasses) * F * kMaxBins, st);
  MI_CHECK_LAUNCH("sort_unique_fields(zero)");
  static_assert(sizeof(int2) == 8, "pair buffers");
  int2* pbuf[2] = {reinterpret_cast<int2*>(W.kbuf[0]), reinterpret_cast<int2*>(W.vbuf[0])};
  const bool self_offs = static_cast<int64_t>(nbins) * tps <= kSelfOffsMaxInts;
  const int2* pin = nullptr;       // pass 0 reads ids
  int32_t* kout = nullptr;
  int32_t* vout = nullptr;
  for (int p = 0; p < D.passes; ++p) {
    const bool last = p == D.passes - 1;
    int32_t* bt = W.bin_total + static_cast<int64_t>(p) * F * kMaxBins;
    hist_fields_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(pin, p == 0 ? ids : nullptr, B, F, D.nbits * p, nbins, tps, W.hist, bt);
    MI_CHECK_LAUNCH("sort_unique_fields(hist)");
    if (!self_offs) {
      bin_scan_k<<<dim3(F * nbins), dim3(kBlock), 0, st>>>(W.hist, tps, nbins, bt, B);
      MI_CHECK_LAUNCH("sort_unique_fields(scan)");
    }
    kout = last ? (p & 1 ? W.vbuf[0] : W.kbuf[0]) : nullptr;
    vout = last ? (p & 1 ? W.vbuf[1] : W.kbuf[1]) : nullptr;
    if (p == 0)
      scatter_runs_k<true><<<dim3(ntiles), dim3(kBlock), 0, st>>>(nullptr, ids, B, F, 0, D.nbits, tps, W.hist, bt, self_offs ? 1 : 0,
                                                                  last ? nullptr : pbuf[0], kout, vout);
    else
      scatter_runs_k<false><<<dim3(ntiles), dim3(kBlock), 0, st>>>(pin, nullptr, B, F, D.nbits * p, D.nbits, tps, W.hist, bt, self_offs ? 1 : 0,
                                                                   last ? nullptr : pbuf[p & 1], kout, vout);
    MI_CHECK_LAUNCH("sort_unique_fields(scatter)");
    pin = pbuf[p & 1];
  }
  head_count_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kout, n, W.heads, B);
  MI_CHECK_LAUNCH("sort_unique_fields(heads)");
  if (ntiles <= kFoldHeadsMaxTiles) {
    compact_fields_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kout, vout, n, W.heads, sorted_entry, uniq_rows, seg_start, num_uniq, B, field_off);
  } else {
    scan_small_k<<<dim3(1), dim3(kScanSmallBlock), 0, st>>>(W.heads, ntiles);
    MI_CHECK_LAUNCH("sort_unique_fields(scan heads)");
    compact_k<<<dim3(ntiles), dim3(kBlock), 0, st>>>(kout, vout, n, W.heads, sorted_entry, uniq_rows, seg_start, num_uniq, B, field_off);
  }
  MI_CHECK_LAUNCH("sort_unique_fields(compact)");
  return MI_OK;
}

}  // extern "C"

// ---- routing helpers of the row-sharded (multi-GPU) path ------------------------------------
namespace {

// request key of entry i for row r: ((chunk * world + owner) * rows_per_rank + local row); sorting by it
// (mi_sort_unique_rows) orders the entries by (chunk, owner, row) and its unique keys are the DISTINCT rows
// a chunk needs from an owner: a row asked for by many entries of a batch crosses the link once.
// self_rank >= 0: the owners are numbered with the asking rank itself LAST (owner o -> o for o < self, o - 1 for
// o > self, world - 1 for self): a rank's requests to itself then sit at the end of every chunk's run — outside the
// part of the buffers the all-to-all ships, which skips the self piece (its split size is 0).
__global__ __launch_bounds__(kBlock) void shard_keys_k(const int32_t* __restrict__ rows, int64_t n, int world,
                                                       int64_t entries_per_chunk, int64_t rows_per_rank, int self_rank,
                                                       int32_t* __restrict__ keys) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t r = rows[i];
  const int64_t chunk = entries_per_chunk > 0 ? i / entries_per_chunk : 0;
  int o = r % world;
  if (self_rank >= 0) o = o == self_rank ? world - 1 : (o > self_rank ? o - 1 : o);
  keys[i] = static_cast<int32_t>((chunk * world + o) * rows_per_rank + r / world);
}

// per distinct request u: the owner-local row to ask for, and the request counts per (chunk, owner) group.
// The keys are sorted, so a group is one contiguous run: its count is (index of the first key past it) - (index of its
// first key), and only the two threads at a run's ends touch counts[] — O(groups) atomics.  (One atomicAdd per request on
// the group's counter, as this kernel first did, serialises 1.7 M atomics on C x world addresses: 19 ms per step with
// one rank and 4 chunks, measured with bench.py --force-shard.)
__global__ __launch_bounds__(kBlock) void route_requests_k(const int32_t* __restrict__ uniq_keys,
                                                           const int32_t* __restrict__ num_uniq, int64_t rows_per_rank,
                                                           int32_t* __restrict__ send_rows, int32_t* __restrict__ counts) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t U = *num_uniq;
  if (u >= U) return;
  const int64_t key = uniq_keys[u];
  const int64_t grp = key / rows_per_rank;
  send_rows[u] = static_cast<int32_t>(key - grp * rows_per_rank);
  if (u + 1 == U) {
    atomicAdd(counts + grp, static_cast<int32_t>(U));                   // the last run ends at U
  } else {
    const int64_t gn = static_cast<int64_t>(uniq_keys[u + 1]) / rows_per_rank;
    if (gn != grp) {                                                    // run of grp ends, run of gn starts, at u + 1
      atomicAdd(counts + grp, static_cast<int32_t>(u + 1));
      atomicAdd(counts + gn, -static_cast<int32_t>(u + 1));
    }
  }
}

// slot[e] = index of the distinct request that entry e belongs to (binary search of the sorted position in
// seg_start)
__global__ __launch_bounds__(kBlock) void segment_slots_k(const int32_t* __restrict__ seg_start,
                                                          const int32_t* __restrict__ sorted_entry,
                                                          const int32_t* __restrict__ num_uniq, int64_t n,
                                                          int32_t* __restrict__ slot) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= n) return;
  int lo = 0, hi = *num_uniq;                      // largest u with seg_start[u] <= k
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_start[mid] <= k) lo = mid; else hi = mid;
  }
  slot[sorted_entry[k]] = lo;
}

__global__ __launch_bounds__(kBlock) void gather_u32_k(const uint32_t* __restrict__ src,
                                                       const int32_t* __restrict__ idx, int64_t n,
                                                       uint32_t* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}

}  // namespace

extern "C" {

int32_t mi_shard_keys(const int32_t* rows, int64_t n, int32_t world, int64_t entries_per_chunk, int64_t rows_per_rank,
                      int32_t self_rank, int32_t* keys, mi_stream_t stream) {
  MI_REQUIRE(n >= 0 && world > 0 && entries_per_chunk >= 0 && rows_per_rank > 0 && self_rank >= -1 && self_rank < world,
             "shard_keys: n=%lld world=%d self_rank=%d", (long long)n, world, self_rank);
  if (n == 0) return MI_OK;
  MI_REQUIRE(rows && keys, "shard_keys: null buffer");
  const int64_t chunks = entries_per_chunk > 0 ? mi::ceil_div(n, entries_per_chunk) : 1;
  MI_REQUIRE(chunks * world * rows_per_rank <= INT32_MAX, "shard_keys: %lld chunks x %d ranks x %lld rows per rank does not fit an int32 key",
             (long long)chunks, world, (long long)rows_per_rank);
  shard_keys_k<<<dim3((unsigned)mi::ceil_div(n, kBlock)), dim3(kBlock), 0, mi::as_stream(stream)>>>(rows, n, world, entries_per_chunk,
                                                                                                   rows_per_rank, self_rank, keys);
  MI_CHECK_LAUNCH("shard_keys");
  return MI_OK;
}

int32_t mi_route_requests(const int32_t* uniq_keys, const int32_t* num_uniq, int64_t n_max, int64_t rows_per_rank,
                          int32_t n_groups, int32_t* send_rows, int32_t* counts, mi_stream_t stream) {
  MI_REQUIRE(n_max >= 0 && rows_per_rank > 0 && n_groups > 0, "route_requests: n_max=%lld", (long long)n_max);
  MI_REQUIRE(counts, "route_requests: null counts");
  hipStream_t st = mi::as_stream(stream);
  zero_i32(counts, n_groups, st);
  MI_CHECK_LAUNCH("route_requests(zero)");
  if (n_max == 0) return MI_OK;
  MI_REQUIRE(uniq_keys && num_uniq && send_rows, "route_requests: null buffer");
  route_requests_k<<<dim3((unsigned)mi::ceil_div(n_max, kBlock)), dim3(kBlock), 0, st>>>(uniq_keys, num_uniq, rows_per_rank, send_rows, counts);
  MI_CHECK_LAUNCH("route_requests");
  return MI_OK;
}

int32_t mi_segment_slots(const int32_t* seg_start, const int32_t* sorted_entry, const int32_t* num_uniq, int64_t n,
                         int32_t* slot_of_entry, mi_stream_t stream) {
  MI_REQUIRE(n >= 0, "segment_slots: n=%lld", (long long)n);
  if (n == 0) return MI_OK;
  MI_REQUIRE(seg_start && sorted_entry && num_uniq && slot_of_entry, "segment_slots: null buffer");
  segment_slots_k<<<dim3((unsigned)mi::ceil_div(n, kBlock)), dim3(kBlock), 0, mi::as_stream(stream)>>>(seg_start, sorted_entry, num_uniq, n,
                                                                                                      slot_of_entry);
  MI_CHECK_LAUNCH("segment_slots");
  return MI_OK;
}

int32_t mi_gather_u32(const void* src, const int32_t* idx, int64_t n, void* out, mi_stream_t stream) {
  MI_REQUIRE(n >= 0, "gather_u32: n=%lld", (long long)n);
  if (n == 0) return MI_OK;
  MI_REQUIRE(src && idx && out, "gather_u32: null buffer");
  gather_u32_k<<<dim3((unsigned)mi::ceil_div(n, kBlock)), dim3(kBlock), 0, mi::as_stream(stream)>>>(
      static_cast<const uint32_t*>(src), idx, n, static_cast<uint32_t*>(out));
  MI_CHECK_LAUNCH("gather_u32");
  return MI_OK;
}

}  // extern "C"
