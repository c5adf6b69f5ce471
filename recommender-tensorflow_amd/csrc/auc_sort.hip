// Exact AUC and per-group AUC at any evaluation size: the examples SORTED by (group, key, label), then counted
// (mi_auc_sorted_counts, include/mi355x_rec.h).  Same two integers per (member, group) as auc.hip's pair counts — the
// (positive, negative) pairs whose positive scores higher, and those that tie — in O(N log N) instead of O(P N-), from
// labels and groups in the examples' own order: no plan, no host layout.  Integers only after the key is made.
//
// An example is one 64-bit word, group : key32 : label (bits 33.. : 1..32 : 0), the key mi_score_key32's.  Sorted, the
// examples of a group are together, inside it equal keys form a TIE RUN, inside a run the negatives come first.  An
// example whose group lies outside [0, S) becomes (group 0, kNoKey, label 1): no score has that key, so it is a run of its
// own at the end of group 0, and the count takes it for neither class — nothing downstream ever sees a group >= S.
//
// This file owns the word format, the sort's three kernels and entry, and the count.  The histogram, the scans, the ballot
// ranks and the running slots of the sort are radix.h's, shared with sort.hip's int32 sorts.
//
// Per member, per pass of the stable LSD radix sort (digits of up to 9 bits over the 33 + ceil(log2 S) bits in use):
//   word_hist_k     per-tile digit histogram (LDS atomics) -> hist[digit][tile]; pass 0 makes the words on the way
//   digit_scan_k    one workgroup per digit: exclusive scan of its row over the tiles, the row's sum -> bin_total[digit]
//   word_scatter_k  a tile adds up the lower digits' totals itself (512 ints), then the stable scatter by ballot ranks
// No global atomic, so nothing to zero.  Then the count, by head flags and segmented scans (DESIGN.md §19 says why not
// by binary search): with neg(i) = 1 for a negative,
//   eq(i) = the negatives of i's run before i, gt(i) = the negatives of i's group before i, minus eq(i)
// are exclusive sums of neg that restart at run heads and at group heads.
//   tile_runs_k<false>  per tile: does it hold a run / group head, and the negatives after its last one
//   tile_carry_k        ONE workgroup: the segmented scan of those over the tiles -> what a tile inherits
//   tile_runs_k<true>   per tile: gt(i), eq(i) of its positives, summed per group INSIDE the workgroup (another segmented
//                       scan, over the threads) — one 64-bit atomic add per counter for every group the tile touches,
//                       by the thread that holds the group's last example of the tile.  S = 1: two atomics per tile.
// No workgroup waits for another, and none reads what another writes inside a launch.  Integer adds commute: the counts
// do not depend on the digit width, the tile count or timing.
#include "radix.h"
#include "score_key.h"

namespace {

// The tile of this file: the count's kernels hold 16 words per thread, and the workspace and every launch are sized by it.
// The sort's tiles are the same ones (one ntiles for both), so it has to be radix.h's.
constexpr int kBlock = 256;
constexpr int kItems = 16;                 // words per thread per tile
constexpr int kTile = kBlock * kItems;     // 4096
static_assert(kBlock == radix::kBlock && kItems == radix::kItems && kTile == radix::kTile, "the sort and the count share tiles");

// what the sort takes from radix.h
using radix::kWaves; using radix::kMaxBits; using radix::kMaxBins; using radix::digit_of; using radix::tile_digit_hist;
using radix::block_excl_scan_chunked; using radix::digit_excl_scan; using radix::wave_first_slots; using radix::ranked_scatter;
using radix::align_up; using radix::Digits; using radix::plan_digits; using radix::bits_for;

constexpr uint32_t kNoKey = 0xffffffffu;   // the image of no score (score_key.h)

// the examples as the caller holds them: one member's logits, the labels, the groups (NULL: all in group 0)
struct Source {
  const float* z;
  const uint8_t* y;
  const int32_t* g;
  int32_t S;
};

__device__ __forceinline__ uint64_t make_word(const Source& s, int64_t i) {
  const int32_t g = s.g ? s.g[i] : 0;
  if (static_cast<uint32_t>(g) >= static_cast<uint32_t>(s.S)) return (static_cast<uint64_t>(kNoKey) << 1) | 1u;
  return (static_cast<uint64_t>(g) << 33) | (static_cast<uint64_t>(mi_score_key32(s.z[i])) << 1) | (s.y[i] ? 1u : 0u);
}
// the key source of a tile (radix.h): pass 0 makes the words from the examples (RAW), the later passes read them
template <bool RAW>
struct WordKeys {
  const uint64_t* __restrict__ words;
  Source src;
  __device__ __forceinline__ uint64_t at(int64_t i) const { return RAW ? make_word(src, i) : words[i]; }
};

// ---- the sort ------------------------------------------------------------------------------------------------------------
// (no totals by atomics here: digit_scan_k has every row's sum anyway)
template <bool RAW>
__global__ __launch_bounds__(kBlock) void word_hist_k(const uint64_t* __restrict__ words, Source src, int64_t n, int shift, int nbins,
                                                      int ntiles, int32_t* __restrict__ hist) {
  tile_digit_hist(WordKeys<RAW>{words, src}, n, shift, nbins, ntiles, hist, nullptr);
}

// block b: hist[b, 0..ntiles) -> its exclusive scan (a tile's offset inside digit b), the row's sum -> bin_total[b]
__global__ __launch_bounds__(kBlock) void digit_scan_k(int32_t* __restrict__ hist, int ntiles, int32_t* __restrict__ bin_total) {
  int32_t* row = hist + static_cast<int64_t>(blockIdx.x) * ntiles;
  const int total = block_excl_scan_chunked<kBlock>(ntiles, 0, [&](int i) { return row[i]; }, [&](int i, int excl, int) { row[i] = excl; });
  if (threadIdx.x == 0) bin_total[blockIdx.x] = total;
}

// The stable scatter of a tile of words (no values): the waves count their digits, every wave derives its own running
// slots — the digit's base (the sum of the lower digits' totals, scanned here) + the tile's offset inside the digit + the
// counts of the waves before it — and scatters its 16 rounds alone, lanes finding their equal-digit peers with ballots.
template <bool RAW>
__global__ __launch_bounds__(kBlock) void word_scatter_k(const uint64_t* __restrict__ words, Source src, int64_t n, int shift, int nbits,
                                                         int ntiles, const int32_t* __restrict__ offs,
                                                         const int32_t* __restrict__ bin_total, uint64_t* __restrict__ out) {
  __shared__ int32_t running[kWaves][kMaxBins];    // per wave: digit counts, then the next output slot of each digit
  __shared__ int32_t dbase[kMaxBins];              // first slot of a digit in the whole array
  __shared__ int32_t wsum[kWaves];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nbins = 1 << nbits;
  for (int b = t; b < kWaves * kMaxBins; b += kBlock) (&running[0][0])[b] = 0;
  __syncthreads();
  const WordKeys<RAW> keys{words, src};
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kTile + w * (64 * kItems) + lane;
  uint64_t key[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * 64;
    const bool valid = i < n;
    key[r] = valid ? keys.at(i) : 0;
    if (valid) atomicAdd(&running[w][digit_of(key[r], shift, nbins - 1)], 1);
  }
  digit_excl_scan<1>(
      nbins, wsum, [&](int b, int (&c)[1]) { c[0] = bin_total[b]; }, [&](int b, int, const int (&pre)[1]) { dbase[b] = pre[0]; });
  __syncthreads();
  wave_first_slots(running, running, nbins, [&](int b) { return dbase[b] + offs[static_cast<int64_t>(b) * ntiles + blockIdx.x]; });
  ranked_scatter<true>(key, shift, nbits, running[w], base, n, [&](int32_t dst, int r) { out[dst] = key[r]; });
}

// ---- the count -----------------------------------------------------------------------------------------------------------
// A segmented sum: f = a segment starts somewhere in the range, v = the sum after the last start (of everything without one)
template <typename T>
struct Seg {
  int f;
  T v;
};
template <typename T>
__device__ __forceinline__ Seg<T> seg_join(Seg<T> a, Seg<T> b) {   // a's range before b's
  return Seg<T>{a.f | b.f, b.f ? b.v : a.v + b.v};
}

// The exclusive segmented scan over the threads of the workgroup (thread t holds (f, v) of its own range): the join of the
// threads before t; *total, where asked for, the join of all.  Every thread calls it; scratch: four entries of LDS.
template <typename T>
__device__ __forceinline__ Seg<T> block_seg_excl(int f, T v, Seg<T>* scratch, Seg<T>* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int f2 = __shfl_up(f, off, 64);
    const T v2 = __shfl_up(v, off, 64);
    if (lane >= off) {
      if (!f) v += v2;
      f |= f2;
    }
  }
  __syncthreads();                       // the previous call's scratch fully consumed
  if (lane == 63) scratch[w] = Seg<T>{f, v};
  __syncthreads();
  Seg<T> mine{__shfl_up(f, 1, 64), __shfl_up(v, 1, 64)};
  if (lane == 0) mine = Seg<T>{0, 0};
  Seg<T> before{0, 0};
  for (int ww = 0; ww < w; ++ww) before = seg_join(before, scratch[ww]);
  if (total) {
    Seg<T> all{0, 0};
    for (int ww = 0; ww < kBlock / 64; ++ww) all = seg_join(all, scratch[ww]);
    *total = all;
  }
  return seg_join(before, mine);
}

// What a tile hands on (tile_runs_k<false>) and what it inherits (tile_carry_k): x, y = a run head in it / the negatives
// after its last run head; z, w = the same for group heads.  carry[tile]: x = the negatives of the run, y = of the group,
// that the tile's first example continues.
__device__ __forceinline__ uint64_t run_of(uint64_t word) { return word >> 1; }     // (group, key)
__device__ __forceinline__ uint32_t group_of(uint64_t word) { return static_cast<uint32_t>(word >> 33); }

// Thread t owns words [t * 16, t * 16 + 16) of its tile, in registers.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) void tile_runs_k(const uint64_t* __restrict__ words, int64_t n, int4* __restrict__ summary,
                                                      const int2* __restrict__ carry, int32_t S,
                                                      unsigned long long* __restrict__ counts) {
  __shared__ Seg<int> si[kBlock / 64];
  __shared__ Seg<long long> sl[kBlock / 64];
  const int t = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kTile + t * kItems;
  uint64_t x[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) x[j] = i0 + j < n ? words[i0 + j] : 0;
  const int have = n - i0 >= kItems ? kItems : (n > i0 ? static_cast<int>(n - i0) : 0);      // the thread's words that exist
  // head flags, one bit per word: a run / a group starts here (a group head is a run head: the run includes the group)
  unsigned int run_head = 0, grp_head = 0;
  {
    const bool first = i0 == 0;
    const uint64_t prev = (i0 > 0 && have > 0) ? words[i0 - 1] : 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const uint64_t p = j ? x[j - 1] : prev;
      if (j < have) {
        if ((j == 0 && first) || run_of(x[j]) != run_of(p)) run_head |= 1u << j;
        if ((j == 0 && first) || group_of(x[j]) != group_of(p)) grp_head |= 1u << j;
      }
    }
  }
  // the negatives after the thread's last run head / group head
  int fa = 0, ta = 0, fb = 0, tb = 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    if ((run_head >> j) & 1u) { fa = 1; ta = 0; }
    if ((grp_head >> j) & 1u) { fb = 1; tb = 0; }
    const int neg = (j < have && !(x[j] & 1u)) ? 1 : 0;
    ta += neg;
    tb += neg;
  }
  Seg<int> all_a, all_b;
  Seg<int> ca = block_seg_excl<int>(fa, ta, si, &all_a);
  Seg<int> cb = block_seg_excl<int>(fb, tb, si, &all_b);
  if (!COUNT) {
    if (t == 0) summary[blockIdx.x] = make_int4(all_a.f, all_a.v, all_b.f, all_b.v);
    return;
  }
  const int2 inherited = carry[blockIdx.x];
  if (!ca.f) ca.v += inherited.x;
  if (!cb.f) cb.v += inherited.y;
  // does the group of the thread's last word end there (inside this tile)?
  bool last_ends = true;
  if (have == kItems && t < kBlock - 1 && i0 + kItems < n) last_ends = group_of(words[i0 + kItems]) != group_of(x[kItems - 1]);
  // pass 0: the thread's sums of gt / eq after its last group head; pass 1, with what the threads before it hand on: the
  // same walk, adding a group's sums to its counters where the group ends
  long long open_gt = 0, open_eq = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int ra = ca.v, rb = cb.v;
    long long gt = open_gt, eq = open_eq;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      if ((run_head >> j) & 1u) ra = 0;
      if ((grp_head >> j) & 1u) { rb = 0; gt = 0; eq = 0; }
      if (j < have) {
        const bool label = x[j] & 1u;
        if (label && static_cast<uint32_t>(x[j] >> 1) != kNoKey) {       // a positive: rb negatives of its group lie before it,
          gt += rb - ra;                                                  // ra of them in its own run
          eq += ra;
        }
        if (!label) { ++ra; ++rb; }
        if (pass == 1) {
          const bool ends = j + 1 < kItems ? (j + 1 >= have || ((grp_head >> (j + 1)) & 1u)) : last_ends;
          const uint32_t g = group_of(x[j]);
          if (ends && g < static_cast<uint32_t>(S)) {
            if (gt) atomicAdd(counts + static_cast<int64_t>(g) * 2, static_cast<unsigned long long>(gt));
            if (eq) atomicAdd(counts + static_cast<int64_t>(g) * 2 + 1, static_cast<unsigned long long>(eq));
          }
        }
      }
    }
    if (pass == 0) {
      const Seg<long long> cg = block_seg_excl<long long>(grp_head != 0, gt, sl, nullptr);
      const Seg<long long> ce = block_seg_excl<long long>(grp_head != 0, eq, sl, nullptr);
      open_gt = cg.v;                       // (no head in the threads before: their whole sum — the tile starts from 0)
      open_eq = ce.v;
    }
  }
}

// ONE workgroup: carry[tile] = the exclusive segmented scan of the tiles' summaries
__global__ __launch_bounds__(kBlock) void tile_carry_k(const int4* __restrict__ summary, int ntiles, int2* __restrict__ carry) {
  __shared__ Seg<int> si[kBlock / 64];
  Seg<int> run_a{0, 0}, run_b{0, 0};
  for (int c0 = 0; c0 < ntiles; c0 += kBlock) {
    const int i = c0 + static_cast<int>(threadIdx.x);
    const int4 s = i < ntiles ? summary[i] : make_int4(0, 0, 0, 0);
    Seg<int> all_a, all_b;
    const Seg<int> ea = block_seg_excl<int>(s.x, s.y, si, &all_a);
    const Seg<int> eb = block_seg_excl<int>(s.z, s.w, si, &all_b);
    if (i < ntiles) carry[i] = make_int2(seg_join(run_a, ea).v, seg_join(run_b, eb).v);
    run_a = seg_join(run_a, all_a);
    run_b = seg_join(run_b, all_b);
  }
}

struct Layout {
  int64_t ntiles, wordsA, wordsB, hist, bin_total, summary, carry, bytes;
};

Layout layout_for(int64_t n) {
  Layout L;
  L.ntiles = mi::ceil_div(n, kTile);
  int64_t o = 0;
  L.wordsA = o; o += align_up(n * 8, 256);
  L.wordsB = o; o += align_up(n * 8, 256);
  L.hist = o; o += align_up(L.ntiles * kMaxBins * 4, 256);
  L.bin_total = o; o += kMaxBins * 4;
  L.summary = o; o += align_up(L.ntiles * 16, 256);
  L.carry = o; o += align_up(L.ntiles * 8, 256);
  L.bytes = o;
  return L;
}

bool sizes_ok(int64_t N, int32_t n_groups) { return N >= 1 && N <= INT32_MAX && n_groups >= 1; }

}  // namespace

extern "C" {

size_t mi_auc_sorted_workspace_bytes(int64_t N, int32_t n_groups) {
  return sizes_ok(N, n_groups) ? static_cast<size_t>(layout_for(N).bytes) : 0;
}

int32_t mi_auc_sorted_counts(const float* logits, int64_t member_stride, int32_t n_members, const uint8_t* labels,
                             const int32_t* groups, int32_t n_groups, int64_t N, int64_t* counts, void* workspace,
                             size_t workspace_bytes, mi_stream_t stream) {
  MI_REQUIRE(logits && labels && counts && workspace, "auc_sorted_counts: logits / labels / counts / workspace");
  MI_REQUIRE(N >= 1 && N <= INT32_MAX, "auc_sorted_counts: N=%lld examples (1 to %d)", (long long)N, INT32_MAX);
  MI_REQUIRE(n_groups >= 1, "auc_sorted_counts: %d groups (at least 1)", n_groups);
  MI_REQUIRE(groups || n_groups == 1, "auc_sorted_counts: groups is NULL with %d groups (NULL: one group)", n_groups);
  MI_REQUIRE(n_members >= 1 && n_members <= MI_AUC_MAX_MEMBERS, "auc_sorted_counts: %d members (1 to %d)", n_members,
             MI_AUC_MAX_MEMBERS);
  MI_REQUIRE(member_stride >= N, "auc_sorted_counts: member_stride=%lld below N=%lld", (long long)member_stride, (long long)N);
  const Layout L = layout_for(N);
  if (workspace_bytes < static_cast<size_t>(L.bytes)) {
    mi::set_error("auc_sorted_counts: workspace of %zu bytes, %lld needed", workspace_bytes, (long long)L.bytes);
    return MI_ERR_WORKSPACE;
  }
  MI_REQUIRE(mi::aligned16(workspace), "auc_sorted_counts: workspace (16-byte aligned)");
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  uint64_t* buf[2] = {reinterpret_cast<uint64_t*>(ws + L.wordsA), reinterpret_cast<uint64_t*>(ws + L.wordsB)};
  int32_t* hist = reinterpret_cast<int32_t*>(ws + L.hist);
  int32_t* bin_total = reinterpret_cast<int32_t*>(ws + L.bin_total);
  int4* summary = reinterpret_cast<int4*>(ws + L.summary);
  int2* carry = reinterpret_cast<int2*>(ws + L.carry);
  const int ntiles = static_cast<int>(L.ntiles);

  // the bits in use: label, key, and the group's ceil(log2 S); digits of equal width, at most 9 bits (S = 1: 4 passes of 9)
  const Digits D = plan_digits(33 + bits_for(n_groups, 31), mi::env_int("MI_AUC_SORT_BITS", kMaxBits));
  const int passes = D.passes, nbits = D.nbits, nbins = 1 << nbits;

  for (int32_t m = 0; m < n_members; ++m) {
    const Source src{logits + static_cast<int64_t>(m) * member_stride, labels, groups, n_groups};
    const uint64_t* in = nullptr;               // pass 0 makes the words from the examples
    for (int p = 0; p < passes; ++p) {
      uint64_t* out = buf[p & 1];
      if (p == 0) word_hist_k<true><<<dim3(ntiles), dim3(kBlock), 0, st>>>(in, src, N, 0, nbins, ntiles, hist);
      else word_hist_k<false><<<dim3(ntiles), dim3(kBlock), 0, st>>>(in, src, N, nbits * p, nbins, ntiles, hist);
      MI_CHECK_LAUNCH("auc_sorted_counts(hist)");
      digit_scan_k<<<dim3(nbins), dim3(kBlock), 0, st>>>(hist, ntiles, bin_total);
      MI_CHECK_LAUNCH("auc_sorted_counts(scan)");
      if (p == 0) word_scatter_k<true><<<dim3(ntiles), dim3(kBlock), 0, st>>>(in, src, N, 0, nbits, ntiles, hist, bin_total, out);
      else word_scatter_k<false><<<dim3(ntiles), dim3(kBlock), 0, st>>>(in, src, N, nbits * p, nbits, ntiles, hist, bin_total, out);
      MI_CHECK_LAUNCH("auc_sorted_counts(scatter)");
      in = out;
    }
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts) + static_cast<int64_t>(m) * n_groups * 2;
    tile_runs_k<false><<<dim3(ntiles), dim3(kBlock), 0, st>>>(in, N, summary, nullptr, n_groups, nullptr);
    MI_CHECK_LAUNCH("auc_sorted_counts(tile runs)");
    tile_carry_k<<<dim3(1), dim3(kBlock), 0, st>>>(summary, ntiles, carry);
    MI_CHECK_LAUNCH("auc_sorted_counts(carry)");
    tile_runs_k<true><<<dim3(ntiles), dim3(kBlock), 0, st>>>(in, N, nullptr, carry, n_groups, c);
    MI_CHECK_LAUNCH("auc_sorted_counts(count)");
  }
  return MI_OK;
}

}  // extern "C"
