// Exact AUC and per-group AUC of every member of a population: the pairs (positive, negative) of a group whose positive
// scores higher, and those that tie, COUNTED (mi_auc_plan / mi_auc_pair_counts, include/mi355x_rec.h).  AUC =
// (2 gt + eq) / (2 P N-) is formed on the host from the two integers; nothing here is a float after the key is made.
//
// The host describes an evaluation set once, for all members: `order`, a permutation of the examples that is segment
// major with each segment's negatives first, and per segment its offset and its number of negatives.  mi_auc_plan cuts
// every segment that has both classes into work items (segment, a tile of at most 64 positives, a run of at most C
// negatives) and leaves the item table on the device.
//
//   auc_pair_counts_k  grid (ceil(items / 4), members), one WAVE per item.  Lane l holds the key of the tile's l-th
//                      positive (gathered through `order`); the wave loads 64 negatives' keys at a time, one per lane,
//                      and hands them round with v_readlane (a uniform lane index: no LDS); every lane does two compares
//                      and two adds per negative.  The lanes' 32-bit counters are summed in the wave and lane 0 adds the
//                      two sums to counts[member, segment, 0..1] with 64-bit integer atomics (a zero sum is not sent).
//
// Integers only, and integer adds commute: the counts do not depend on C, on the grid or on timing.  No workgroup reads
// what another writes, none waits for another, there is no LDS and no barrier.  Lanes past the tile's positives and
// negatives past the run's end carry keys that count nothing — every lane reaches every cross-lane operation.
#include "common.h"
#include "score_key.h"

#include <memory>
#include <new>

namespace {

constexpr int kWaves = 4;                       // items per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kTile = 64;                       // positives per item: one per lane
constexpr int kRun = 2048;                      // negatives per item, the built-in C
constexpr int kMaxRun = 1 << 24;                // 64 lanes x C compares stay inside the wave's 32-bit sums
constexpr int64_t kMaxItems = 1 << 24;          // the item table stays below 512 MB
constexpr uint64_t kPlanMagic = 0x6d695f6175635f31ull;   // "mi_auc_1"
constexpr uint32_t kNoKey = 0xffffffffu;        // the image of no score (score_key.h): neither above nor equal to any key

struct Item {
  int32_t seg;                                  // the segment the counts belong to
  int32_t pos0, npos;                           // positions [pos0, pos0 + npos) of `order`: the tile's positives
  int32_t neg0, nneg;                           // positions [neg0, neg0 + nneg): the run's negatives
  int32_t pad[3];
};
static_assert(sizeof(Item) == 32, "items are read as eight words");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void auc_pair_counts_k(const Item* __restrict__ items, int32_t n_items,
                                                              const float* __restrict__ logits, int64_t member_stride,
                                                              const int32_t* __restrict__ order, int32_t n_segments,
                                                              unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));   // (uniform: the item lives in SGPRs)
  const int64_t it = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  const bool live = it < n_items;
  const Item I = items[live ? it : 0];
  const int npos = live ? I.npos : 0, nneg = live ? I.nneg : 0;
  const float* __restrict__ z = logits + static_cast<int64_t>(blockIdx.y) * member_stride;

  const bool has = lane < npos;
  const uint32_t kp = has ? mi_score_key32(z[order[I.pos0 + lane]]) : 0u;
  uint32_t gt = 0, eq = 0;
  for (int j0 = 0; j0 < nneg; j0 += 64) {
    const int j = j0 + lane;
    const uint32_t kn = j < nneg ? mi_score_key32(z[order[I.neg0 + j]]) : kNoKey;
    const int cnt = nneg - j0 < 64 ? nneg - j0 : 64;
    for (int l0 = 0; l0 < cnt; l0 += 8) {       // (a group of 8 may run past cnt: those lanes hold kNoKey)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t n = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(kn), l0 + u));
        gt += kp > n ? 1u : 0u;
        eq += kp == n ? 1u : 0u;
      }
    }
  }
  gt = wave_sum(has ? gt : 0u);                 // (a lane without a positive compared key 0: its counts are dropped)
  eq = wave_sum(has ? eq : 0u);
  if (lane == 0 && live) {
    unsigned long long* c = counts + (static_cast<int64_t>(blockIdx.y) * n_segments + I.seg) * 2;
    if (gt) atomicAdd(c, static_cast<unsigned long long>(gt));
    if (eq) atomicAdd(c + 1, static_cast<unsigned long long>(eq));
  }
}

// The checks of a layout and the number of items it yields (-1: refused, the error is set)
int64_t count_items(const char* who, const int64_t* seg_off, const int64_t* seg_neg, int32_t n_segments, int32_t neg_run,
                    int32_t& run) {
  if (!seg_off || !seg_neg) {
    mi::set_error("%s: seg_off / seg_neg", who);
    return -1;
  }
  if (n_segments < 1) {
    mi::set_error("%s: %d segments (at least 1)", who, n_segments);
    return -1;
  }
  if (neg_run < 0 || neg_run > kMaxRun) {
    mi::set_error("%s: neg_run=%d (0 = the built-in choice, at most %d)", who, neg_run, kMaxRun);
    return -1;
  }
  run = neg_run ? neg_run : kRun;
  if (seg_off[0] != 0) {
    mi::set_error("%s: seg_off[0]=%lld (the segments ascend from 0 to N)", who, (long long)seg_off[0]);
    return -1;
  }
  int64_t items = 0;
  for (int32_t s = 0; s < n_segments; ++s) {
    const int64_t n = seg_off[s + 1] - seg_off[s], neg = seg_neg[s];
    if (n < 0) {
      mi::set_error("%s: seg_off[%d]=%lld after seg_off[%d]=%lld (the segments ascend from 0 to N)", who, s + 1,
                    (long long)seg_off[s + 1], s, (long long)seg_off[s]);
      return -1;
    }
    if (seg_off[s + 1] > INT32_MAX) {
      mi::set_error("%s: N=%lld examples (1 to %d)", who, (long long)seg_off[s + 1], INT32_MAX);
      return -1;
    }
    if (neg < 0 || neg > n) {
      mi::set_error("%s: seg_neg[%d]=%lld negatives in a segment of %lld examples", who, s, (long long)neg, (long long)n);
      return -1;
    }
    if (neg > 0 && neg < n) {
      items += mi::ceil_div(n - neg, kTile) * mi::ceil_div(neg, run);
      if (items > kMaxItems) {
        mi::unsupported("%s: more than %lld work items (the entry is meant for the held-out sets of sweeps)", who,
                        (long long)kMaxItems);
        return -2;
      }
    }
  }
  if (seg_off[n_segments] < 1) {
    mi::set_error("%s: N=%lld examples (1 to %d)", who, (long long)seg_off[n_segments], INT32_MAX);
    return -1;
  }
  return items;
}

}  // namespace

extern "C" {

size_t mi_auc_plan_bytes(const int64_t* seg_off, const int64_t* seg_neg, int32_t n_segments, int32_t neg_run) {
  int32_t run = 0;
  const int64_t items = count_items("auc_plan_bytes", seg_off, seg_neg, n_segments, neg_run, run);
  return items < 0 ? 0 : sizeof(Item) * static_cast<size_t>(items > 0 ? items : 1);
}

int32_t mi_auc_plan(const int64_t* seg_off, const int64_t* seg_neg, int32_t n_segments, int32_t neg_run, void* device_table,
                    size_t device_table_bytes, mi_auc_plan_t* plan, mi_stream_t stream) {
  MI_REQUIRE(plan, "auc_plan: plan");
  int32_t run = 0;
  const int64_t items = count_items("auc_plan", seg_off, seg_neg, n_segments, neg_run, run);
  if (items < 0) return items == -2 ? MI_ERR_UNSUPPORTED : MI_ERR_INVALID;
  const size_t need = sizeof(Item) * static_cast<size_t>(items > 0 ? items : 1);
  MI_REQUIRE(device_table, "auc_plan: device_table");
  if (device_table_bytes < need) {
    mi::set_error("auc_plan: device table of %zu bytes, %zu needed", device_table_bytes, need);
    return MI_ERR_WORKSPACE;
  }
  MI_REQUIRE(mi::aligned16(device_table), "auc_plan: device_table (16-byte aligned)");
  if (items > 0) {
    const std::unique_ptr<Item[]> tab(new (std::nothrow) Item[items]);
    MI_REQUIRE(tab, "auc_plan: out of host memory");
    int64_t k = 0;
    for (int32_t s = 0; s < n_segments; ++s) {
      const int64_t off = seg_off[s], neg = seg_neg[s], pos = seg_off[s + 1] - off - neg;
      if (neg < 1 || pos < 1) continue;
      for (int64_t p0 = 0; p0 < pos; p0 += kTile)
        for (int64_t n0 = 0; n0 < neg; n0 += run) {
          Item& I = tab[k++];
          I.seg = s;
          I.pos0 = static_cast<int32_t>(off + neg + p0);
          I.npos = static_cast<int32_t>(pos - p0 < kTile ? pos - p0 : kTile);
          I.neg0 = static_cast<int32_t>(off + n0);
          I.nneg = static_cast<int32_t>(neg - n0 < run ? neg - n0 : run);
          I.pad[0] = I.pad[1] = I.pad[2] = 0;
        }
    }
    const int32_t rc = mi::upload_table(device_table, tab.get(), sizeof(Item) * static_cast<size_t>(items), stream, "auc_plan");
    if (rc != MI_OK) return rc;
  }
  plan->device_table = device_table; plan->N = seg_off[n_segments]; plan->n_segments = n_segments;
  plan->n_items = static_cast<int32_t>(items);
  plan->magic = kPlanMagic;
  return MI_OK;
}

int32_t mi_auc_pair_counts(const mi_auc_plan_t* plan, const float* logits, int64_t member_stride, int32_t n_members,
                           const int32_t* order, int64_t* counts, mi_stream_t stream) {
  MI_REQUIRE(plan && plan->magic == kPlanMagic && plan->device_table, "auc_pair_counts: plan (not written by mi_auc_plan)");
  MI_REQUIRE(plan->N >= 1 && plan->N <= INT32_MAX && plan->n_segments >= 1 && plan->n_items >= 0 && plan->n_items <= kMaxItems,
             "auc_pair_counts: plan (damaged)");
  MI_REQUIRE(logits && order && counts, "auc_pair_counts: logits / order / counts");
  MI_REQUIRE(n_members >= 1 && n_members <= MI_AUC_MAX_MEMBERS, "auc_pair_counts: %d members (1 to %d)", n_members,
             MI_AUC_MAX_MEMBERS);
  MI_REQUIRE(member_stride >= plan->N, "auc_pair_counts: member_stride=%lld below N=%lld", (long long)member_stride,
             (long long)plan->N);
  if (plan->n_items == 0) return MI_OK;         // (no segment has both classes: every count stays as it is)
  const unsigned blocks = static_cast<unsigned>(mi::ceil_div(plan->n_items, kWaves));
  auc_pair_counts_k<<<dim3(blocks, n_members), dim3(kThreads), 0, mi::as_stream(stream)>>>(
      static_cast<const Item*>(plan->device_table), plan->n_items, logits, member_stride, order, plan->n_segments,
      reinterpret_cast<unsigned long long*>(counts));
  MI_CHECK_LAUNCH("auc_pair_counts");
  return MI_OK;
}

}  // extern "C"
