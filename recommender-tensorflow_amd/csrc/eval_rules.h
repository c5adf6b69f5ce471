// The streaming eval counters of mi_eval_accumulate (include/mi355x_rec.h), defined once: tf.metrics.auc's
// thresholds, the bucket an example falls into, the class rule of model_utils.py:12 and the fp64 terms of the three sums.
// head.hip (eval_accumulate_k, logits from memory) and train_fused.hip (eval_fused_group_k, logits from the fused forward)
// count with these, into LDS arrays laid out the same way, so the two give the same integers for the same logits.
#pragma once
#include "common.h"

constexpr int kAucThresholds = 200;                 // tf.metrics.auc default num_thresholds
constexpr int kEvalHist = 2 * (kAucThresholds + 1); // hist[y][k]: label y, sigmoid above exactly k thresholds
constexpr int kEvalCounts = 8;                      // n, n_pos, n_pred_pos, n_correct, tp@.5, fp@.5, fn@.5, (unused)

// threshold j of the 200, ascending (tf.metrics.auc: kepsilon = 1e-7 outside [0, 1])
__device__ __forceinline__ float mi_auc_threshold(int j) {
  if (j == 0) return static_cast<float>(0.0 - 1e-7);
  if (j == kAucThresholds - 1) return static_cast<float>(1.0 + 1e-7);
  return static_cast<float>(static_cast<double>(j) * 1.0 / static_cast<double>(kAucThresholds - 1));
}

// fills th [kAucThresholds] and zeroes lh [kEvalHist] and lc [kEvalCounts] (LDS) with `threads` threads; the caller barriers
__device__ __forceinline__ void mi_eval_init(float* th, unsigned int* lh, unsigned int* lc, int tid, int threads) {
  for (int j = tid; j < kAucThresholds; j += threads) th[j] = mi_auc_threshold(j);
  for (int j = tid; j < kEvalHist; j += threads) lh[j] = 0;
  if (tid < kEvalCounts) lc[tid] = 0;
}

// k = #{j : th[j] < p} (thresholds ascending => "p > th[j]" <=> j < k)
__device__ __forceinline__ int mi_auc_bucket(const float* th, float p) {
  int lo = 0, hi = kAucThresholds;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (th[mid] < p) lo = mid + 1; else hi = mid; }
  return lo;
}

// one example (logit x, label y in {0, 1}) into the LDS counters; adds its fp64 terms to sl (loss), sp (sigmoid), sy (label)
__device__ __forceinline__ void mi_eval_count(float x, int y, const float* th, unsigned int* lh, unsigned int* lc, double& sl,
                                              double& sp, double& sy) {
  const float p = mi_sigmoid_stable(x);
  atomicAdd(&lh[y * (kAucThresholds + 1) + mi_auc_bucket(th, p)], 1u);
  const int cls = p > 0.5f ? 1 : 0;       // model_utils.py:12
  atomicAdd(&lc[0], 1u);
  if (y) atomicAdd(&lc[1], 1u);
  if (cls) atomicAdd(&lc[2], 1u);
  if (cls == y) atomicAdd(&lc[3], 1u);
  if (cls && y) atomicAdd(&lc[4], 1u);
  if (cls && !y) atomicAdd(&lc[5], 1u);
  if (!cls && y) atomicAdd(&lc[6], 1u);
  const double xd = x;
  sl += fmax(xd, 0.0) - xd * y + log1p(exp(-fabs(xd)));
  sp += p; sy += y;
}

// the workgroup's LDS counters into the caller-zeroed global arrays: integer atomics, order independent; the caller barriers first
__device__ __forceinline__ void mi_eval_flush(const unsigned int* lh, const unsigned int* lc, unsigned long long* hist,
                                              unsigned long long* counts, int tid, int threads) {
  for (int j = tid; j < kEvalHist; j += threads) {
    const unsigned int v = lh[j];
    if (v) atomicAdd(&hist[j], static_cast<unsigned long long>(v));
  }
  if (tid < 7 && lc[tid]) atomicAdd(&counts[tid], static_cast<unsigned long long>(lc[tid]));
}
