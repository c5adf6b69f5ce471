// The optimizers' update rules, one definition for every translation unit that applies them (optim.hip: the dense and
// sparse applies and the lazy catch-up; train_fused.hip: the one-launch train step).  Both are compiled with
// -ffp-contract=off: each expression below is written in the order of TF's Eigen expressions, one rounding per
// operation, so fp32 results equal the numpy oracle's (oracle/optimizers.py) bit for bit given equal gradients.
// Update rules: SURVEY Appendix A.6/A.7.
#pragma once
#include "common.h"

namespace {

struct Hp {
  int kind;
  float lr, beta1, beta2, eps, lr_t, decay, momentum, lr_power, l1, l2;
};

Hp make_hp(const mi_opt_hparams* h) {
  return Hp{h->kind, h->lr, h->beta1, h->beta2, h->epsilon, h->lr_t, h->decay, h->momentum,
            h->lr_power, h->l1, h->l2};
}

// one element of a dense variable (training_ops.cc Apply* functors)
__device__ __forceinline__ void dense_rule(const Hp& h, float& w, float& s0, float& s1, float g) {
  switch (h.kind) {
    case MI_OPT_ADAM: {
      s0 = s0 + (g - s0) * (1.f - h.beta1);
      s1 = s1 + (g * g - s1) * (1.f - h.beta2);
      w = w - (s0 * h.lr_t) / (sqrtf(s1) + h.eps);
    } break;
    case MI_OPT_ADAGRAD: {
      s0 = s0 + g * g;
      w = w - (g * h.lr) * (1.f / sqrtf(s0));
    } break;
    case MI_OPT_FTRL: {
      const float na = s0 + g * g;
      s1 = s1 + (g - ((sqrtf(na) - sqrtf(s0)) / h.lr) * w);
      const float adj = fminf(fmaxf(s1, -h.l1), h.l1);
      w = (adj - s1) / (sqrtf(na) / h.lr + 2.f * h.l2);
      s0 = na;
    } break;
    case MI_OPT_RMSPROP: {
      s0 = s0 + (g * g - s0) * (1.f - h.decay);
      s1 = s1 * h.momentum + (g * h.lr) / sqrtf(s0 + h.eps);
      w = w - s1;
    } break;
    default:
      w = w - g * h.lr;
  }
}

// one element of a TOUCHED row of a sparse variable.  Adam: adam.py _apply_sparse_shared
// (m*beta1 then scatter_add); the others act on touched rows exactly like the dense rule.
__device__ __forceinline__ void sparse_rule(const Hp& h, float& w, float& s0, float& s1, float g) {
  if (h.kind == MI_OPT_ADAM) {
    s0 = s0 * h.beta1 + g * (1.f - h.beta1);
    s1 = s1 * h.beta2 + (g * g) * (1.f - h.beta2);
    w = w - (h.lr_t * s0) / (sqrtf(s1) + h.eps);
  } else {
    dense_rule(h, w, s0, s1, g);
  }
}

// One step of TF Adam's whole-table sweep on an element of a row the step's batch does not touch (g = 0 in
// _apply_sparse_shared: SURVEY Appendix A.6).
__device__ __forceinline__ void replay_step(float& w, float& m, float& v, float lr_t, float b1, float b2, float eps) {
  m = m * b1;
  v = v * b2;
  w = w - (lr_t * m) / (sqrtf(v) + eps);
}

// Lazy replay of that sweep for the steps a row sat out.
__device__ __forceinline__ void replay(float& w, float& m, float& v, int s_from, int s_to,
                                       const float* __restrict__ lr_table, float b1, float b2,
                                       float eps) {
  for (int s = s_from; s <= s_to; ++s) replay_step(w, m, v, lr_table[s], b1, b2, eps);
}

}  // namespace
