// Training small models: one whole optimizer.minimize(loss) of a DeepFM — gather, wide part, FM term, MLP forward with
// dropout, sigmoid-CE head, full backward, dense Adam and TF's dense-equivalent sparse Adam — as ONE launch
// (mi_train_step_fused, include/mi355x_rec.h).  Replaces, for a model whose state fits the chip's caches, what
// trainers/deep_fm.py:36-125 and model_utils.py:57-72 have TensorFlow execute per step.  mi_train_step_model is the same
// launch under any of the five optimizers of optim_rules.h, with a second rule for the wide part (trainers/linear_deep.py:
// 32-39), slots a rule does not keep left out, and the wide part on a subset of the columns (struct Args below).
//
//   train_fused_k    block 0 = the BATCH workgroup, blocks 1 .. G-1 = SWEEP workgroups.
//     batch   everything that depends on the loss, phases separated by workgroup barriers:
//       0. rows     field_off[f] + ids[b, f] into LDS
//       1. forward  sumv and the FM term (products rounded one by one: a one-field model gives exactly 0), the wide sum
//                   and layer 1 straight from the gathered table rows; then one phase per later layer, outputs
//                   (after activation and dropout) in LDS.  Numeric column j (deep_fm.py:59-74) is one more row of the
//                   concat, x[b, j] V[j, :], behind the F gathered ones: recomputed from x_num and numeric_embeddings
//                   wherever it is read (sumv / FM term, layer 1, the gradients), never stored; the wide sum takes
//                   x[b, j] w_num[j] after the categorical weights
//       2. head     logit = ((lin + bias) + fm) + dnn, loss, dlogit
//       3. backward per layer, top down: the weight and bias gradient into the dense-gradient workspace, then the
//                   data gradient IN PLACE over the layer's input (the activation's derivative is taken from the
//                   stored output, the dropout mask from its zeros); layer 1's data gradient is d_concat; then the
//                   numeric columns' gradients, each summed over b ascending by one thread: dV[j, e] and dw_num[j]
//       4. apply    per DISTINCT touched row (the first entry of a row leads; entries of a row are summed in
//                   ascending entry order) sparse_rule on the table record and the wide record, stamp = step;
//                   dense_rule on every dense variable with the gradient of phase 3 (numeric_embeddings under hp, the
//                   numeric linear weights under the wide rule, as the wide bias)
//     sweep   each workgroup owns a slice of the R rows, builds the batch's touched set itself (a bitmap of R bits in
//             LDS, from ids) and gives every row of its slice that is NOT touched one step of TF Adam's whole-table
//             sweep (replay_step of optim_rules.h), table record and wide record, stamp = step.  Only records under
//             Adam are swept, each with its own rule's lr_t; with no part under Adam there is no sweep workgroup (in a
//             group: such a member's return at once) and untouched rows are neither read nor written.
//   Touched and untouched rows are disjoint and the dense variables belong to block 0: no workgroup reads what another
//   writes in this launch and none waits for another — no flags, no grid barrier, no float atomics to global memory.
//   Results do not depend on G.
//
//   train_fused_group_k   M independent models, one step each, in ONE launch (mi_train_group_step): grid (1 + G, M),
//     blockIdx.y = the member, blockIdx.x == 0 its batch workgroup, the others its sweep workgroups.  A workgroup copies
//     its member's Args from the device table mi_train_group_plan wrote, fills in what changes per step (ids, labels,
//     outputs, step, lr_t = lr_table[step], seed = seed_base + step 1000003) and runs batch_block / sweep_block below:
//     the arithmetic has this one definition, so a member's bits are those of train_fused_k on it alone.  A member's
//     workgroups touch only that member's buffers.
//
//   eval_fused_group_k    the same M models over a whole evaluation set in ONE launch (mi_eval_group): grid (X, M), a workgroup
//     runs forward_block — phases 0-2 of batch_block, the forward's one definition — without dropout over its member's tiles
//     and keeps mi_eval_accumulate's counters (eval_rules.h) in LDS; nothing of any model is written (see the kernel).
//
// Arithmetic: fp32 throughout; compiled with -ffp-contract=off (the update rules and the FM term are written one
// rounding per operation); the MLP's dot products use explicit fmaf.
#include <memory>
#include <new>

#include "common.h"
#include "eval_rules.h"
#include "optim_rules.h"

namespace {

constexpr int kThreads = 512;
constexpr int kMaxBatch = 128;
constexpr int kMaxFields = 32;
constexpr int kMaxNumeric = 16;
constexpr int kMaxEmb = 16;
constexpr int kMaxHidden = 3;
constexpr int kMaxWidth = 64;
constexpr int kMaxLayers = kMaxHidden + 1;          // + the logits layer
constexpr int64_t kMaxConcat = 16384;               // B (F + nd) E
constexpr int64_t kMaxRows = int64_t(1) << 18;      // a 32 KB bitmap
constexpr int kMaxSweepBlocks = 1024;
constexpr size_t kMaxLds = 160 * 1024 - 1024;       // (the static arrays below take the rest)
constexpr int kRowsInFlight = 4;

struct Layer {
  int64_t w_off, b_off;                 // offsets into the flat dense buffer: kernel [fan_in, fan_out], bias [fan_out]
  int32_t fan_in, fan_out;
  int32_t out_off, pad;                 // the layer's output [B][fan_out] in LDS (float offset)
};

// Two rules: hp is the rule of the table records and the MLP's variables (slots tm / tv, dm / dv), hpw the rule of the WIDE
// part — the lin_w records (lm / lv) and the wide bias at lin_bias_off (dwm / dwv, indexed like dense).  With one optimizer
// the plan sets hpw = hp and dwm / dwv = dm / dv.  A slot pointer is NULL where the rule keeps no such slot (Adagrad: slot 1;
// SGD: both): that slot is neither loaded nor stored.  last_step is NULL when neither rule is Adam (no stamps, no sweep).
struct Args {
  float* table; float* tm; float* tv;   // or NULL (no FM term and no DNN)
  float* lin_w; float* lm; float* lv;   // or NULL (no wide part)
  int32_t* last_step;
  const int64_t* field_off;
  const int32_t* ids;
  const uint8_t* labels;
  float* dense; float* dm; float* dv;
  float* dwm; float* dwv;
  uint64_t wide_mask;                   // bit f set: field f has a wide weight (mi_predict_fused's wide_fields)
  float* gdense;                        // workspace: the dense gradient, indexed like dense
  float* dcat_ws;                       // workspace: d_concat [B][(F + nd) E] when LDS has no room for it, else NULL
  float* logits; float* loss;
  const float* x_num;                   // [B][nd], or NULL (nd = 0)
  int64_t ts, R, lin_bias_off;
  int64_t num_emb_off, lin_num_off;     // in dense: numeric_embeddings [nd][E], the numeric linear weights [nd]
  uint64_t seed;
  int32_t B, F, E, ls, act, n_layers, use_linear, use_fm, step, nd;
  int32_t o_sumv, o_tq, o_lin, o_dl, o_dcat;   // float offsets in LDS (the rows [B F] int32 lead)
  float keep, scale;
  Hp hp, hpw;
  Layer l[kMaxLayers];
};

// a slot that may be absent: 0 stands in for the value no rule reads, and nothing is stored
__device__ __forceinline__ float ld_slot(const float* s, int64_t o) { return s ? s[o] : 0.f; }
__device__ __forceinline__ void st_slot(float* s, int64_t o, float v) { if (s) s[o] = v; }
__device__ __forceinline__ float4 ld4_slot(const float* s, int64_t o) { return s ? ld4(s + o) : make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void st4_slot(float* s, int64_t o, float4 v) { if (s) st4(s + o, v); }

__device__ __forceinline__ int32_t row_of(const Args& p, int i) {
  const int f = i % p.F;
  int64_t r = p.field_off[f] + p.ids[i];
  r = r < 0 ? 0 : (r >= p.R ? p.R - 1 : r);             // (ids are trusted to lie inside their field; a bad one stays inside the arrays)
  return static_cast<int32_t>(r);
}

// ---- sweep workgroups ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void sweep_block(const Args& p, uint32_t* __restrict__ bm) {
  // the records under Adam: TF Adam's sparse apply walks the whole variable; the other four rules touch the batch's rows only
  const bool t_adam = p.table && p.hp.kind == MI_OPT_ADAM, l_adam = p.lin_w && p.hpw.kind == MI_OPT_ADAM;
  if (!t_adam && !l_adam) return;                       // (a member of a group without an Adam part: its rows stay as they are)
  const int tid = threadIdx.x;
  const int words = static_cast<int>((p.R + 31) >> 5);
  for (int i = tid; i < words; i += kThreads) bm[i] = 0u;
  __syncthreads();
  const int n = p.B * p.F;
  for (int i = tid; i < n; i += kThreads) {
    const int32_t r = row_of(p, i);
    atomicOr(&bm[r >> 5], 1u << (r & 31));
  }
  __syncthreads();
  const int cpf = t_adam ? p.E / 4 : 1;
  const int64_t G = static_cast<int64_t>(gridDim.x) - 1;
  const int64_t per = (p.R + G - 1) / G;
  const int64_t lo = (static_cast<int64_t>(blockIdx.x) - 1) * per;
  const int64_t hi = lo + per < p.R ? lo + per : p.R;
  const int64_t items = hi > lo ? (hi - lo) * cpf : 0;
  const float b1 = p.hp.beta1, b2 = p.hp.beta2, eps = p.hp.eps, lr_t = p.hp.lr_t;
  const float wb1 = p.hpw.beta1, wb2 = p.hpw.beta2, weps = p.hpw.eps, wlr_t = p.hpw.lr_t;      // (each part its own schedule)
  for (int64_t i0 = tid; i0 < items; i0 += static_cast<int64_t>(kThreads) * kRowsInFlight) {
    float4 w[kRowsInFlight], m[kRowsInFlight], v[kRowsInFlight];
    float lw[kRowsInFlight], lm[kRowsInFlight], lv[kRowsInFlight];
    int64_t r[kRowsInFlight];
    int c[kRowsInFlight];
    bool on[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const int64_t i = i0 + static_cast<int64_t>(u) * kThreads;
      on[u] = i < items;
      r[u] = lo + (on[u] ? i / cpf : 0);
      c[u] = on[u] ? static_cast<int>(i % cpf) : 0;
      on[u] = on[u] && !((bm[r[u] >> 5] >> (r[u] & 31)) & 1u);
      w[u] = m[u] = v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      lw[u] = lm[u] = lv[u] = 0.f;
      if (on[u] && t_adam) {
        const int64_t o = r[u] * p.ts + 4 * c[u];
        w[u] = ld4(p.table + o); m[u] = ld4(p.tm + o); v[u] = ld4(p.tv + o);
      }
      if (on[u] && c[u] == 0 && l_adam) {
        const int64_t o = r[u] * p.ls;
        lw[u] = p.lin_w[o]; lm[u] = p.lm[o]; lv[u] = p.lv[o];
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      if (!on[u]) continue;
      if (t_adam) {
        const int64_t o = r[u] * p.ts + 4 * c[u];
        replay_step(w[u].x, m[u].x, v[u].x, lr_t, b1, b2, eps);
        replay_step(w[u].y, m[u].y, v[u].y, lr_t, b1, b2, eps);
        replay_step(w[u].z, m[u].z, v[u].z, lr_t, b1, b2, eps);
        replay_step(w[u].w, m[u].w, v[u].w, lr_t, b1, b2, eps);
        st4(p.table + o, w[u]); st4(p.tm + o, m[u]); st4(p.tv + o, v[u]);
      }
      if (c[u] == 0) {
        const int64_t o = r[u] * p.ls;
        if (l_adam) {
          replay_step(lw[u], lm[u], lv[u], wlr_t, wb1, wb2, weps);
          p.lin_w[o] = lw[u]; p.lm[o] = lm[u]; p.lv[o] = lv[u];
        }
        p.last_step[o] = p.step;
      }
    }
  }
}

// ---- the batch workgroup --------------------------------------------------------------------------------------------
// output (b, n) of a layer from its pre-activation sum: bias, activation, dropout (hidden layers only)
__device__ __forceinline__ float finish(const Args& p, float acc, float bias, bool last, int li, int b, int n, uint32_t thresh) {
  float v = acc + bias;
  if (last) return v;
  v = mi_act(p.act, v);
  if (p.keep < 1.f)                                              // layer i's mask: seed + 7919 i (engine._layer_seed)
    v = mi_drop_keep_at(p.seed + 7919ull * static_cast<uint64_t>(li), static_cast<uint32_t>(b), static_cast<uint32_t>(n), thresh)
            ? v / p.keep : 0.f;
  return v;
}

// Phases 0-2 of a batch: rows, forward, head.  The one definition of the model's forward in this file: the training step
// (kTrain: also dlogit, into dl and over the logits layer's output, and its sum into red[1]) and the evaluation kernel
// (no gradient, keep = 1) run it.  Returns the thread's logit (thread b < B holds example b; 0 elsewhere); p.logits may be
// NULL; p.loss[0] = the batch loss, reduced in the head's order, is written before the return (after a barrier).
template <bool kTrain>
__device__ __forceinline__ float forward_block(const Args& p, char* lds, const Layer* layers, float (*red)[kThreads / 64]) {
  const int tid = threadIdx.x;
  const int B = p.B, F = p.F, E = p.E, L = p.n_layers, nd = p.nd;
  const int64_t ts = p.ts;
  const float* __restrict__ xn = p.x_num;                           // (read only when nd > 0)
  const float* __restrict__ Vn = p.dense + p.num_emb_off;
  int32_t* rows = reinterpret_cast<int32_t*>(lds);
  float* fl = reinterpret_cast<float*>(lds);
  float* sumv = fl + p.o_sumv;
  float* tq = fl + p.o_tq;
  float* zlin = fl + p.o_lin;
  float* dl = fl + p.o_dl;
  const uint32_t thresh = mi_drop_thresh16(p.keep);

  // 0. the batch's rows
  for (int i = tid; i < B * F; i += kThreads) rows[i] = row_of(p, i);
  __syncthreads();

  // 1. forward: FM sums, the wide sum, layer 1
  {
    const int nE = (p.table && p.use_fm) ? B * E : 0, nL = p.use_linear ? B : 0;
    const int w1 = L ? layers[0].fan_out : 0, n1 = B * w1;
    for (int i = tid; i < nE + nL + n1; i += kThreads) {
      if (i < nE) {
        const int b = i / E, c = i - b * E;
        float s = 0.f, q = 0.f;
        for (int f = 0; f < F; ++f) {
          const float v = p.table[static_cast<int64_t>(rows[b * F + f]) * ts + c];
          s = s + v;
          q = q + v * v;
        }
        for (int j = 0; j < nd; ++j) {                            // the numeric rows, behind the categorical ones
          const float v = xn[b * nd + j] * Vn[j * E + c];
          s = s + v;
          q = q + v * v;
        }
        sumv[i] = s;
        tq[i] = s * s - q;                                        // deep_fm.py:81-87 (one field: exactly 0)
      } else if (i < nE + nL) {
        const int b = i - nE;
        float acc = 0.f;
        for (int f = 0; f < F; ++f)
          if ((p.wide_mask >> f) & 1u) acc = acc + p.lin_w[static_cast<int64_t>(rows[b * F + f]) * p.ls];
        for (int j = 0; j < nd; ++j) acc = acc + xn[b * nd + j] * p.dense[p.lin_num_off + j];
        zlin[b] = acc;
      } else {
        const int j = i - nE - nL, b = j / w1, n = j - b * w1;
        const float* __restrict__ W = p.dense + layers[0].w_off;
        float acc = 0.f;
        for (int f = 0; f < F; ++f) {
          const float* __restrict__ row = p.table + static_cast<int64_t>(rows[b * F + f]) * ts;
          for (int c = 0; c < E; c += 4) {
            const float4 x = ld4(row + c);
            const float* __restrict__ wk = W + static_cast<int64_t>(f * E + c) * w1 + n;
            acc = fmaf(x.x, wk[0], acc);
            acc = fmaf(x.y, wk[w1], acc);
            acc = fmaf(x.z, wk[2 * w1], acc);
            acc = fmaf(x.w, wk[3 * w1], acc);
          }
        }
        for (int jn = 0; jn < nd; ++jn) {                          // rows F E .. of kernel_0: the numeric rows x V[jn, :]
          const float x = xn[b * nd + jn];
          const float* __restrict__ wk = W + static_cast<int64_t>((F + jn) * E) * w1 + n;
          for (int c = 0; c < E; ++c) acc = fmaf(x * Vn[jn * E + c], wk[c * w1], acc);
        }
        fl[layers[0].out_off + j] = finish(p, acc, p.dense[layers[0].b_off + n], L == 1, 0, b, n, thresh);
      }
    }
  }
  __syncthreads();
  for (int li = 1; li < L; ++li) {
    const Layer ly = layers[li];
    const float* __restrict__ in = fl + layers[li - 1].out_off;
    const float* __restrict__ W = p.dense + ly.w_off;
    const int K = ly.fan_in, N = ly.fan_out;
    for (int j = tid; j < B * N; j += kThreads) {
      const int b = j / N, n = j - b * N;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(in[b * K + k], W[k * N + n], acc);
      fl[ly.out_off + j] = finish(p, acc, p.dense[ly.b_off + n], li + 1 == L, li, b, n, thresh);
    }
    __syncthreads();
  }

  // 2. head (the order of mi_sigmoid_ce_head); the logits layer's output becomes its gradient
  float z = 0.f;
  {
    float per = 0.f, d = 0.f;
    if (tid < B) {
      if (p.use_linear) z = zlin[tid] + p.dense[p.lin_bias_off];
      if (p.table && p.use_fm) {
        float t = 0.f;
        for (int c = 0; c < E; ++c) t = t + tq[tid * E + c];
        z = z + 0.5f * t;
      }
      if (L) z = z + fl[layers[L - 1].out_off + tid];
      const float y = static_cast<float>(p.labels[tid]);
      per = mi_sigmoid_ce_loss(z, y) * p.scale;
      if (p.logits) p.logits[tid] = z;
      if (kTrain) {
        d = mi_sigmoid_ce_grad(z, y, p.scale);
        dl[tid] = d;
        if (L) fl[layers[L - 1].out_off + tid] = d;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      per += __shfl_xor(per, o);
      if (kTrain) d += __shfl_xor(d, o);
    }
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = per;
      if (kTrain) red[1][tid >> 6] = d;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int nw = (B + 63) >> 6;                                 // waves that hold examples (at most 2)
    float s = red[0][0];
    for (int w = 1; w < nw; ++w) s = s + red[0][w];
    p.loss[0] = s;
  }
  return z;
}

__device__ __forceinline__ void batch_block(const Args& p, char* lds, const Layer* layers, float (*red)[kThreads / 64]) {
  forward_block<true>(p, lds, layers, red);
  const int tid = threadIdx.x;
  const int B = p.B, F = p.F, E = p.E, L = p.n_layers, nd = p.nd, D = (F + nd) * E;
  const int64_t ts = p.ts;
  const float* __restrict__ xn = p.x_num;
  const float* Vn = p.dense + p.num_emb_off;                        // (phase 4 writes these: no __restrict__)
  const int32_t* rows = reinterpret_cast<const int32_t*>(lds);
  float* fl = reinterpret_cast<float*>(lds);
  const float* sumv = fl + p.o_sumv;
  const float* dl = fl + p.o_dl;
  float* dcat = p.dcat_ws ? p.dcat_ws : fl + p.o_dcat;
  const int nw = (B + 63) >> 6;

  // 3. backward through the MLP, top down
  for (int li = L - 1; li >= 0; --li) {
    const Layer ly = layers[li];
    const float* __restrict__ dy = fl + ly.out_off;
    const float* __restrict__ W = p.dense + ly.w_off;
    const int K = ly.fan_in, N = ly.fan_out;
    float* prev = li ? fl + layers[li - 1].out_off : nullptr;
    // weight and bias gradient
    for (int i = tid; i < K * N + N; i += kThreads) {
      float acc = 0.f;
      if (i < K * N) {
        const int k = i / N, n = i - k * N;
        if (li) {
          for (int b = 0; b < B; ++b) acc = fmaf(prev[b * K + k], dy[b * N + n], acc);
        } else {
          const int f = k / E, c = k - f * E;
          if (f < F) {
            for (int b = 0; b < B; ++b)
              acc = fmaf(p.table[static_cast<int64_t>(rows[b * F + f]) * ts + c], dy[b * N + n], acc);
          } else {                                                  // a numeric row of the concat, as the forward formed it
            const float v = Vn[(f - F) * E + c];
            for (int b = 0; b < B; ++b) acc = fmaf(xn[b * nd + (f - F)] * v, dy[b * N + n], acc);
          }
        }
        p.gdense[ly.w_off + i] = acc;
      } else {
        const int n = i - K * N;
        for (int b = 0; b < B; ++b) acc = acc + dy[b * N + n];
        p.gdense[ly.b_off + n] = acc;
      }
    }
    if (li) {
      __syncthreads();                                            // (the loop above read what the loop below overwrites)
      for (int i = tid; i < B * K; i += kThreads) {
        const int b = i / K, k = i - b * K;
        float g = 0.f;
        for (int n = 0; n < N; ++n) g = fmaf(dy[b * N + n], W[k * N + n], g);
        const float x = prev[i];                                  // the stored output: act(pre) / keep, or 0 (dropped)
        if (p.act == 1) {
          g = x > 0.f ? g / p.keep : 0.f;
        } else {
          const bool dropped = p.keep < 1.f && x == 0.f;
          g = dropped ? 0.f : (g / p.keep) * mi_act_deriv_from_output(p.act, x * p.keep);
        }
        prev[i] = g;
      }
    } else {
      for (int i = tid; i < B * K; i += kThreads) {               // d_concat [B][(F + nd) E] (K >= that; rows past it belong to no column)
        const int b = i / K, k = i - b * K;
        if (k >= D) continue;
        float g = 0.f;
        for (int n = 0; n < N; ++n) g = fmaf(dy[b * N + n], W[k * N + n], g);
        dcat[b * D + k] = g;
      }
    }
    __syncthreads();
  }
  // the numeric columns: dV[j, c] = sum_b x[b, j] g[b, j, c] with the entry gradient of the categorical rows,
  // g = d_concat[b, F + j, c] + dlogit[b] (sumv[b, c] - x[b, j] V[j, c]), and dw_num[j] = sum_b dlogit[b] x[b, j]; one thread
  // per element, b ascending.  The same thread applies its element in phase 4: nothing else reads V or w_num from here on.
  for (int i = tid; i < nd * E + (p.use_linear ? nd : 0); i += kThreads) {
    float acc = 0.f;
    if (i < nd * E) {
      const int j = i / E, c = i - j * E;
      const float w = Vn[i];
      for (int b = 0; b < B; ++b) {
        const float x = xn[b * nd + j];
        float g = L ? dcat[b * D + (F + j) * E + c] : 0.f;
        if (p.use_fm) g = g + dl[b] * (sumv[b * E + c] - x * w);
        acc = acc + x * g;
      }
      p.gdense[p.num_emb_off + i] = acc;
    } else {
      const int j = i - nd * E;
      for (int b = 0; b < B; ++b) acc = acc + dl[b] * xn[b * nd + j];
      p.gdense[p.lin_num_off + j] = acc;
    }
  }

  // 4. apply.  Sparse: item (entry e, float4 chunk c) — the first entry of a row leads it
  {
    const int cpf = p.table ? E / 4 : 1;
    for (int i = tid; i < B * F * cpf; i += kThreads) {
      const int e = i / cpf, c = i - e * cpf, b = e / F, f = e - b * F;
      const int32_t r = rows[e];
      float4 w = make_float4(0.f, 0.f, 0.f, 0.f), g = w;
      const int64_t o = static_cast<int64_t>(r) * ts + 4 * c;
      if (p.table) w = ld4(p.table + o);
      float gl = 0.f;
      bool leader = true;
      for (int b2 = 0; b2 < B; ++b2) {
        if (rows[b2 * F + f] != r) continue;
        if (b2 < b) { leader = false; break; }
        const float d = dl[b2];
        if (p.table) {
          // d_concat[b, f, :] + dlogit[b] (sumv[b, :] - row): the entry gradient of mi_sparse_apply_fused
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (L) {
            const float* q = dcat + b2 * D + f * E + 4 * c;
            v = make_float4(q[0], q[1], q[2], q[3]);
          }
          if (p.use_fm) {
            const float* s = sumv + b2 * E + 4 * c;
            v.x = v.x + d * (s[0] - w.x); v.y = v.y + d * (s[1] - w.y);
            v.z = v.z + d * (s[2] - w.z); v.w = v.w + d * (s[3] - w.w);
          }
          g.x = g.x + v.x; g.y = g.y + v.y; g.z = g.z + v.z; g.w = g.w + v.w;
        }
        gl = gl + d;
      }
      if (!leader) continue;
      if (p.table) {
        float4 m = ld4_slot(p.tm, o), v = ld4_slot(p.tv, o);
        sparse_rule(p.hp, w.x, m.x, v.x, g.x);
        sparse_rule(p.hp, w.y, m.y, v.y, g.y);
        sparse_rule(p.hp, w.z, m.z, v.z, g.z);
        sparse_rule(p.hp, w.w, m.w, v.w, g.w);
        st4(p.table + o, w); st4_slot(p.tm, o, m); st4_slot(p.tv, o, v);
      }
      if (c == 0) {
        const int64_t ol = static_cast<int64_t>(r) * p.ls;
        if (p.lin_w && ((p.wide_mask >> f) & 1u)) {               // (a field without a wide weight: its record stays as it is)
          float lw = p.lin_w[ol], m = ld_slot(p.lm, ol), v = ld_slot(p.lv, ol);
          sparse_rule(p.hpw, lw, m, v, gl);
          p.lin_w[ol] = lw; st_slot(p.lm, ol, m); st_slot(p.lv, ol, v);
        }
        if (p.last_step) p.last_step[ol] = p.step;
      }
    }
  }
  // dense: every variable of the MLP, and the wide part's bias (its gradient is the sum of dlogit)
  for (int li = 0; li < L; ++li) {
    const Layer ly = layers[li];
    const int kn = ly.fan_in * ly.fan_out;
    for (int i = tid; i < kn + ly.fan_out; i += kThreads) {
      const int64_t o = i < kn ? ly.w_off + i : ly.b_off + (i - kn);
      float w = p.dense[o], m = ld_slot(p.dm, o), v = ld_slot(p.dv, o);
      dense_rule(p.hp, w, m, v, p.gdense[o]);
      p.dense[o] = w; st_slot(p.dm, o, m); st_slot(p.dv, o, v);
    }
  }
  // numeric_embeddings follow hp like the MLP; the numeric linear weights belong to the wide part (hpw, dwm / dwv).  Element i
  // is applied by the thread that wrote its gradient.
  for (int i = tid; i < nd * E + (p.use_linear ? nd : 0); i += kThreads) {
    const bool wide = i >= nd * E;
    const int64_t o = wide ? p.lin_num_off + (i - nd * E) : p.num_emb_off + i;
    float* const sm = wide ? p.dwm : p.dm;
    float* const sv = wide ? p.dwv : p.dv;
    float w = p.dense[o], m = ld_slot(sm, o), v = ld_slot(sv, o);
    dense_rule(wide ? p.hpw : p.hp, w, m, v, p.gdense[o]);
    p.dense[o] = w; st_slot(sm, o, m); st_slot(sv, o, v);
  }
  if (p.use_linear && tid == 0) {
    float g = red[1][0];
    for (int w = 1; w < nw; ++w) g = g + red[1][w];
    const int64_t o = p.lin_bias_off;
    float w = p.dense[o], m = ld_slot(p.dwm, o), v = ld_slot(p.dwv, o);
    dense_rule(p.hpw, w, m, v, g);                                 // (the wide part's rule and its own dense slots)
    p.dense[o] = w; st_slot(p.dwm, o, m); st_slot(p.dwv, o, v);
  }
}

__global__ __launch_bounds__(kThreads) void train_fused_k(const Args p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ Layer layers[kMaxLayers];
  __shared__ float red[2][kThreads / 64];
  if (blockIdx.x) {
    sweep_block(p, reinterpret_cast<uint32_t*>(lds));
    return;
  }
  // (the layer table: compile-time indices into the kernel arguments, runtime indices into LDS afterwards)
#pragma unroll
  for (int i = 0; i < kMaxLayers; ++i)
    if (threadIdx.x == i) layers[i] = p.l[i];
  __syncthreads();
  batch_block(p, lds, layers, red);
}

// one member of a population: its Args as mi_train_group_plan validated them (ids / labels / logits / loss / step / seed /
// hp.lr_t / hpw.lr_t are filled in by the kernel), the Adam schedule table of each rule (NULL: the rule is not Adam; with
// one rule both name the same table) and the step-free part of its dropout seed
struct Member {
  Args a;
  const float* lr_table;                // lr_t of step s at [s], lr_len entries
  const float* lr_table_w;              // the wide part's, lr_len_w entries
  uint64_t seed_base;
  int64_t lr_len, lr_len_w;
};

__global__ __launch_bounds__(kThreads) void train_fused_group_k(const Member* __restrict__ members, const int32_t* __restrict__ ids,
                                                                int64_t ids_stride, const float* __restrict__ x_num,
                                                                int64_t x_stride, const uint8_t* __restrict__ labels,
                                                                int64_t labels_stride, float* __restrict__ logits,
                                                                float* __restrict__ loss, int32_t step) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ Args sp;
  __shared__ Layer layers[kMaxLayers];
  __shared__ float red[2][kThreads / 64];
  const int y = blockIdx.y;
  const Member* me = members + y;
  mi_copy_words<kThreads>(&sp, &me->a);
  __syncthreads();
  if (threadIdx.x == 0) {
    // (mi_train_group_step checked the step against every table: stay inside)
    if (me->lr_table) sp.hp.lr_t = me->lr_table[step < me->lr_len ? step : me->lr_len - 1];
    if (me->lr_table_w) sp.hpw.lr_t = me->lr_table_w[step < me->lr_len_w ? step : me->lr_len_w - 1];
    sp.ids = ids + y * ids_stride;
    sp.x_num = x_num ? x_num + y * x_stride : nullptr;
    sp.labels = labels + y * labels_stride;
    sp.logits = logits + static_cast<int64_t>(y) * sp.B;
    sp.loss = loss + y;
    sp.step = step;
    sp.seed = me->seed_base + static_cast<uint64_t>(step) * 1000003ull;    // engine._layer_seed(0) of this step
  }
  if (threadIdx.x < kMaxLayers) layers[threadIdx.x] = sp.l[threadIdx.x];
  __syncthreads();
  if (blockIdx.x) {
    sweep_block(sp, reinterpret_cast<uint32_t*>(lds));
    return;
  }
  batch_block(sp, lds, layers, red);
}

// ---- evaluation of a population -----------------------------------------------------------------------------------------
// eval_fused_group_k   grid (X, M), blockIdx.y = the member.  A workgroup runs forward_block — keep = 1 whatever the member's
//   dropout, no gradient — over the tiles t = blockIdx.x, blockIdx.x + X, ... of its member (tile t = examples
//   [t B, min(N, (t + 1) B)) of the evaluation set) and counts every example with eval_rules.h into LDS.  Per tile it writes
//   batch_loss[i, t] (the head's order; the member's scale, tail_scale[i] on a short last tile), the three fp64 sums
//   partials[i, t, :] (wave shuffle, then the waves in ascending order: one writer, a plain vector store) and, if asked, the
//   logits.  At its end it adds its hist / counts to the member's own arrays with integer atomics.  Nothing of the model and no
//   training workspace is written; no workgroup reads what another writes and none waits for another; no result depends on X.
struct EvalShared {
  Args sp;
  Layer layers[kMaxLayers];
  float red[2][kThreads / 64];
  float th[kAucThresholds];
  unsigned int lh[kEvalHist];
  unsigned int lc[kEvalCounts];
  double ls[kThreads / 64][4];
};
// what a forward needs of the dynamic LDS ends where d_concat would begin: at most this, whatever the plan asked for
constexpr size_t kMaxForwardLds = sizeof(float) * static_cast<size_t>(kMaxConcat / 4 + 2 * (kMaxConcat / 8) + 2 * kMaxBatch +
                                                                       kMaxHidden * kMaxBatch * kMaxWidth + kMaxBatch);
static_assert(kMaxForwardLds + sizeof(EvalShared) + 256 <= 160 * 1024, "the evaluation kernel's LDS");

__global__ __launch_bounds__(kThreads) void eval_fused_group_k(const Member* __restrict__ members, const int32_t* __restrict__ ids,
                                                               const float* __restrict__ x_num, int64_t x_stride,
                                                               const uint8_t* __restrict__ labels, int64_t N, int64_t T,
                                                               const float* __restrict__ tail_scale, float* __restrict__ logits,
                                                               float* __restrict__ batch_loss, unsigned long long* __restrict__ hist,
                                                               unsigned long long* __restrict__ counts, double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ EvalShared es;
  const int tid = threadIdx.x;
  const int y = blockIdx.y;
  mi_copy_words<kThreads>(&es.sp, &members[y].a);
  mi_eval_init(es.th, es.lh, es.lc, tid, kThreads);
  __syncthreads();
  if (tid < kMaxLayers) es.layers[tid] = es.sp.l[tid];
  const int B = es.sp.B, F = es.sp.F;
  const float scale = es.sp.scale;
  __syncthreads();
  for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
    const int64_t b0 = t * B;
    const int n = static_cast<int>(N - b0 < B ? N - b0 : B);
    if (tid == 0) {
      es.sp.ids = ids + b0 * F;
      es.sp.x_num = x_num ? x_num + y * x_stride + b0 * es.sp.nd : nullptr;
      es.sp.labels = labels + b0;
      es.sp.logits = logits ? logits + y * N + b0 : nullptr;
      es.sp.loss = batch_loss + y * T + t;
      es.sp.B = n;
      es.sp.scale = n < B ? tail_scale[y] : scale;
      es.sp.keep = 1.f;
    }
    __syncthreads();
    const float z = forward_block<false>(es.sp, lds, es.layers, es.red);
    double sl = 0, sp = 0, sy = 0;
    if (tid < n) mi_eval_count(z, labels[b0 + tid] ? 1 : 0, es.th, es.lh, es.lc, sl, sp, sy);
    if (tid < ((n + 63) & ~63)) {                                   // (wave-uniform: the waves that hold examples)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { sl += __shfl_xor(sl, o); sp += __shfl_xor(sp, o); sy += __shfl_xor(sy, o); }
      if ((tid & 63) == 0) { es.ls[tid >> 6][0] = sl; es.ls[tid >> 6][1] = sp; es.ls[tid >> 6][2] = sy; }
    }
    __syncthreads();
    if (tid < 3) {
      const int nw = (n + 63) >> 6;
      double v = es.ls[0][tid];
      for (int w = 1; w < nw; ++w) v = v + es.ls[w][tid];
      partials[(y * T + t) * 3 + tid] = v;
    }
    __syncthreads();                                                // (the next tile rewrites sp, red and ls)
  }
  mi_eval_flush(es.lh, es.lc, hist + static_cast<int64_t>(y) * kEvalHist, counts + static_cast<int64_t>(y) * kEvalCounts, tid, kThreads);
}

using mi::unsupported;

int64_t align4(int64_t n) { return (n + 3) & ~int64_t(3); }

// LDS of the batch workgroup without d_concat (floats)
int64_t batch_lds_floats(int64_t B, int32_t F, int32_t E, const int32_t* widths, int32_t n_layers) {
  int64_t n = align4(B * F) + 2 * align4(B * E) + 2 * align4(B);
  for (int i = 0; i < n_layers; ++i) n += align4(B * widths[i + 1]);
  return n;
}

// the dense gradient, then d_concat [B][(F + nd) E]
size_t workspace_bytes_of(int64_t B, int32_t F, int32_t nd, int32_t E, int64_t n_dense) {
  if (B < 0 || F < 0 || nd < 0 || E < 0 || n_dense < 0) return 0;
  return sizeof(float) * static_cast<size_t>(align4(n_dense) + align4(B * (F + nd) * E));
}

// slots a rule keeps: Adam, Ftrl and RMSProp two, Adagrad slot 0 only, SGD none
int slots_of(int kind) { return kind == MI_OPT_SGD ? 0 : (kind == MI_OPT_ADAGRAD ? 1 : 2); }

// what the Adam-only entries (mi_train_step_fused, mi_train_group_plan) describe, as the general description: one rule,
// every field in the wide part
mi_fused_model_t model_of(const mi_fused_member_t& m, int32_t F) {
  mi_fused_model_t g{};
  g.table = m.table; g.t_m = m.t_m; g.t_v = m.t_v; g.table_stride = m.table_stride;
  g.lin_w = m.lin_w; g.l_m = m.l_m; g.l_v = m.l_v; g.last_step = m.last_step; g.R = m.R;
  g.dense = m.dense; g.d_m = m.d_m; g.d_v = m.d_v; g.n_dense = m.n_dense;
  g.layer_off = m.layer_off; g.widths = m.widths; g.lin_bias_off = m.lin_bias_off;
  g.lr_table = m.lr_table; g.lr_table_len = m.lr_table_len; g.seed_base = m.seed_base;
  g.workspace = m.workspace; g.workspace_bytes = m.workspace_bytes;
  g.lin_stride = m.lin_stride; g.E = m.E; g.n_layers = m.n_layers; g.activation = m.activation;
  g.use_linear = m.use_linear; g.use_fm = m.use_fm; g.use_dnn = m.use_dnn;
  g.keep_prob = m.keep_prob; g.scale = m.scale; g.hp = m.hp;
  g.wide_fields = (F >= 1 && F < 64) ? (uint64_t(1) << F) - 1 : ~uint64_t(0);
  return g;
}

// The checks of one model, in mi_train_step_fused's order, and its Args (everything but ids / labels / logits / loss / step /
// seed / lr_t, which the caller fills in; have_batch / have_outputs: the caller holds those pointers — a plan has none yet),
// the dynamic LDS of its workgroups and the built-in number of sweep workgroups (0: no part is under Adam, nothing to
// sweep).  Writes nothing but `a`.  (m's lr_table*, lr_table*_len and seed_base belong to the group plan.)  num: the model's
// numeric columns, or NULL (none); a.x_num is the caller's to fill in, like ids.
int32_t plan_model(const mi_fused_model_t& m, const mi_fused_numeric_t* num, const int64_t* field_off, int64_t B, int32_t F,
                   int32_t step, bool have_batch, bool have_outputs, int32_t sweep_blocks, Args& a, size_t& lds_out,
                   int& blocks_out) {
  const int64_t R = m.R, n_dense = m.n_dense;
  const int32_t nd = num ? num->n_numeric : 0;
  const int32_t n_layers = m.n_layers;
  const int32_t* widths = m.widths;
  const bool two = m.two_rules != 0;
  const mi_opt_hparams& hw = two ? m.hp_wide : m.hp;
  for (const mi_opt_hparams* h : {&m.hp, &hw}) {
    MI_REQUIRE(h->kind >= MI_OPT_ADAM && h->kind <= MI_OPT_SGD, "train_step_fused: optimizer kind %d (0 to 4)", h->kind);
    MI_REQUIRE(h->kind != MI_OPT_FTRL || h->lr_power == -0.5f,
               "train_step_fused: Ftrl learning_rate_power %f unsupported (TF default -0.5 only)", h->lr_power);
  }
  MI_REQUIRE(!two || m.use_linear, "train_step_fused: two_rules without the wide part (use_linear = 0)");
  MI_REQUIRE(m.use_linear || m.use_fm || m.use_dnn, "train_step_fused: no part of the model is switched on");
  MI_REQUIRE(m.activation >= 0 && m.activation <= 3, "train_step_fused: activation %d", m.activation);
  MI_REQUIRE(step >= 1, "train_step_fused: step=%d (the global step after this call, 1-based)", step);
  MI_REQUIRE(m.keep_prob > 0.f && m.keep_prob <= 1.f, "train_step_fused: keep_prob=%g (in (0, 1])", m.keep_prob);
  if (B < 1 || B > kMaxBatch) return unsupported("train_step_fused: B=%lld (1 to %d examples)", (long long)B, kMaxBatch);
  if (F < 1 || F > kMaxFields) return unsupported("train_step_fused: F=%d categorical fields (1 to %d)", F, kMaxFields);
  const bool emb = m.use_fm || m.use_dnn;
  if (emb && (m.E < 4 || m.E > kMaxEmb || (m.E & 3)))
    return unsupported("train_step_fused: embedding size %d (a multiple of 4, at most %d)", m.E, kMaxEmb);
  const int32_t E = emb ? m.E : 4;
  if (nd < 0 || nd > kMaxNumeric) return unsupported("train_step_fused: %d numeric columns (0 to %d)", nd, kMaxNumeric);
  if (nd == 0 && B * F * E > kMaxConcat)
    return unsupported("train_step_fused: B F E = %lld (at most %lld)", (long long)(B * F * E), (long long)kMaxConcat);
  if (B * (F + nd) * E > kMaxConcat)
    return unsupported("train_step_fused: B (F + n_numeric) E = %lld (at most %lld)", (long long)(B * (F + nd) * E),
                       (long long)kMaxConcat);
  MI_REQUIRE(nd == 0 || emb, "train_step_fused: %d numeric columns without the FM term and the DNN (their embeddings enter nothing)", nd);
  if (R < 1 || R > kMaxRows) return unsupported("train_step_fused: R=%lld table rows (1 to %lld)", (long long)R, (long long)kMaxRows);
  if (sweep_blocks < 0 || sweep_blocks > kMaxSweepBlocks)
    return unsupported("train_step_fused: sweep_blocks=%d (0 = the built-in choice, at most %d)", sweep_blocks, kMaxSweepBlocks);
  const int nt = slots_of(m.hp.kind), nw = slots_of(hw.kind);      // slots of the table / MLP rule and of the wide rule
  const bool adam = (emb && m.hp.kind == MI_OPT_ADAM) || (m.use_linear && hw.kind == MI_OPT_ADAM);
  MI_REQUIRE(field_off && have_batch && (m.last_step || !adam), "train_step_fused: field_off / ids / labels / last_step");
  MI_REQUIRE(have_outputs, "train_step_fused: logits / loss");
  float* const t_m = nt >= 1 ? m.t_m : nullptr;
  float* const t_v = nt >= 2 ? m.t_v : nullptr;
  MI_REQUIRE(!emb || (m.table && (nt < 1 || t_m) && (nt < 2 || t_v) && mi::aligned16(m.table) && mi::aligned16(t_m) &&
                      mi::aligned16(t_v)),
             "train_step_fused: table / t_m / t_v (16-byte aligned)");
  MI_REQUIRE(!m.use_linear || F > 63 || (m.wide_fields >> F) == 0,
             "train_step_fused: wide_fields names a field at or above F=%d", F);
  MI_REQUIRE(m.table_stride == 0 || (m.table_stride >= E && (m.table_stride & 3) == 0),
             "train_step_fused: table_stride=%lld (0 = E, else >= E and a multiple of 4)", (long long)m.table_stride);
  MI_REQUIRE(m.lin_stride >= 1, "train_step_fused: lin_stride=%d", m.lin_stride);
  MI_REQUIRE(!m.use_linear || (m.lin_w && (nw < 1 || m.l_m) && (nw < 2 || m.l_v)), "train_step_fused: lin_w / l_m / l_v");
  MI_REQUIRE(m.dense && (nt < 1 || m.d_m) && (nt < 2 || m.d_v) && n_dense >= 1, "train_step_fused: dense / d_m / d_v / n_dense");
  MI_REQUIRE(!two || ((nw < 1 || m.dw_m) && (nw < 2 || m.dw_v)), "train_step_fused: dw_m / dw_v (the wide rule's dense slots)");
  MI_REQUIRE(!m.use_linear || (m.lin_bias_off >= 0 && m.lin_bias_off < n_dense), "train_step_fused: lin_bias_off");
  MI_REQUIRE(nd == 0 || (num->num_emb_off >= 0 && num->num_emb_off + static_cast<int64_t>(nd) * E <= n_dense),
             "train_step_fused: num_emb_off=%lld ([%d, %d] numeric_embeddings inside the %lld dense variables)",
             (long long)num->num_emb_off, nd, E, (long long)n_dense);
  MI_REQUIRE(nd == 0 || !m.use_linear || (num->lin_num_off >= 0 && num->lin_num_off + nd <= n_dense),
             "train_step_fused: lin_num_off=%lld (%d numeric linear weights inside the %lld dense variables)",
             (long long)num->lin_num_off, nd, (long long)n_dense);
  MI_REQUIRE(m.use_dnn ? n_layers >= 1 : n_layers == 0, "train_step_fused: %d layers (a DNN has at least its logits layer)", n_layers);
  if (n_layers > kMaxLayers)
    return unsupported("train_step_fused: %d hidden layers (at most %d)", n_layers - 1, kMaxHidden);
  MI_REQUIRE(n_layers == 0 || (m.layer_off && widths), "train_step_fused: layer_off / widths");
  a = Args{};
  for (int i = 0; i < n_layers; ++i) {
    const int fi = widths[i], fo = widths[i + 1];
    MI_REQUIRE(fi >= 1 && fo >= 1, "train_step_fused: width %d -> %d", fi, fo);
    MI_REQUIRE(i + 1 < n_layers || fo == 1, "train_step_fused: the last layer has %d outputs (1 expected)", fo);
    if (i + 1 < n_layers && fo > kMaxWidth) return unsupported("train_step_fused: hidden width %d (at most %d)", fo, kMaxWidth);
    const int64_t wo = m.layer_off[2 * i], bo = m.layer_off[2 * i + 1];
    MI_REQUIRE(wo >= 0 && bo >= 0 && wo + static_cast<int64_t>(fi) * fo <= n_dense && bo + fo <= n_dense,
               "train_step_fused: layer %d lies outside the %lld dense variables", i, (long long)n_dense);
    a.l[i].w_off = wo; a.l[i].b_off = bo; a.l[i].fan_in = fi; a.l[i].fan_out = fo;
  }
  MI_REQUIRE(n_layers == 0 || widths[0] == (F + nd) * E, "train_step_fused: widths[0]=%d, the %d input columns expected",
             n_layers ? widths[0] : 0, (F + nd) * E);
  const size_t need = workspace_bytes_of(B, F, nd, E, n_dense);
  if (m.workspace_bytes < need || !m.workspace) {
    mi::set_error("train_step_fused: workspace of %zu bytes, %zu needed", m.workspace_bytes, need);
    return MI_ERR_WORKSPACE;
  }
  MI_REQUIRE(mi::aligned16(m.workspace), "train_step_fused: workspace (16-byte aligned)");

  // LDS plan of the batch workgroup
  const int iB = static_cast<int>(B);
  int64_t o = align4(B * F);
  a.o_sumv = static_cast<int32_t>(o); o += align4(B * E);
  a.o_tq = static_cast<int32_t>(o); o += align4(B * E);
  a.o_lin = static_cast<int32_t>(o); o += align4(B);
  a.o_dl = static_cast<int32_t>(o); o += align4(B);
  for (int i = 0; i < n_layers; ++i) { a.l[i].out_off = static_cast<int32_t>(o); o += align4(B * widths[i + 1]); }
  const int64_t dcat = n_layers ? align4(B * (F + nd) * E) : 0;
  a.gdense = static_cast<float*>(m.workspace);
  a.dcat_ws = nullptr;
  a.o_dcat = static_cast<int32_t>(o);
  if (sizeof(float) * static_cast<size_t>(o + dcat) <= kMaxLds) o += dcat;
  else a.dcat_ws = a.gdense + align4(n_dense);
  size_t lds = sizeof(float) * static_cast<size_t>(o);
  if (lds > kMaxLds) return unsupported("train_step_fused: %zu bytes of LDS for B=%d F=%d E=%d and these widths", lds, iB, F, E);
  const size_t bitmap = sizeof(uint32_t) * static_cast<size_t>((R + 31) / 32);
  if (bitmap > lds) lds = bitmap;

  // (a slot the rule does not keep: NULL, whatever the caller passed)
  a.table = emb ? m.table : nullptr; a.tm = emb ? t_m : nullptr; a.tv = emb ? t_v : nullptr;
  a.lin_w = m.use_linear ? m.lin_w : nullptr;
  a.lm = (m.use_linear && nw >= 1) ? m.l_m : nullptr; a.lv = (m.use_linear && nw >= 2) ? m.l_v : nullptr;
  a.last_step = adam ? m.last_step : nullptr; a.field_off = field_off;
  a.dense = m.dense; a.dm = nt >= 1 ? m.d_m : nullptr; a.dv = nt >= 2 ? m.d_v : nullptr;
  a.dwm = nw >= 1 ? (two ? m.dw_m : m.d_m) : nullptr; a.dwv = nw >= 2 ? (two ? m.dw_v : m.d_v) : nullptr;
  a.wide_mask = m.use_linear ? m.wide_fields : 0;
  a.ts = m.table_stride ? m.table_stride : E; a.R = R; a.lin_bias_off = m.lin_bias_off;
  a.nd = nd; a.num_emb_off = nd ? num->num_emb_off : 0; a.lin_num_off = (nd && m.use_linear) ? num->lin_num_off : 0;
  a.B = iB; a.F = F; a.E = E; a.ls = m.lin_stride; a.act = m.activation; a.n_layers = n_layers;
  a.use_linear = m.use_linear != 0; a.use_fm = m.use_fm != 0;
  a.keep = m.keep_prob; a.scale = m.scale; a.hp = make_hp(&m.hp); a.hpw = make_hp(&hw);

  const int64_t items = R * ((emb && m.hp.kind == MI_OPT_ADAM) ? E / 4 : 1);
  const int64_t want = mi::ceil_div(items, static_cast<int64_t>(kThreads) * kRowsInFlight);
  blocks_out = !adam ? 0 : (sweep_blocks ? sweep_blocks : static_cast<int>(want < 1 ? 1 : (want > 128 ? 128 : want)));
  lds_out = lds;
  return MI_OK;
}

constexpr uint64_t kPlanMagic = 0x6d695f67726f7570ull;   // "mi_group"
// a plan whose members have nd numeric columns: kPlanMagicNumeric + nd, so that the entries without an x_num know it
constexpr uint64_t kPlanMagicNumeric = 0x6d695f6e756d0000ull;   // "mi_num", then nd
int plan_numeric(const mi_fused_group_plan_t* plan) {           // nd of a plan (0: none), -1: not a plan
  if (!plan || !plan->device_table) return -1;
  if (plan->magic == kPlanMagic) return 0;
  const uint64_t nd = plan->magic - kPlanMagicNumeric;
  return (nd >= 1 && nd <= static_cast<uint64_t>(kMaxNumeric)) ? static_cast<int>(nd) : -1;
}
constexpr int kGroupGridBlocks = 1 << 16;                // the built-in sweep_blocks keeps (1 + G) M at or below this
constexpr int kEvalResident = 4 * 256;                   // workgroups of one evaluation launch (the built-in choice)

// one step of one model: mi_train_step_fused, mi_train_step_model and mi_train_step_model_numeric behind their own checks
int32_t step_one(const mi_fused_model_t& m, const mi_fused_numeric_t* num, const int64_t* field_off, const int32_t* ids,
                 const float* x_num, const uint8_t* labels, int64_t B, int32_t F, uint64_t seed, int32_t step, float* logits,
                 float* loss, int32_t sweep_blocks, mi_stream_t stream) {
  Args a;
  size_t lds = 0;
  int blocks = 0;
  const int32_t rc = plan_model(m, num, field_off, B, F, step, ids && labels, logits && loss, sweep_blocks, a, lds, blocks);
  if (rc != MI_OK) return rc;
  MI_REQUIRE(a.nd == 0 || x_num, "train_step_fused: x_num (the model has %d numeric columns)", a.nd);
  a.ids = ids; a.labels = labels; a.logits = logits; a.loss = loss; a.seed = seed; a.step = step;
  a.x_num = a.nd ? x_num : nullptr;
  const int32_t rl = mi::raise_lds(&train_fused_k, lds, "train_step_fused");
  if (rl != MI_OK) return rl;
  train_fused_k<<<dim3(1 + blocks), dim3(kThreads), lds, mi::as_stream(stream)>>>(a);       // (no Adam part: the batch workgroup alone)
  MI_CHECK_LAUNCH("train_step_fused");
  return MI_OK;
}

// mi_train_group_plan (adam_only: its members, behind that entry's refusal), mi_train_group_plan_models and
// mi_train_group_plan_models_numeric: model(i) is member i's description, numerics[i] its numeric columns (NULL: none)
template <typename Get>
int32_t plan_group(Get model, const mi_fused_numeric_t* numerics, bool adam_only, int32_t n_members, int64_t B, int32_t F,
                   const int64_t* field_off, void* device_table, size_t device_table_bytes, mi_fused_group_plan_t* plan,
                   mi_stream_t stream) {
  MI_REQUIRE(plan, "train_group_plan: plan");
  MI_REQUIRE(n_members >= 1, "train_group_plan: %d members (at least 1)", n_members);
  if (n_members > MI_FUSED_GROUP_MAX_MEMBERS)
    return unsupported("train_group_plan: %d members (at most %d in one launch)", n_members, MI_FUSED_GROUP_MAX_MEMBERS);
  const size_t need = mi_train_group_plan_bytes(n_members);
  if (!device_table || device_table_bytes < need) {
    mi::set_error("train_group_plan: device table of %zu bytes, %zu needed", device_table_bytes, need);
    return MI_ERR_WORKSPACE;
  }
  MI_REQUIRE(mi::aligned16(device_table), "train_group_plan: device_table (16-byte aligned)");
  struct Owned { const void* p; int32_t member; };
  constexpr int kOwned = 13;
  const std::unique_ptr<Member[]> tab(new (std::nothrow) Member[n_members]);
  const std::unique_ptr<Owned[]> owned(new (std::nothrow) Owned[kOwned * static_cast<size_t>(n_members)]);
  MI_REQUIRE(tab && owned, "train_group_plan: out of host memory");
  size_t n_owned = 0, lds = 0;
  int blocks = 0;
  int64_t max_step = INT32_MAX;
  const int32_t nd = numerics ? numerics[0].n_numeric : 0;       // (one set of feature columns: the members share it, like F)
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_fused_model_t m = model(i);
    size_t lds_i = 0;
    int blocks_i = 0;
    int32_t rc = MI_OK;
    if (adam_only && m.hp.kind != MI_OPT_ADAM) rc = unsupported("train_step_fused: optimizer kind %d (Adam only)", m.hp.kind);
    if (rc == MI_OK && numerics && numerics[i].n_numeric != nd) {
      mi::set_error("train_step_fused: %d numeric columns, member 0 has %d (the members share one set of feature columns)",
                    numerics[i].n_numeric, nd);
      rc = MI_ERR_INVALID;
    }
    if (rc == MI_OK) rc = plan_model(m, numerics ? numerics + i : nullptr, field_off, B, F, 1, true, true, 0, tab[i].a, lds_i, blocks_i);
    // a schedule table exactly for a rule that is Adam (with one rule the wide part reads hp's)
    const bool t_adam = m.hp.kind == MI_OPT_ADAM, w_adam = m.two_rules && m.hp_wide.kind == MI_OPT_ADAM;
    if (rc == MI_OK && t_adam && (!m.lr_table || m.lr_table_len < 2)) {
      mi::set_error("train_step_fused: lr_table of %lld entries (lr_t of step s at [s], s >= 1)", (long long)m.lr_table_len);
      rc = MI_ERR_INVALID;
    }
    if (rc == MI_OK && w_adam && (!m.lr_table_wide || m.lr_table_wide_len < 2)) {
      mi::set_error("train_step_fused: lr_table_wide of %lld entries (lr_t of step s at [s], s >= 1)", (long long)m.lr_table_wide_len);
      rc = MI_ERR_INVALID;
    }
    if (rc != MI_OK) {
      mi::member_error("train_group_plan", i);
      return rc;
    }
    tab[i].lr_table = t_adam ? m.lr_table : nullptr; tab[i].lr_len = t_adam ? m.lr_table_len : 0;
    tab[i].lr_table_w = m.two_rules ? (w_adam ? m.lr_table_wide : nullptr) : tab[i].lr_table;
    tab[i].lr_len_w = m.two_rules ? (w_adam ? m.lr_table_wide_len : 0) : tab[i].lr_len;
    tab[i].seed_base = m.seed_base;
    if (lds_i > lds) lds = lds_i;
    if (blocks_i > blocks) blocks = blocks_i;
    if (t_adam && m.lr_table_len - 1 < max_step) max_step = m.lr_table_len - 1;
    if (w_adam && m.lr_table_wide_len - 1 < max_step) max_step = m.lr_table_wide_len - 1;
    const Args& a = tab[i].a;
    const void* own[kOwned] = {a.table, a.tm, a.tv, a.lin_w, a.lm, a.lv, a.last_step, a.dense, a.dm, a.dv,
                               m.two_rules ? a.dwm : nullptr, m.two_rules ? a.dwv : nullptr, m.workspace};
    for (const void* p : own)
      if (p) owned[n_owned++] = Owned{p, i};
  }
  // two members (or two roles of one member) on the same memory: every pointer above is written by its member's workgroups
  qsort(owned.get(), n_owned, sizeof(Owned), [](const void* x, const void* y) {
    const Owned* a = static_cast<const Owned*>(x);
    const Owned* b = static_cast<const Owned*>(y);
    return a->p < b->p ? -1 : (a->p > b->p ? 1 : (a->member < b->member ? -1 : (a->member > b->member ? 1 : 0)));
  });
  for (size_t j = 1; j < n_owned; ++j)
    MI_REQUIRE(owned[j].p != owned[j - 1].p,
               "train_group_plan: member %d and member %d share a state or workspace pointer (%p): members are independent",
               owned[j - 1].member, owned[j].member, owned[j].p);
  const int32_t rc = mi::upload_table(device_table, tab.get(), need, stream, "train_group_plan");
  if (rc != MI_OK) return rc;
  while (blocks > 1 && static_cast<int64_t>(1 + blocks) * n_members > kGroupGridBlocks) --blocks;
  plan->device_table = device_table; plan->n_members = n_members; plan->B = static_cast<int32_t>(B); plan->F = F;
  plan->lds_bytes = static_cast<uint32_t>(lds); plan->sweep_blocks = blocks; plan->max_step = static_cast<int32_t>(max_step);
  plan->magic = nd ? kPlanMagicNumeric + static_cast<uint64_t>(nd) : kPlanMagic;
  return MI_OK;
}

// mi_train_group_step and mi_train_group_step_numeric behind their plan checks (nd: the plan's numeric columns)
int32_t group_step(const mi_fused_group_plan_t* plan, int nd, int32_t n_members, const int32_t* ids, int64_t ids_member_stride,
                   const float* x_num, int64_t x_member_stride, const uint8_t* labels, int64_t labels_member_stride, int64_t B,
                   int32_t step, float* logits, float* loss, int32_t sweep_blocks, mi_stream_t stream) {
  MI_REQUIRE(n_members == plan->n_members, "train_group_step: %d members, the plan has %d", n_members, plan->n_members);
  MI_REQUIRE(B == plan->B, "train_group_step: B=%lld, the plan was made for %d", (long long)B, plan->B);
  MI_REQUIRE(step >= 1, "train_group_step: step=%d (the global step after this call, 1-based)", step);
  MI_REQUIRE(step <= plan->max_step, "train_group_step: step=%d, the shortest lr_table of the plan ends at %d", step, plan->max_step);
  MI_REQUIRE(ids && labels && logits && loss, "train_group_step: ids / labels / logits / loss");
  MI_REQUIRE(ids_member_stride == 0 || ids_member_stride == B * plan->F,
             "train_group_step: ids_member_stride=%lld (0 = one batch for all members, or B F = %lld)",
             (long long)ids_member_stride, (long long)(B * plan->F));
  MI_REQUIRE(nd == 0 || x_num, "train_group_step: x_num (the plan's members have %d numeric columns)", nd);
  MI_REQUIRE(nd == 0 || x_member_stride == 0 || x_member_stride == B * nd,
             "train_group_step: x_num_member_stride=%lld (0 = one batch for all members, or B n_numeric = %lld)",
             (long long)x_member_stride, (long long)(B * nd));
  MI_REQUIRE(labels_member_stride == 0 || labels_member_stride == B,
             "train_group_step: labels_member_stride=%lld (0 = one batch for all members, or B = %lld)",
             (long long)labels_member_stride, (long long)B);
  if (sweep_blocks < 0 || sweep_blocks > kMaxSweepBlocks)
    return unsupported("train_group_step: sweep_blocks=%d (0 = the built-in choice, at most %d)", sweep_blocks, kMaxSweepBlocks);
  // (a plan without any part under Adam has no sweep: the batch workgroups alone, whatever sweep_blocks says)
  const int blocks = plan->sweep_blocks == 0 ? 0 : (sweep_blocks ? sweep_blocks : plan->sweep_blocks);
  MI_REQUIRE(blocks >= 0 && blocks <= kMaxSweepBlocks && plan->lds_bytes <= kMaxLds, "train_group_step: plan (damaged)");
  const int32_t rl = mi::raise_lds(&train_fused_group_k, plan->lds_bytes, "train_group_step");
  if (rl != MI_OK) return rl;
  train_fused_group_k<<<dim3(1 + blocks, n_members), dim3(kThreads), plan->lds_bytes, mi::as_stream(stream)>>>(
      static_cast<const Member*>(plan->device_table), ids, ids_member_stride, nd ? x_num : nullptr, nd ? x_member_stride : 0,
      labels, labels_member_stride, logits, loss, step);
  MI_CHECK_LAUNCH("train_group_step");
  return MI_OK;
}

// mi_eval_group and mi_eval_group_numeric behind their plan checks
int32_t eval_group(const mi_fused_group_plan_t* plan, int nd, int32_t n_members, const int32_t* ids, const float* x_num,
                   int64_t x_member_stride, const uint8_t* labels, int64_t N, const float* tail_scale, float* logits,
                   float* batch_loss, int64_t* hist, int64_t* counts, double* partials, int32_t blocks, mi_stream_t stream) {
  MI_REQUIRE(n_members == plan->n_members, "eval_group: %d members, the plan has %d", n_members, plan->n_members);
  MI_REQUIRE(N >= 1 && N <= INT32_MAX, "eval_group: N=%lld examples (1 to %d)", (long long)N, INT32_MAX);
  MI_REQUIRE(ids && labels, "eval_group: ids / labels");
  MI_REQUIRE(nd == 0 || x_num, "eval_group: x_num (the plan's members have %d numeric columns)", nd);
  MI_REQUIRE(nd == 0 || x_member_stride == 0 || x_member_stride == N * nd,
             "eval_group: x_num_member_stride=%lld (0 = one set for all members, or N n_numeric = %lld)",
             (long long)x_member_stride, (long long)(N * nd));
  MI_REQUIRE(batch_loss && hist && counts && partials, "eval_group: batch_loss / hist / counts / partials");
  MI_REQUIRE(plan->B >= 1 && plan->B <= kMaxBatch && plan->lds_bytes <= kMaxLds, "eval_group: plan (damaged)");
  MI_REQUIRE(N % plan->B == 0 || tail_scale, "eval_group: tail_scale (the last tile has %lld of %d examples)",
             (long long)(N % plan->B), plan->B);
  if (blocks < 0 || blocks > kMaxSweepBlocks)
    return unsupported("eval_group: blocks=%d (0 = the built-in choice, at most %d)", blocks, kMaxSweepBlocks);
  const int64_t T = mi::ceil_div(N, plan->B);
  // built-in X: kEvalResident workgroups in all (4 per compute unit of the 256, twice the 2 that 127 VGPRs let run side by
  // side, so a workgroup that ends early is followed by another), shared out among the members, never more than a member has
  // tiles; X M stays inside the training launch's 65536 workgroups
  int64_t X = blocks;
  if (!X) {
    X = kEvalResident / n_members;
    if (X < 1) X = 1;
    if (X > T) X = T;
  }
  MI_REQUIRE(X * n_members <= kGroupGridBlocks, "eval_group: blocks=%d for %d members (at most %d workgroups in all)", blocks,
             n_members, kGroupGridBlocks);
  const size_t lds = plan->lds_bytes < kMaxForwardLds ? plan->lds_bytes : kMaxForwardLds;
  const int32_t rl = mi::raise_lds(&eval_fused_group_k, lds, "eval_group");
  if (rl != MI_OK) return rl;
  eval_fused_group_k<<<dim3(static_cast<unsigned>(X), n_members), dim3(kThreads), lds, mi::as_stream(stream)>>>(
      static_cast<const Member*>(plan->device_table), ids, nd ? x_num : nullptr, nd ? x_member_stride : 0, labels, N, T,
      tail_scale, logits, batch_loss, reinterpret_cast<unsigned long long*>(hist),
      reinterpret_cast<unsigned long long*>(counts), partials);
  MI_CHECK_LAUNCH("eval_group");
  return MI_OK;
}

}  // namespace

extern "C" {

size_t mi_train_step_fused_workspace_bytes(int64_t B, int32_t F, int32_t E, int64_t n_dense) {
  return workspace_bytes_of(B, F, 0, E, n_dense);
}

size_t mi_train_step_fused_workspace_bytes_numeric(int64_t B, int32_t F, int32_t n_numeric, int32_t E, int64_t n_dense) {
  return workspace_bytes_of(B, F, n_numeric, E, n_dense);
}

int32_t mi_train_step_fused(float* table, float* t_m, float* t_v, int64_t table_stride, float* lin_w, float* l_m, float* l_v,
                            int32_t lin_stride, int32_t* last_step, const int64_t* field_off, int64_t R, const int32_t* ids,
                            const uint8_t* labels, int64_t B, int32_t F, int32_t E, float* dense, float* d_m, float* d_v,
                            int64_t n_dense, const int64_t* layer_off, const int32_t* widths, int32_t n_layers,
                            int32_t activation, int32_t use_linear, int32_t use_fm, int32_t use_dnn, int64_t lin_bias_off,
                            float keep_prob, uint64_t seed, float scale, int32_t step, const mi_opt_hparams* hp,
                            float* logits, float* loss, int32_t sweep_blocks, void* workspace, size_t workspace_bytes,
                            mi_stream_t stream) {
  MI_REQUIRE(hp, "train_step_fused: hp");
  mi_fused_member_t m{};                 // (lr_table, lr_table_len and seed_base stay unused: the call brings lr_t and the seed)
  m.table = table; m.t_m = t_m; m.t_v = t_v; m.table_stride = table_stride;
  m.lin_w = lin_w; m.l_m = l_m; m.l_v = l_v; m.lin_stride = lin_stride;
  m.last_step = last_step; m.R = R; m.E = E;
  m.dense = dense; m.d_m = d_m; m.d_v = d_v; m.n_dense = n_dense;
  m.layer_off = layer_off; m.widths = widths; m.n_layers = n_layers; m.activation = activation;
  m.use_linear = use_linear; m.use_fm = use_fm; m.use_dnn = use_dnn; m.lin_bias_off = lin_bias_off;
  m.keep_prob = keep_prob; m.scale = scale; m.hp = *hp;
  m.workspace = workspace; m.workspace_bytes = workspace_bytes;
  if (hp->kind != MI_OPT_ADAM) return unsupported("train_step_fused: optimizer kind %d (Adam only)", hp->kind);
  return step_one(model_of(m, F), nullptr, field_off, ids, nullptr, labels, B, F, seed, step, logits, loss, sweep_blocks, stream);
}

int32_t mi_train_step_model(const mi_fused_model_t* model, const int64_t* field_off, const int32_t* ids, const uint8_t* labels,
                            int64_t B, int32_t F, uint64_t seed, int32_t step, float* logits, float* loss, int32_t sweep_blocks,
                            mi_stream_t stream) {
  MI_REQUIRE(model, "train_step_fused: model");
  return step_one(*model, nullptr, field_off, ids, nullptr, labels, B, F, seed, step, logits, loss, sweep_blocks, stream);
}

int32_t mi_train_step_model_numeric(const mi_fused_model_t* model, const mi_fused_numeric_t* numeric, const int64_t* field_off,
                                    const int32_t* ids, const float* x_num, const uint8_t* labels, int64_t B, int32_t F,
                                    uint64_t seed, int32_t step, float* logits, float* loss, int32_t sweep_blocks,
                                    mi_stream_t stream) {
  MI_REQUIRE(model, "train_step_fused: model");
  return step_one(*model, numeric, field_off, ids, x_num, labels, B, F, seed, step, logits, loss, sweep_blocks, stream);
}

size_t mi_train_group_plan_bytes(int32_t n_members) {
  return n_members < 0 ? 0 : sizeof(Member) * static_cast<size_t>(n_members);
}

int32_t mi_train_group_plan(const mi_fused_member_t* members, int32_t n_members, int64_t B, int32_t F, const int64_t* field_off,
                            void* device_table, size_t device_table_bytes, mi_fused_group_plan_t* plan, mi_stream_t stream) {
  MI_REQUIRE(plan, "train_group_plan: plan");
  MI_REQUIRE(n_members >= 1, "train_group_plan: %d members (at least 1)", n_members);
  if (n_members > MI_FUSED_GROUP_MAX_MEMBERS)
    return unsupported("train_group_plan: %d members (at most %d in one launch)", n_members, MI_FUSED_GROUP_MAX_MEMBERS);
  MI_REQUIRE(members, "train_group_plan: members");
  return plan_group([&](int32_t i) { return model_of(members[i], F); }, nullptr, true, n_members, B, F, field_off, device_table,
                    device_table_bytes, plan, stream);
}

int32_t mi_train_group_plan_models(const mi_fused_model_t* models, int32_t n_members, int64_t B, int32_t F,
                                   const int64_t* field_off, void* device_table, size_t device_table_bytes,
                                   mi_fused_group_plan_t* plan, mi_stream_t stream) {
  MI_REQUIRE(plan, "train_group_plan: plan");
  MI_REQUIRE(n_members >= 1, "train_group_plan: %d members (at least 1)", n_members);
  if (n_members > MI_FUSED_GROUP_MAX_MEMBERS)
    return unsupported("train_group_plan: %d members (at most %d in one launch)", n_members, MI_FUSED_GROUP_MAX_MEMBERS);
  MI_REQUIRE(models, "train_group_plan: models");
  return plan_group([&](int32_t i) { return models[i]; }, nullptr, false, n_members, B, F, field_off, device_table,
                    device_table_bytes, plan, stream);
}

int32_t mi_train_group_plan_models_numeric(const mi_fused_model_t* models, const mi_fused_numeric_t* numerics, int32_t n_members,
                                           int64_t B, int32_t F, const int64_t* field_off, void* device_table,
                                           size_t device_table_bytes, mi_fused_group_plan_t* plan, mi_stream_t stream) {
  MI_REQUIRE(plan, "train_group_plan: plan");
  MI_REQUIRE(n_members >= 1, "train_group_plan: %d members (at least 1)", n_members);
  if (n_members > MI_FUSED_GROUP_MAX_MEMBERS)
    return unsupported("train_group_plan: %d members (at most %d in one launch)", n_members, MI_FUSED_GROUP_MAX_MEMBERS);
  MI_REQUIRE(models, "train_group_plan: models");
  return plan_group([&](int32_t i) { return models[i]; }, numerics, false, n_members, B, F, field_off, device_table,
                    device_table_bytes, plan, stream);
}

int32_t mi_train_group_step(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids, int64_t ids_member_stride,
                            const uint8_t* labels, int64_t labels_member_stride, int64_t B, int32_t step, float* logits,
                            float* loss, int32_t sweep_blocks, mi_stream_t stream) {
  const int nd = plan_numeric(plan);
  MI_REQUIRE(nd >= 0, "train_group_step: plan (not written by mi_train_group_plan)");
  MI_REQUIRE(nd == 0, "train_group_step: the plan's members have %d numeric columns and this entry brings no x_num "
             "(mi_train_group_step_numeric does)", nd);
  return group_step(plan, 0, n_members, ids, ids_member_stride, nullptr, 0, labels, labels_member_stride, B, step, logits, loss,
                    sweep_blocks, stream);
}

int32_t mi_train_group_step_numeric(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids,
                                    int64_t ids_member_stride, const float* x_num, int64_t x_num_member_stride,
                                    const uint8_t* labels, int64_t labels_member_stride, int64_t B, int32_t step, float* logits,
                                    float* loss, int32_t sweep_blocks, mi_stream_t stream) {
  const int nd = plan_numeric(plan);
  MI_REQUIRE(nd >= 0, "train_group_step: plan (not written by mi_train_group_plan)");
  return group_step(plan, nd, n_members, ids, ids_member_stride, x_num, x_num_member_stride, labels, labels_member_stride, B,
                    step, logits, loss, sweep_blocks, stream);
}

int32_t mi_eval_group(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids, const uint8_t* labels, int64_t N,
                      const float* tail_scale, float* logits, float* batch_loss, int64_t* hist, int64_t* counts, double* partials,
                      int32_t blocks, mi_stream_t stream) {
  const int nd = plan_numeric(plan);
  MI_REQUIRE(nd >= 0, "eval_group: plan (not written by mi_train_group_plan)");
  MI_REQUIRE(nd == 0, "eval_group: the plan's members have %d numeric columns and this entry brings no x_num "
             "(mi_eval_group_numeric does)", nd);
  return eval_group(plan, 0, n_members, ids, nullptr, 0, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks,
                    stream);
}

int32_t mi_eval_group_numeric(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids, const float* x_num,
                              int64_t x_num_member_stride, const uint8_t* labels, int64_t N, const float* tail_scale,
                              float* logits, float* batch_loss, int64_t* hist, int64_t* counts, double* partials, int32_t blocks,
                              mi_stream_t stream) {
  const int nd = plan_numeric(plan);
  MI_REQUIRE(nd >= 0, "eval_group: plan (not written by mi_train_group_plan)");
  return eval_group(plan, nd, n_members, ids, x_num, x_num_member_stride, labels, N, tail_scale, logits, batch_loss, hist, counts,
                    partials, blocks, stream);
}

}  // extern "C"
