// Top-K recommendation: every (query, candidate) pair scored by the model and the best K candidates of each query kept,
// without the pair matrix ever reaching HBM (mi_pair_topk, include/mi355x_rec.h).
//
// The model splits over the two sides of a pair (Q = query fields, C = candidate fields):
//   logit(q, c) = w_q + w_c + s_q . s_c + MLP_{2..L}(act(a_q + a_c))
// with w = lin + fm of the side (the candidate side also carries the wide bias), s = the side's sum of embeddings and
// a = the side's rows of layer 1 (b1 on the candidate side).  The caller computes the per-side tensors with the existing
// entry points; what is left per pair runs here.
//
//   pair_score_topk_k  grid (query blocks of 32) x (candidate splits).  A wave scores ONE candidate against the
//                      workgroup's 32 queries: h1 = act(a_q + a_c) is formed in registers as it is consumed, layers
//                      2..L-1 run on the fp32-input MFMA in the transposed form Y^T = W^T X^T (the 32 pairs are the
//                      MFMA's columns, so a layer's accumulators are the next layer's B operand with no LDS round trip;
//                      the weights' k order follows the accumulator's row map), the logits layer is a dot product.
//                      Narrow MLPs (every width after layer 1 below 32) take a VALU loop instead.  Each query keeps a
//                      sorted top-K list in LDS; a candidate that does not beat the list's K-th key is rejected by one
//                      64-bit compare, survivors are appended and merged into the list in batches (rank merge).
//   topk_merge_k       one workgroup per query: the splits' partial lists merged into the final [U, K].
//
// The pair kernels are a 2 x 2 — how a pair is scored, by what is done with the score:
//                                     keep the best K                  count the keys above named targets (count_ranks)
//   one model's logit                 pair_score_topk_k (written out)  pair_target_ranks_k: SoloScorer, members on grid z
//   the members' mean (MeanScorer)    pair_score_topk_group_k          pair_target_ranks_mean_k
//                                     (select_topk)
// A scorer answers "the score of candidate c for this lane's query"; a body owns the LDS and what is written.  The three
// kernels that read the member table build a scorer and call a body; the mean is formed in MeanScorer alone, the counting
// loop stands in count_ranks alone.  pair_score_topk_k states its selection itself (see there for why) and select_topk
// restates it for the mean.  rank_sum_k adds the splits' counts of the two on the right.
//
// Order: one 64-bit key per (score, candidate): the score's bits made monotone in the high word (NaN -> 0, below every
// number; -0 as +0, and returned as +0), the complemented index in the low word, so "larger key" = higher score, then lower index.  Key 0 is
// the empty slot.  Keys of one query are distinct, so every merge is a rank computation with one answer: the results do
// not depend on the split count, the order in which waves append survivors, or timing.  No workgroup waits for another.
#include "common.h"
#include "score_key.h"

namespace {

constexpr int kQB = 32;                 // queries per workgroup = the MFMA's N
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kSurv = 64;               // survivor slots per query between merges (one round adds at most kWaves)
constexpr int kMaxK = 256;
constexpr int kMaxLayers = 8;           // layers after layer 1 (hidden layers 2..L-1 and the logits layer)
constexpr int kMaxH1 = 4096;
constexpr int kMaxRegWidth = 256;       // widths held in registers: layers 2, 4, ... (layers 3, 5, ...: half of it)
constexpr int kTargetBlocks = 512;      // workgroups the split count aims at (two per CU of an MI355X)
constexpr int kMergeLds = 64 * 1024;    // the final merge's LDS image of one query's partial lists

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Layer {
  int64_t w_off, b_off;                 // offsets into the flat dense buffer: kernel [fan_in, fan_out], bias [fan_out]
  int32_t fan_in, fan_out;
};

// one model as pair_score and the dnn_* functions read it
struct ScoreArgs {
  const float* aqT;                     // [H1][Upad] (workspace: a_q transposed, zero columns past U)
  const float* a_c;                     // [I][H1]
  const float* sqT;                     // [E][Upad]
  const float* s_c;                     // [I][E]
  const float* w_q;                     // [U] or NULL
  const float* w_c;                     // [I] or NULL
  const float* dense;
  const Layer* l;                       // [n_layers] (workspace; a table in the kernel arguments would be copied to
                                        // scratch by the runtime-indexed reads)
  int32_t Upad, H1, E, act, n_layers;
};

// what select_topk does with the scores
struct SelectArgs {
  const uint32_t* excl;                 // [U][words] bitmask or NULL
  float* scores;                        // [U][I] or NULL
  uint64_t* part;                       // [U][splits][K]
  int64_t U, I, chunk;
  int32_t K, splits, words;
};

// what count_ranks does with them
struct RanksArgs {
  const uint32_t* excl;                 // [U][words] bitmask or NULL
  const int32_t* targets;               // [U][Tq]
  float* target_scores;                 // [members on the grid][U][Tq] or NULL
  int32_t* part;                        // [members on the grid][splits][U][Tq]
  int64_t U, I, chunk;
  int32_t Tq, splits, words;
};

struct LayerTable {
  Layer l[kMaxLayers];
};

__device__ __forceinline__ uint64_t rank_key(float s, uint32_t c) {
  return (static_cast<uint64_t>(mi_score_key32(s)) << 32) | static_cast<uint32_t>(~c);
}
__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t u = static_cast<uint32_t>(key >> 32);
  if (u == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ int32_t key_index(uint64_t key) { return static_cast<int32_t>(~static_cast<uint32_t>(key)); }

// row of a 32x32 accumulator tile held in register r by lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- MFMA path ------------------------------------------------------------------------------------------------------
// y[b] (feature b*32 + acc_row(r, h), pair = lane & 31) <- act(y + bias), zero past N
template <int NB>
__device__ __forceinline__ void epilogue(f32x16 (&y)[NB], const float* __restrict__ bias, int N, int act, int h) {
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = b * 32 + acc_row(r, h);
      y[b][r] = n < N ? mi_act(act, y[b][r] + bias[n]) : 0.f;
    }
  }
}

// layer 2: the input h1 = act(a_q + a_c) is made as it is consumed, two k per MFMA step
template <int NB, class Args>
__device__ __forceinline__ void layer2_mfma(const Args& p, const float* __restrict__ ac, int64_t qcol, int h,
                                            f32x16 (&y)[NB]) {
  const int col = static_cast<int>(qcol & 31);
  const Layer L = p.l[0];
  const float* __restrict__ W = p.dense + L.w_off;
  const int K = L.fan_in, N = L.fan_out;
#pragma unroll
  for (int b = 0; b < NB; ++b) y[b] = f32x16{};
  for (int k0 = 0; k0 < K; k0 += 2) {
    const int k = k0 + h;
    float hv = 0.f;
    if (k < K) hv = mi_act(p.act, p.aqT[static_cast<int64_t>(k) * p.Upad + qcol] + ac[k]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b * 32 >= N) break;
      const int n = b * 32 + col;
      const float w = (k < K && n < N) ? W[static_cast<int64_t>(k) * N + n] : 0.f;
      y[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, hv, y[b], 0, 0, 0);
    }
  }
  epilogue<NB>(y, p.dense + L.b_off, N, p.act, h);
}

// a hidden layer whose input x is in registers: k-step (bi, r) takes the lane's own x[bi][r] as B and the weight row
// of that feature as A
template <int NI, int NO, class Args>
__device__ __forceinline__ void layer_mfma(const Args& p, const Layer L, const f32x16 (&x)[NI], f32x16 (&y)[NO],
                                           int col, int h) {
  const float* __restrict__ W = p.dense + L.w_off;
  const int K = L.fan_in, N = L.fan_out;
#pragma unroll
  for (int b = 0; b < NO; ++b) y[b] = f32x16{};
#pragma unroll
  for (int bi = 0; bi < NI; ++bi) {
    if (bi * 32 < K) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = bi * 32 + acc_row(r, h);
#pragma unroll
      for (int bo = 0; bo < NO; ++bo) {
        if (bo * 32 >= N) break;
        const int n = bo * 32 + col;
        const float w = (k < K && n < N) ? W[static_cast<int64_t>(k) * N + n] : 0.f;
        y[bo] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, x[bi][r], y[bo], 0, 0, 0);
      }
    }
    }
  }
  epilogue<NO>(y, p.dense + L.b_off, N, p.act, h);
}

template <int NB, class Args>
__device__ __forceinline__ float logits_mfma(const Args& p, const Layer L, const f32x16 (&x)[NB], int h) {
  const float* __restrict__ W = p.dense + L.w_off;
  float s = 0.f;
#pragma unroll
  for (int bi = 0; bi < NB; ++bi) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = bi * 32 + acc_row(r, h);
      if (k < L.fan_in) s = fmaf(x[bi][r], W[k], s);
    }
  }
  s += __shfl_xor(s, 32);
  return s + p.dense[L.b_off];
}

// the outputs of layers 2, 4, ... live in y (NP tiles of 32 features), those of layers 3, 5, ... in x (NQ tiles)
template <int NP, int NQ, class Args>
__device__ __forceinline__ float dnn_mfma(const Args& p, const float* __restrict__ ac, int64_t qcol, int h) {
  const int col = static_cast<int>(qcol & 31);
  f32x16 y[NP], x[NQ];
  layer2_mfma<NP>(p, ac, qcol, h, y);
  int i = 1;
  while (true) {                       // ping-pong between the two register tiles
    if (i == p.n_layers - 1) return logits_mfma<NP>(p, p.l[i], y, h);
    layer_mfma<NP, NQ>(p, p.l[i], y, x, col, h);
    ++i;
    if (i == p.n_layers - 1) return logits_mfma<NQ>(p, p.l[i], x, h);
    layer_mfma<NQ, NP>(p, p.l[i], x, y, col, h);
    ++i;
  }
}

// ---- VALU path: one lane per pair (lanes 32..63 repeat lanes 0..31); widths after layer 1 at most 32 ---------------
constexpr int kValuW = 32;

__device__ __forceinline__ void epilogue_valu(float (&y)[kValuW], const float* __restrict__ bias, int N, int act) {
#pragma unroll
  for (int j = 0; j < kValuW; ++j) y[j] = j < N ? mi_act(act, y[j] + bias[j]) : 0.f;
}

template <class Args>
__device__ __forceinline__ void layer_valu(const Args& p, const Layer L, const float (&x)[kValuW], float (&y)[kValuW]) {
  const float* __restrict__ W = p.dense + L.w_off;
  const int K = L.fan_in, N = L.fan_out;
#pragma unroll
  for (int j = 0; j < kValuW; ++j) y[j] = 0.f;
#pragma unroll
  for (int k = 0; k < kValuW; ++k) {
#pragma unroll
    for (int j = 0; j < kValuW; ++j)
      if (k < K && j < N) y[j] = fmaf(x[k], W[k * N + j], y[j]);
  }
  epilogue_valu(y, p.dense + L.b_off, N, p.act);
}

template <class Args>
__device__ __forceinline__ float logits_valu(const Args& p, const Layer L, const float (&x)[kValuW]) {
  const float* __restrict__ W = p.dense + L.w_off;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kValuW; ++k)
    if (k < L.fan_in) s = fmaf(x[k], W[k], s);
  return s + p.dense[L.b_off];
}

template <class Args>
__device__ __forceinline__ float dnn_valu(const Args& p, const float* __restrict__ ac, int64_t qcol) {
  const int H1 = p.H1;
  const float* __restrict__ aq = p.aqT + qcol;
  if (p.n_layers == 0) return aq[0] + ac[0];                      // no hidden layer: layer 1 is the logits layer
  if (p.n_layers == 1) {                                           // one hidden layer: its output meets the logits weights
    const Layer L = p.l[0];
    const float* __restrict__ W = p.dense + L.w_off;
    float s = 0.f;
    for (int k = 0; k < H1; ++k) s = fmaf(mi_act(p.act, aq[static_cast<int64_t>(k) * p.Upad] + ac[k]), W[k], s);
    return s + p.dense[L.b_off];
  }
  float x[kValuW], y[kValuW];
  {
    const Layer L = p.l[0];
    const float* __restrict__ W = p.dense + L.w_off;
    const int N = L.fan_out;
#pragma unroll
    for (int j = 0; j < kValuW; ++j) y[j] = 0.f;
    for (int k = 0; k < H1; ++k) {
      const float hv = mi_act(p.act, aq[static_cast<int64_t>(k) * p.Upad] + ac[k]);
#pragma unroll
      for (int j = 0; j < kValuW; ++j)
        if (j < N) y[j] = fmaf(hv, W[k * N + j], y[j]);
    }
    epilogue_valu(y, p.dense + L.b_off, N, p.act);
  }
  int i = 1;
  while (true) {
    if (i == p.n_layers - 1) return logits_valu(p, p.l[i], y);
    layer_valu(p, p.l[i], y, x);
    ++i;
    if (i == p.n_layers - 1) return logits_valu(p, p.l[i], x);
    layer_valu(p, p.l[i], x, y);
    ++i;
  }
}

// ---- the score of one pair -------------------------------------------------------------------------------------------
// logit(q, c) of the model p for candidate c and the lane's query column qcol: the DNN on act(a_q + a_c), the E-wide dot of
// the two embedding sums, and the head's order ((w_q + w_c) + dot) + dnn.  wq / sq: the lane's w_q and its column of sqT
// (NULL without the FM term).  Every scorer calls this: a group member's score is its own kernel's, bit for bit
// (every product is an explicit fmaf and no multiply feeds an add, so there is nothing for the compiler to contract).
template <bool MFMA, int NP, int NQ, class Args>
__device__ __forceinline__ float pair_score(const Args& p, int64_t c, int64_t qcol, int h, float wq,
                                            const float* __restrict__ sq) {
  float dnn = 0.f;
  if (p.H1 > 0) {
    const float* __restrict__ ac = p.a_c + c * p.H1;
    if constexpr (MFMA) dnn = dnn_mfma<NP, NQ>(p, ac, qcol, h);
    else dnn = dnn_valu(p, ac, qcol);
  }
  float dot = 0.f;
  if (sq) {
    const float* __restrict__ sc = p.s_c + c * p.E;
    for (int e = 0; e < p.E; ++e) dot = fmaf(sq[static_cast<int64_t>(e) * p.Upad], sc[e], dot);
  }
  return ((wq + (p.w_c ? p.w_c[c] : 0.f)) + dot) + dnn;
}

// ---- selection --------------------------------------------------------------------------------------------------------
// Merge every query's survivors into its sorted list: a list entry moves down by the survivors that beat it, a survivor
// lands at (list entries that beat it) + (survivors that beat it).  Entries pushed to K or beyond drop out; empty slots
// (key 0) are beaten by every survivor, so they fill the tail.  Wave w owns queries w, w + 4, ...
__device__ __forceinline__ void merge_survivors(uint64_t* list, const uint64_t* surv, int* nsurv, int K, int wave, int lane) {
  constexpr int kPer = kMaxK / 64;
  for (int qq = wave; qq < kQB; qq += kWaves) {                   // the same trip count in every wave: barriers inside
    uint64_t* L = list + qq * K;
    const uint64_t* S = surv + qq * kSurv;
    const int n = nsurv[qq];
    uint64_t lv[kPer];
    int lp[kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      const int j = lane + 64 * t;
      lv[t] = 0;
      lp[t] = K;
      if (j < K && n > 0) {
        lv[t] = L[j];
        int cnt = 0;
        for (int u = 0; u < n; ++u) cnt += S[u] > lv[t];
        lp[t] = j + cnt;
      }
    }
    uint64_t sv = 0;
    int sp = K;
    if (lane < n) {
      sv = S[lane];
      int cnt = 0;
      for (int u = 0; u < n; ++u) cnt += S[u] > sv;
      int lo = 0, hi = K;                                           // list entries above sv (the list is descending)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L[mid] > sv) lo = mid + 1; else hi = mid;
      }
      sp = lo + cnt;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPer; ++t)
      if (lp[t] < K) L[lp[t]] = lv[t];
    if (sp < K) L[sp] = sv;
    if (lane == 0) nsurv[qq] = 0;
    __syncthreads();
  }
}

// ---- the pair kernels' grid ------------------------------------------------------------------------------------------
// Block x: 32 queries, one per lane of a half wave (the halves h are the MFMA's two k steps; on the VALU path lanes 32..63
// repeat lanes 0..31).  Block y: a split, candidates [c_begin, c_end), every wave scoring ONE candidate at a time.
struct Place {
  int tid, wave, lane, col, h, split;
  int64_t q0, q, c_begin, c_end;
  bool q_ok;                            // the lane's query exists
};

__device__ __forceinline__ Place place(int64_t U, int64_t I, int64_t chunk) {
  Place at;
  at.tid = threadIdx.x; at.wave = at.tid >> 6; at.lane = at.tid & 63; at.col = at.lane & 31; at.h = at.lane >> 5;
  at.split = blockIdx.y;
  at.q0 = static_cast<int64_t>(blockIdx.x) * kQB;
  at.q = at.q0 + at.col;
  at.c_begin = at.split * chunk;
  at.c_end = at.c_begin + chunk < I ? at.c_begin + chunk : I;
  at.q_ok = at.q < U;
  return at;
}

// is candidate c on query q's exclusion list (excl [U][words] bits, or NULL)?
__device__ __forceinline__ bool excluded(const uint32_t* __restrict__ excl, int words, int64_t q, int64_t c) {
  return excl && ((excl[q * words + (c >> 5)] >> (c & 31)) & 1u);
}

// ---- the scorers: "the score of candidate c for this lane's query" ---------------------------------------------------
// One member of the table, on the VALU path: its arguments, the lane's w_q and its column of sqT fetched once.
struct SoloScorer {
  const ScoreArgs& p;
  const int64_t qcol;
  const float wq;
  const float* __restrict__ const sq;
  __device__ __forceinline__ SoloScorer(const ScoreArgs& p, const Place& at)
      : p(p), qcol(at.q), wq((p.w_q && at.q_ok) ? p.w_q[at.q] : 0.f), sq(p.sqT ? p.sqT + at.q : nullptr) {}
  // c: the wave's one candidate, or a candidate per lane (a target: a_c, s_c and w_c become per-lane loads)
  __device__ __forceinline__ float operator()(int64_t c, int h) const { return pair_score<false, 1, 1>(p, c, qcol, h, wq, sq); }
};

// A member of a group as the kernels see it, in device memory (workspace): its scoring arguments (s.l points at l below,
// s.aqT / s.sqT at the member's transposes in the workspace) and the caller's query-side tensors the transposes are made from.
struct GroupMember {
  ScoreArgs s;
  const float* a_q;                     // [U][H1]
  const float* s_q;                     // [U][E]
  Layer l[kMaxLayers];
};

// A member's scoring arguments from the table, word by word and every word made wave-uniform (readfirstlane): the loop
// bounds, the activation and the pointers stay in scalar registers, as pair_score_topk_k holds its kernel arguments.  A
// pointer is put together from its two words AS A GLOBAL ONE: a pointer read from memory is a generic pointer to the
// compiler, and it treats what a generic (flat) load returns as divergent — the layer table's widths, every loop bound.
struct MemberWords {
  const uint32_t* __restrict__ w;
  __device__ __forceinline__ uint32_t u32(size_t off) const { return __builtin_amdgcn_readfirstlane(w[off / 4]); }
  template <class T>
  __device__ __forceinline__ const T* ptr(size_t off) const {
    const uint64_t v = u32(off) | (static_cast<uint64_t>(u32(off + 4)) << 32);
    return (const T*)(const __attribute__((address_space(1))) T*)v;
  }
};

__device__ __forceinline__ ScoreArgs load_member(const GroupMember* __restrict__ gm) {
  const MemberWords m{reinterpret_cast<const uint32_t*>(&gm->s)};
  ScoreArgs p;
  p.aqT = m.ptr<float>(offsetof(ScoreArgs, aqT)); p.a_c = m.ptr<float>(offsetof(ScoreArgs, a_c));
  p.sqT = m.ptr<float>(offsetof(ScoreArgs, sqT)); p.s_c = m.ptr<float>(offsetof(ScoreArgs, s_c));
  p.w_q = m.ptr<float>(offsetof(ScoreArgs, w_q)); p.w_c = m.ptr<float>(offsetof(ScoreArgs, w_c));
  p.dense = m.ptr<float>(offsetof(ScoreArgs, dense)); p.l = m.ptr<Layer>(offsetof(ScoreArgs, l));
  p.Upad = static_cast<int32_t>(m.u32(offsetof(ScoreArgs, Upad))); p.H1 = static_cast<int32_t>(m.u32(offsetof(ScoreArgs, H1)));
  p.E = static_cast<int32_t>(m.u32(offsetof(ScoreArgs, E))); p.act = static_cast<int32_t>(m.u32(offsetof(ScoreArgs, act)));
  p.n_layers = static_cast<int32_t>(m.u32(offsetof(ScoreArgs, n_layers)));
  return p;
}

// The members' mean logit
//   z = (((z_0 + z_1) + z_2) + ... + z_{M-1}) / (float)M    ascending member order, one rounding per operation
// (mi_predict_group's definition), z_m = member m's own score on the VALU path (the entries refuse a member whose own call
// would take the MFMA path): a group of one scores as the solo kernel does, bit for bit.  The member table is read from
// device memory with wave-uniform addresses; nothing of it lives in LDS.  member_scores [M][U][I] or NULL takes every z_m.
struct MeanScorer {
  const GroupMember* __restrict__ tab;
  int M;
  const Place& at;
  float* __restrict__ member_scores;
  int64_t U, I;
  __device__ __forceinline__ float operator()(int64_t c, int h) const {
    float acc = 0.f;
    for (int m = 0; m < M; ++m) {
      const ScoreArgs p = load_member(tab + m);
      const float z = SoloScorer(p, at)(c, h);
      if (member_scores && h == 0 && at.q_ok) member_scores[(static_cast<int64_t>(m) * U + at.q) * I + c] = z;
      acc = m == 0 ? z : acc + z;
    }
    return acc / static_cast<float>(M);
  }
};

// ---- keep the best K ---------------------------------------------------------------------------------------------------
// Every query's sorted list and its survivor slots live in LDS; the split's lists go to part [U][splits][K].  The loop is
// pair_score_topk_k's, over a scorer.
template <class Scorer>
__device__ __forceinline__ void select_topk(const Scorer& score, const SelectArgs& a, const Place& at) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int K = a.K, tid = at.tid, col = at.col;
  uint64_t* list = reinterpret_cast<uint64_t*>(lds);             // [kQB][K], descending, 0 = empty
  uint64_t* surv = list + kQB * K;                                // [kQB][kSurv]
  int* nsurv = reinterpret_cast<int*>(surv + kQB * kSurv);        // [kQB]
  for (int i = tid; i < kQB * K; i += kThreads) list[i] = 0;
  if (tid < kQB) nsurv[tid] = 0;
  __syncthreads();
  for (int64_t base = at.c_begin; base < at.c_end; base += kWaves) {
    const int64_t c = base + at.wave;
    if (c < at.c_end) {                                           // (wave-uniform)
      const float s = score(c, at.h);
      if (at.h == 0 && at.q_ok) {
        if (a.scores) a.scores[at.q * a.I + c] = s;
        if (!excluded(a.excl, a.words, at.q, c)) {
          const uint64_t key = rank_key(s, static_cast<uint32_t>(c));
          if (key > list[col * K + K - 1]) {
            const int slot = atomicAdd(&nsurv[col], 1);
            surv[col * kSurv + slot] = key;
          }
        }
      }
    }
    // (__syncthreads_or evaluates its argument BEFORE its barrier: the counts are read only after every wave's appends of
    // this round are in — a stale count could skip a merge the next round's appends need, and overflow the slots)
    __syncthreads();
    if (__syncthreads_or(tid < kQB && nsurv[tid] > kSurv - kWaves)) merge_survivors(list, surv, nsurv, K, at.wave, at.lane);
  }
  __syncthreads();
  if (__syncthreads_or(tid < kQB && nsurv[tid] > 0)) merge_survivors(list, surv, nsurv, K, at.wave, at.lane);
  for (int i = tid; i < kQB * K; i += kThreads) {
    const int qq = i / K;
    if (at.q0 + qq < a.U) a.part[((at.q0 + qq) * a.splits + at.split) * K + (i - qq * K)] = list[i];
  }
}

// ---- count the keys above named targets --------------------------------------------------------------------------------
// A workgroup first scores its 32 queries' targets (the candidate differs per lane) and keeps their keys in LDS, then runs
// the candidate loop over its chunk and counts, per target of the query, whether the candidate's key is larger.  Keys of one
// query are distinct and a target's own pair scores to the target's own bits, so the count never includes the target.
//   tkey [Tq][kQB]          the targets' keys; ~0 (above every key) where the target has no rank
//   cnt  [kWaves][Tq][kQB]  one set of counters per wave: lane (col, h) alone adds to targets j = h, h + 2, ... of query
//                           col in its wave's set, so the adds are plain LDS read-modify-writes — no atomics, no barrier in
//                           the candidate loop, and the idle half of the VALU path's wave does half of the compares
// The split's counts go plainly to part [m][splits][U][Tq] (-1: no rank; m: the scorer's place among the members on the
// grid, 0 where they are a loop in the scorer); rank_sum_k adds the splits.  Integers only: the result depends neither on
// the split count nor on timing, and no workgroup waits for another.
constexpr uint64_t kNoRank = ~static_cast<uint64_t>(0);

template <class Scorer>
__device__ __forceinline__ void count_ranks(const Scorer& score, const RanksArgs& a, const Place& at, int m) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int Tq = a.Tq, tid = at.tid, col = at.col;
  uint64_t* tkey = reinterpret_cast<uint64_t*>(lds);             // [Tq][kQB]
  int* cnt = reinterpret_cast<int*>(tkey + Tq * kQB);             // [kWaves][Tq][kQB]
  for (int i = tid; i < kWaves * Tq * kQB; i += kThreads) cnt[i] = 0;
  // the targets: thread (col, j0 = tid / 32) takes targets j0, j0 + 8, ... of query col.  Every lane scores one (candidate 0
  // where it has none, the result dropped — never stored, and q_ok guards w_q): a mean scorer's wave-uniform reads of the
  // member table never run under an empty exec mask.
  for (int j = tid >> 5; j < Tq; j += kThreads / kQB) {
    int64_t t = at.q_ok ? a.targets[at.q * Tq + j] : -1;
    const bool has = t >= 0 && t < a.I && !excluded(a.excl, a.words, at.q, t);
    if (!has) t = 0;
    float s = score(t, 0);
    uint64_t key = rank_key(s, static_cast<uint32_t>(t));
    if (!has) {
      s = __uint_as_float(0x7fc00000u);
      key = kNoRank;
    }
    if (at.q_ok && at.split == 0 && a.target_scores) a.target_scores[(static_cast<int64_t>(m) * a.U + at.q) * Tq + j] = s;
    tkey[j * kQB + col] = key;
  }
  __syncthreads();
  int* mine = cnt + at.wave * Tq * kQB + col;
  for (int64_t c = at.c_begin + at.wave; c < at.c_end; c += kWaves) {     // (c is wave-uniform)
    const float s = score(c, at.h);
    if (at.q_ok && !excluded(a.excl, a.words, at.q, c)) {
      const uint64_t key = rank_key(s, static_cast<uint32_t>(c));
      for (int j = at.h; j < Tq; j += 2) mine[j * kQB] += key > tkey[j * kQB + col];
    }
  }
  __syncthreads();
  // thread i = (query i / Tq, target i % Tq): the block's rows of part are contiguous
  int32_t* out = a.part + ((static_cast<int64_t>(m) * a.splits + at.split) * a.U + at.q0) * Tq;
  const int64_t rows = a.U - at.q0 < kQB ? a.U - at.q0 : kQB;
  for (int i = tid; i < rows * Tq; i += kThreads) {
    const int qq = i / Tq, j = i - qq * Tq, slot = j * kQB + qq;
    int n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += cnt[w * Tq * kQB + slot];
    out[i] = tkey[slot] == kNoRank ? -1 : n;
  }
}

// ---- the kernels -----------------------------------------------------------------------------------------------------
// pair_score_topk_k keeps its own statement of the selection, over its own by-value argument struct (every word wave-uniform,
// in scalar registers; the scoring functions read the fields they name from it as they do from a ScoreArgs).  The MFMA
// instances sit at the register ceiling and the kernel is the most used of the four: built as select_topk over a scorer it ran
// 0.3 to 1.7 % slower in every variant measured (profiles/rank_one_body.md), so the loop below and select_topk's are kept equal
// by hand.  A change to the survivor protocol is made in both.
struct PairArgs {
  const float *aqT, *a_c, *sqT, *s_c, *w_q, *w_c, *dense;
  const uint32_t* excl;
  float* scores;
  uint64_t* part;
  int64_t U, I, chunk;
  const Layer* l;
  int32_t Upad, H1, E, K, splits, words, act, n_layers;
};

template <bool MFMA, int NP, int NQ>
__global__ __launch_bounds__(kThreads) void pair_score_topk_k(const PairArgs p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int K = p.K;
  uint64_t* list = reinterpret_cast<uint64_t*>(lds);             // [kQB][K], descending, 0 = empty
  uint64_t* surv = list + kQB * K;                                // [kQB][kSurv]
  int* nsurv = reinterpret_cast<int*>(surv + kQB * kSurv);        // [kQB]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQB;
  const int split = blockIdx.y;
  const int64_t c_begin = split * p.chunk;
  const int64_t c_end = c_begin + p.chunk < p.I ? c_begin + p.chunk : p.I;
  for (int i = tid; i < kQB * K; i += kThreads) list[i] = 0;
  if (tid < kQB) nsurv[tid] = 0;
  __syncthreads();
  const int64_t q = q0 + col;
  const bool q_ok = q < p.U;
  const float wq = (p.w_q && q_ok) ? p.w_q[q] : 0.f;
  const float* __restrict__ sq = p.sqT ? p.sqT + q0 + col : nullptr;
  for (int64_t base = c_begin; base < c_end; base += kWaves) {
    const int64_t c = base + wave;
    if (c < c_end) {                                              // (wave-uniform)
      const float s = pair_score<MFMA, NP, NQ>(p, c, q0 + col, h, wq, sq);
      if (h == 0 && q_ok) {
        if (p.scores) p.scores[q * p.I + c] = s;
        const bool excluded = p.excl && ((p.excl[q * p.words + (c >> 5)] >> (c & 31)) & 1u);
        if (!excluded) {
          const uint64_t key = rank_key(s, static_cast<uint32_t>(c));
          if (key > list[col * K + K - 1]) {
            const int slot = atomicAdd(&nsurv[col], 1);
            surv[col * kSurv + slot] = key;
          }
        }
      }
    }
    __syncthreads();                                              // (the protocol: select_topk)
    if (__syncthreads_or(tid < kQB && nsurv[tid] > kSurv - kWaves)) merge_survivors(list, surv, nsurv, K, wave, lane);
  }
  __syncthreads();
  if (__syncthreads_or(tid < kQB && nsurv[tid] > 0)) merge_survivors(list, surv, nsurv, K, wave, lane);
  for (int i = tid; i < kQB * K; i += kThreads) {
    const int qq = i / K;
    if (q0 + qq < p.U) p.part[((q0 + qq) * p.splits + split) * K + (i - qq * K)] = list[i];
  }
}

// The kernels that read the member table take their body's arguments one by one, as __restrict__ pointers, and fill its struct
// themselves.  By value a SelectArgs leaves 36 unused bytes of private memory per lane reserved, and a RanksArgs loses the promise
// that the kernel's stores leave a member's weights alone: they become vector loads, the rank entries 13-17 % slower (measured).
__global__ __launch_bounds__(kThreads) void pair_score_topk_group_k(
    const GroupMember* __restrict__ tab, int M, const uint32_t* __restrict__ excl, float* __restrict__ scores,
    float* __restrict__ member_scores, uint64_t* __restrict__ part, int64_t U, int64_t I, int64_t chunk, int K, int splits, int words) {
  const SelectArgs a{excl, scores, part, U, I, chunk, K, splits, words};
  const Place at = place(a.U, a.I, a.chunk);
  select_topk(MeanScorer{tab, M, at, member_scores, a.U, a.I}, a, at);
}

// grid z: the members, every one for itself
__global__ __launch_bounds__(kThreads) void pair_target_ranks_k(
    const GroupMember* __restrict__ tab, const uint32_t* __restrict__ excl, const int32_t* __restrict__ targets,
    float* __restrict__ target_scores, int32_t* __restrict__ part, int64_t U, int64_t I, int64_t chunk, int Tq, int splits, int words) {
  const RanksArgs a{excl, targets, target_scores, part, U, I, chunk, Tq, splits, words};
  const Place at = place(a.U, a.I, a.chunk);
  const ScoreArgs p = load_member(tab + blockIdx.z);
  count_ranks(SoloScorer(p, at), a, at, blockIdx.z);
}

__global__ __launch_bounds__(kThreads) void pair_target_ranks_mean_k(
    const GroupMember* __restrict__ tab, int M, const uint32_t* __restrict__ excl, const int32_t* __restrict__ targets,
    float* __restrict__ target_scores, int32_t* __restrict__ part, int64_t U, int64_t I, int64_t chunk, int Tq, int splits, int words) {
  const RanksArgs a{excl, targets, target_scores, part, U, I, chunk, Tq, splits, words};
  const Place at = place(a.U, a.I, a.chunk);
  count_ranks(MeanScorer{tab, M, at, nullptr, a.U, a.I}, a, at, 0);
}

// ranks[m][e] = the sum over the splits of part[m][split][e], -1 where the target has no rank; n = U * Tq, grid (blocks, M)
__global__ __launch_bounds__(256) void rank_sum_k(const int32_t* __restrict__ part, int splits, int64_t n,
                                                  int32_t* __restrict__ ranks) {
  const int64_t m = blockIdx.y;
  const int32_t* __restrict__ src = part + m * splits * n;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * 256) {
    int32_t r = src[e];
    if (r >= 0)
      for (int s = 1; s < splits; ++s) r += src[s * n + e];
    ranks[m * n + e] = r;
  }
}

// one workgroup per query: entry (s, j) of the partial lists has rank j + (entries of the other lists above it)
__global__ __launch_bounds__(256) void topk_merge_k(const uint64_t* __restrict__ part, int splits, int K,
                                                    float* __restrict__ top_score, int32_t* __restrict__ top_idx) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* m = reinterpret_cast<uint64_t*>(lds);
  __shared__ int total;
  const int64_t u = blockIdx.x;
  const int n = splits * K;
  const uint64_t* src = part + u * n;
  for (int i = threadIdx.x; i < n; i += 256) m[i] = src[i];
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const uint64_t x = m[i];
    if (x == 0) continue;
    ++mine;
    const int s = i / K, j = i - s * K;
    int r = j;
    for (int s2 = 0; s2 < splits && r < K; ++s2) {
      if (s2 == s) continue;
      const uint64_t* L = m + s2 * K;
      int lo = 0, hi = K;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L[mid] > x) lo = mid + 1; else hi = mid;
      }
      r += lo;
    }
    if (r < K) {
      top_score[u * K + r] = key_score(x);
      top_idx[u * K + r] = key_index(x);
    }
  }
  atomicAdd(&total, mine);
  __syncthreads();
  for (int r = total + threadIdx.x; r < K; r += 256) {
    top_score[u * K + r] = -__builtin_huge_valf();
    top_idx[u * K + r] = -1;
  }
}

// dst[k][q] = src[q][k] for q < U, 0 for U <= q < Upad
__global__ __launch_bounds__(256) void transpose_pad_k(const float* __restrict__ src, int64_t U, int W, int Upad,
                                                       float* __restrict__ dst) {
  const int64_t n = static_cast<int64_t>(W) * Upad;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t k = i / Upad, q = i - k * Upad;
    dst[i] = q < U ? src[q * W + k] : 0.f;
  }
}

__global__ __launch_bounds__(64) void layer_table_k(const LayerTable t, int n, Layer* __restrict__ out) {
#pragma unroll
  for (int i = 0; i < kMaxLayers; ++i)
    if (i < n && threadIdx.x == 0) out[i] = t.l[i];
}

__global__ __launch_bounds__(256) void zero_u32_k(uint32_t* __restrict__ p, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) p[i] = 0;
}

// one workgroup per query: its excluded candidates as bits of [U][words] (entries outside [0, I) are ignored)
__global__ __launch_bounds__(256) void excl_mask_k(const int64_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                   int64_t I, int words, uint32_t* __restrict__ mask) {
  const int64_t u = blockIdx.x;
  for (int64_t e = off[u] + threadIdx.x; e < off[u + 1]; e += 256) {
    const int32_t c = idx[e];
    if (c >= 0 && c < I) atomicOr(&mask[u * words + (c >> 5)], 1u << (c & 31));
  }
}

// The member table reaches the workspace through the kernel arguments, kTabChunk members a launch (compile-time
// indices: see ScoreArgs::l) — no host-to-device copy, so the call neither synchronises nor needs pinned memory.
constexpr int kTabChunk = 8;
struct MemberChunk {
  GroupMember m[kTabChunk];
};
static_assert(sizeof(MemberChunk) <= 3072, "the member chunk travels in the kernel arguments");

__global__ __launch_bounds__(64) void member_table_k(const MemberChunk t, int n, GroupMember* __restrict__ out) {
#pragma unroll
  for (int i = 0; i < kTabChunk; ++i)
    if (i < n && threadIdx.x == 0) out[i] = t.m[i];
}

// transpose_pad_k for every member in one launch: grid (blocks, M, 2), z = 0: a_q -> aqT, z = 1: s_q -> sqT
__global__ __launch_bounds__(256) void transpose_pad_group_k(const GroupMember* __restrict__ tab, int64_t U) {
  const GroupMember& gm = tab[blockIdx.y];
  const bool a = blockIdx.z == 0;
  const float* __restrict__ src = a ? gm.a_q : gm.s_q;
  float* __restrict__ dst = const_cast<float*>(a ? gm.s.aqT : gm.s.sqT);
  if (!dst) return;
  const int W = a ? gm.s.H1 : gm.s.E, Upad = gm.s.Upad;
  const int64_t n = static_cast<int64_t>(W) * Upad;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t k = i / Upad, q = i - k * Upad;
    dst[i] = q < U ? src[q * W + k] : 0.f;
  }
}

inline size_t align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }

// workgroups of 256 threads for the n elements of a grid-stride kernel (at most 2048)
inline unsigned grid_blocks(int64_t n) { const int64_t b = mi::ceil_div(n, 256); return static_cast<unsigned>(b < 2048 ? b : 2048); }

// The pair kernels' grid for U queries and I candidates.  The split rule: about kTargetBlocks workgroups over query blocks x
// the members on the grid, at least 64 candidates per split, and at most cap splits (what the final merge's LDS holds).
struct Split {
  int64_t Upad, qblocks, chunk;
  int32_t splits, words;
};

Split make_split(int64_t U, int64_t I, int64_t grid_members, int64_t cap = INT64_MAX) {
  Split sp;
  sp.qblocks = mi::ceil_div(U, kQB);
  sp.Upad = sp.qblocks * kQB;
  int64_t s = mi::ceil_div(kTargetBlocks, sp.qblocks * grid_members);
  const int64_t s_min_chunk = mi::ceil_div(I, 64);
  if (s > cap) s = cap;
  if (s > s_min_chunk) s = s_min_chunk;
  if (s < 1) s = 1;
  sp.chunk = mi::ceil_div(I, s);
  sp.splits = static_cast<int32_t>(mi::ceil_div(I, sp.chunk));
  sp.words = static_cast<int32_t>(mi::ceil_div(I, 32));
  return sp;
}

struct Plan {
  Split sp;
  size_t off_layers, off_aq, off_sq, off_mask, off_part, total;
};

Plan make_plan(int64_t U, int64_t I, int32_t k, int32_t H1, int32_t E) {
  Plan pl;
  pl.sp = make_split(U, I, 1, kMergeLds / (8 * static_cast<int64_t>(k)));
  size_t o = 0;
  pl.off_layers = o; o += align256(sizeof(Layer) * kMaxLayers);
  pl.off_aq = o; o += align256(sizeof(float) * static_cast<size_t>(H1) * pl.sp.Upad);
  pl.off_sq = o; o += align256(sizeof(float) * static_cast<size_t>(E) * pl.sp.Upad);
  pl.off_mask = o; o += align256(sizeof(uint32_t) * static_cast<size_t>(U) * pl.sp.words);
  pl.off_part = o; o += align256(sizeof(uint64_t) * static_cast<size_t>(U) * pl.sp.splits * k);
  pl.total = o;
  return pl;
}

bool sizes_ok(int64_t U, int64_t I, int32_t k, int32_t H1, int32_t E) {
  return U >= 1 && I >= 1 && I <= INT32_MAX && k >= 1 && k <= kMaxK && H1 >= 0 && H1 <= kMaxH1 && E >= 0 && E <= 256 &&
         mi::ceil_div(U, kQB) <= INT32_MAX;
}

// The checks of mi_pair_topk in their order, shared with mi_pair_topk_group (which prefixes "member i:" and has checked the
// per-call arguments — outputs, excl_paired — itself): fills the layer table and maxw, the largest hidden width after layer 1.
int32_t check_model(int64_t U, int64_t I, int32_t k, const float* a_q, const float* s_q, const float* a_c, const float* s_c,
                    int32_t H1, int32_t E, const float* dense, const int64_t* layer_off, const int32_t* widths,
                    int32_t n_layers, int32_t activation, bool outputs, bool excl_paired, LayerTable& lt, int& maxw) {
  MI_REQUIRE(sizes_ok(U, I, k, H1, E), "pair_topk: U=%lld I=%lld k=%d H1=%d E=%d out of range (U, I >= 1, 1 <= k <= %d, "
             "H1 <= %d, E <= 256)", (long long)U, (long long)I, k, H1, E, kMaxK, kMaxH1);
  MI_REQUIRE(outputs, "pair_topk: top_score / top_idx");
  MI_REQUIRE(activation >= 0 && activation <= 3, "pair_topk: activation %d", activation);
  MI_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "pair_topk: %d layers after layer 1 (at most %d)", n_layers, kMaxLayers);
  MI_REQUIRE(H1 == 0 || (a_q && a_c && dense && (n_layers == 0 || (layer_off && widths))),
             "pair_topk: a_q / a_c / dense / layer_off / widths");
  MI_REQUIRE(H1 > 0 || n_layers == 0, "pair_topk: layers without a layer 1");
  MI_REQUIRE(H1 == 0 || n_layers > 0 || H1 == 1, "pair_topk: without hidden layers layer 1 is the logits layer (H1 = 1)");
  MI_REQUIRE(E == 0 || (s_q && s_c), "pair_topk: s_q / s_c");
  MI_REQUIRE(excl_paired, "pair_topk: excl_off and excl_idx go together");
  int wp = 0, wq = 0;                            // widths of layers 2..L-1 at even / odd positions
  maxw = 0;
  for (int i = 0; i < n_layers; ++i) {
    const int fi = widths[i], fo = widths[i + 1];
    MI_REQUIRE(fi >= 1 && fo >= 1, "pair_topk: width %d -> %d", fi, fo);
    MI_REQUIRE(i > 0 || fi == H1, "pair_topk: widths[0]=%d != H1=%d", fi, H1);
    MI_REQUIRE(i + 1 < n_layers || fo == 1, "pair_topk: the last layer has %d outputs (1 expected)", fo);
    MI_REQUIRE(layer_off[2 * i] >= 0 && layer_off[2 * i + 1] >= 0, "pair_topk: layer offsets");
    if (i + 1 < n_layers) {
      if (fo > maxw) maxw = fo;
      int& w = (i & 1) ? wq : wp;
      if (fo > w) w = fo;
    }
    lt.l[i] = Layer{layer_off[2 * i], layer_off[2 * i + 1], fi, fo};
  }
  MI_REQUIRE(wp <= kMaxRegWidth && wq <= kMaxRegWidth / 2, "pair_topk: hidden widths after layer 1: layers 2, 4, ... at most "
             "%d (here %d), layers 3, 5, ... at most %d (here %d)", kMaxRegWidth, wp, kMaxRegWidth / 2, wq);
  return MI_OK;
}

// does mi_pair_topk score this model on the MFMA (launch_pair<true, ...>)?  Otherwise the VALU loop (<false, 1, 1>)
inline bool takes_mfma(int n_layers, int maxw) { return n_layers >= 2 && maxw >= kValuW; }

using mi::unsupported;

// ---- a group of members (mi_pair_topk_group and the two rank entries) ------------------------------------------------
// What every group entry (`who`, for the texts) refuses first, in this order: the member count, then the table itself.
int32_t check_member_count(const char* who, const mi_rank_member_t* members, int32_t n_members) {
  MI_REQUIRE(n_members >= 1, "%s: %d members (at least 1)", who, n_members);
  if (n_members > MI_PAIR_TOPK_GROUP_MAX_MEMBERS)
    return unsupported("%s: %d members (at most %d in one launch)", who, n_members, MI_PAIR_TOPK_GROUP_MAX_MEMBERS);
  MI_REQUIRE(members, "%s: members", who);
  return MI_OK;
}

// Every member is checked before anything is launched: check_model (the entry has checked the per-call arguments), and the
// mean scorer's and the rank kernels' VALU scope.  kernel: the entry's word for what scores, "the group kernel" / "the kernel".
int32_t check_members(const char* who, const char* kernel, const mi_rank_member_t* members, int32_t n_members, int64_t U,
                      int64_t I, int32_t k) {
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_rank_member_t& m = members[i];
    LayerTable lt{};
    int maxw = 0;
    const int32_t rc = check_model(U, I, k, m.a_q, m.s_q, m.a_c, m.s_c, m.H1, m.E, m.dense, m.layer_off, m.widths, m.n_layers,
                                   m.activation, true, true, lt, maxw);
    if (rc != MI_OK) {
      mi::member_error(who, i);
      return rc;
    }
    if (takes_mfma(m.n_layers, maxw))
      return unsupported("%s: member %d: %d layers after layer 1 with a hidden width of %d: %s takes the VALU pair path only "
                         "(fewer than two layers after layer 1, or every hidden width after layer 1 below %d)", who, i,
                         m.n_layers, maxw, kernel, kValuW);
  }
  return MI_OK;
}

bool group_sizes_ok(const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t k) {
  if (!members || n < 1 || n > MI_PAIR_TOPK_GROUP_MAX_MEMBERS) return false;
  for (int32_t i = 0; i < n; ++i)
    if (!sizes_ok(U, I, k, members[i].H1, members[i].E)) return false;
  return true;
}

// The member table in the workspace, and behind it every member's transposes aqT [H1][Upad] and sqT [E][Upad].
struct TablePlace {
  size_t off_table, off_sides;
};

// The workspace keeps 352 bytes per member for the table — what a GroupMember took while it carried the selection's
// arguments as well — so every offset behind the table and every *_workspace_bytes answer is what callers have been given.
// (56 bytes a member lie unused: the slot can shrink to sizeof(GroupMember) with the next ABI version.)
constexpr size_t kTableSlot = 352;
static_assert(sizeof(GroupMember) <= kTableSlot, "the member table outgrew its place in the workspace");

inline size_t side_bytes(int64_t Upad, int32_t H1, int32_t E) {
  return align256(sizeof(float) * static_cast<size_t>(H1) * Upad) + align256(sizeof(float) * static_cast<size_t>(E) * Upad);
}

TablePlace place_table(const mi_rank_member_t* members, int32_t n, int64_t Upad, size_t& o) {
  TablePlace tp;
  tp.off_table = o; o += align256(kTableSlot * static_cast<size_t>(n));
  tp.off_sides = o;
  for (int32_t i = 0; i < n; ++i) o += side_bytes(Upad, members[i].H1, members[i].E);
  return tp;
}

// Writes the table, kTabChunk members a launch, and transposes every member's query side in one more launch.
GroupMember* write_member_table(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t Upad, char* ws,
                                const TablePlace& tp, hipStream_t st) {
  GroupMember* tab = reinterpret_cast<GroupMember*>(ws + tp.off_table);
  size_t side = tp.off_sides;
  int maxside = 0;
  MemberChunk ch{};
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_rank_member_t& m = members[i];
    GroupMember& gm = ch.m[i % kTabChunk];
    gm = GroupMember{};
    for (int j = 0; j < m.n_layers; ++j)
      gm.l[j] = Layer{m.layer_off[2 * j], m.layer_off[2 * j + 1], m.widths[j], m.widths[j + 1]};
    ScoreArgs& a = gm.s;
    a.aqT = m.H1 ? reinterpret_cast<float*>(ws + side) : nullptr;
    a.sqT = m.E ? reinterpret_cast<float*>(ws + side + align256(sizeof(float) * static_cast<size_t>(m.H1) * Upad)) : nullptr;
    side += side_bytes(Upad, m.H1, m.E);
    a.a_c = m.a_c; a.s_c = m.s_c; a.w_q = m.w_q; a.w_c = m.w_c; a.dense = m.dense;
    a.l = tab[i].l;                              // (the address of this member's layers in the workspace)
    a.Upad = static_cast<int32_t>(Upad); a.H1 = m.H1; a.E = m.E; a.act = m.activation; a.n_layers = m.n_layers;
    gm.a_q = m.a_q; gm.s_q = m.s_q;
    if (m.H1 > maxside) maxside = m.H1;
    if (m.E > maxside) maxside = m.E;
    if (i % kTabChunk == kTabChunk - 1 || i + 1 == n_members) {
      const int first = i - i % kTabChunk;
      member_table_k<<<dim3(1), dim3(64), 0, st>>>(ch, i - first + 1, tab + first);
    }
  }
  if (maxside)
    transpose_pad_group_k<<<dim3(grid_blocks(static_cast<int64_t>(maxside) * Upad), static_cast<unsigned>(n_members), 2), dim3(256), 0,
                            st>>>(tab, U);
  return tab;
}

// the exclusion lists as the bit mask the kernels test (nothing to do without lists: mask is NULL)
void prepare_mask(const int64_t* excl_off, const int32_t* excl_idx, int64_t U, int64_t I, int32_t words, uint32_t* mask,
                  hipStream_t st) {
  if (!mask) return;
  zero_u32_k<<<dim3(grid_blocks(U * words)), dim3(256), 0, st>>>(mask, U * words);
  excl_mask_k<<<dim3(static_cast<unsigned>(U)), dim3(256), 0, st>>>(excl_off, excl_idx, I, words, mask);
}

// ---- top-K: the selection's LDS, its launch for one model, and the final merge ---------------------------------------
inline size_t select_lds(int32_t k) { return sizeof(uint64_t) * kQB * (k + kSurv) + sizeof(int) * kQB; }

template <bool MFMA, int NP, int NQ>
int32_t launch_pair(const PairArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  const int32_t rl = mi::raise_lds(&pair_score_topk_k<MFMA, NP, NQ>, lds, "pair_topk");
  if (rl != MI_OK) return rl;
  pair_score_topk_k<MFMA, NP, NQ><<<grid, dim3(kThreads), lds, st>>>(a);
  return MI_OK;
}

int32_t finish_topk(const uint64_t* part, int64_t U, int32_t splits, int32_t k, float* top_score, int32_t* top_idx,
                    hipStream_t st) {
  topk_merge_k<<<dim3(static_cast<unsigned>(U)), dim3(256), sizeof(uint64_t) * splits * k, st>>>(part, splits, k, top_score,
                                                                                                 top_idx);
  MI_CHECK_LAUNCH("topk_merge_k");
  return MI_OK;
}

// What the group shares (query blocks, splits, exclusion mask, partial lists: make_plan with no per-model tensors) and
// where the member table and the members' transposes lie in the workspace.
constexpr size_t kMaxGroupLds = 160 * 1024;      // the dynamic LDS a launch can be raised to on gfx950

struct GroupPlan {
  Plan pl;
  TablePlace tp;
  size_t total;
};

GroupPlan make_group_plan(const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t k) {
  GroupPlan gp;
  gp.pl = make_plan(U, I, k, 0, 0);
  size_t o = gp.pl.total;
  gp.tp = place_table(members, n, gp.pl.sp.Upad, o);
  gp.total = o;
  return gp;
}

// ---- target ranks: every member for itself (the members on grid z), or under the members' mean (a loop in the scorer) --
struct RanksKind {
  bool mean;
  const char *who, *prepare, *kernel;           // the entry's name in its texts
};
constexpr RanksKind kEachMember{false, "pair_target_ranks", "pair_target_ranks (prepare)", "pair_target_ranks_k"};
constexpr RanksKind kMembersMean{true, "pair_target_ranks_mean", "pair_target_ranks_mean (prepare)", "pair_target_ranks_mean_k"};

// No selection lists: nothing but the split rule bounds the splits.  The workspace: the exclusion mask, the splits' partial
// counts (one set per member on the grid), the member table and the members' transposes.
struct RanksPlan {
  Split sp;
  int32_t grid_members;
  size_t off_mask, off_part, total;
  TablePlace tp;
};

RanksPlan make_ranks_plan(const RanksKind& kind, const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t Tq) {
  RanksPlan rp;
  rp.grid_members = kind.mean ? 1 : n;
  rp.sp = make_split(U, I, rp.grid_members);
  size_t o = 0;
  rp.off_mask = o; o += align256(sizeof(uint32_t) * static_cast<size_t>(U) * rp.sp.words);
  rp.off_part = o; o += align256(sizeof(int32_t) * static_cast<size_t>(rp.grid_members) * rp.sp.splits * U * Tq);
  rp.tp = place_table(members, n, rp.sp.Upad, o);
  rp.total = o;
  return rp;
}

size_t target_ranks_bytes(const RanksKind& kind, const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                          int32_t Tq) {
  if (Tq < 1 || Tq > MI_PAIR_RANKS_MAX_TARGETS || !group_sizes_ok(members, n_members, U, I, 1)) return 0;
  return make_ranks_plan(kind, members, n_members, U, I, Tq).total;
}

int32_t target_ranks_call(const RanksKind& kind, const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                          const int64_t* excl_off, const int32_t* excl_idx, const int32_t* targets, int32_t Tq, int32_t* ranks,
                          float* target_scores, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  const char* who = kind.who;
  int32_t rc = check_member_count(who, members, n_members);
  if (rc != MI_OK) return rc;
  MI_REQUIRE(Tq >= 1 && Tq <= MI_PAIR_RANKS_MAX_TARGETS, "%s: Tq=%d targets per query (1 to %d in one call)", who, Tq,
             MI_PAIR_RANKS_MAX_TARGETS);
  MI_REQUIRE(targets && ranks, "%s: targets / ranks", who);
  MI_REQUIRE(!excl_off == !excl_idx, "%s: excl_off and excl_idx go together", who);
  rc = check_members(who, "the kernel", members, n_members, U, I, 1);
  if (rc != MI_OK) return rc;
  const RanksPlan rp = make_ranks_plan(kind, members, n_members, U, I, Tq);
  const Split& sp = rp.sp;
  MI_REQUIRE(workspace && workspace_bytes >= rp.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, rp.total);
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + rp.off_mask) : nullptr;
  const GroupMember* tab = write_member_table(members, n_members, U, sp.Upad, ws, rp.tp, st);
  prepare_mask(excl_off, excl_idx, U, I, sp.words, mask, st);
  MI_CHECK_LAUNCH(kind.prepare);
  int32_t* part = reinterpret_cast<int32_t*>(ws + rp.off_part);
  const size_t lds = (sizeof(uint64_t) + sizeof(int) * kWaves) * kQB * static_cast<size_t>(Tq);      // at most 48 KB
  const dim3 grid(static_cast<unsigned>(sp.qblocks), static_cast<unsigned>(sp.splits), static_cast<unsigned>(rp.grid_members));
  if (kind.mean)
    pair_target_ranks_mean_k<<<grid, dim3(kThreads), lds, st>>>(tab, n_members, mask, targets, target_scores, part, U, I, sp.chunk,
                                                                Tq, sp.splits, sp.words);
  else
    pair_target_ranks_k<<<grid, dim3(kThreads), lds, st>>>(tab, mask, targets, target_scores, part, U, I, sp.chunk, Tq, sp.splits,
                                                           sp.words);
  MI_CHECK_LAUNCH(kind.kernel);
  const int64_t n = U * Tq;
  rank_sum_k<<<dim3(grid_blocks(n), static_cast<unsigned>(rp.grid_members)), dim3(256), 0, st>>>(part, sp.splits, n, ranks);
  MI_CHECK_LAUNCH("rank_sum_k");
  return MI_OK;
}

}  // namespace

extern "C" {

size_t mi_pair_topk_workspace_bytes(int64_t U, int64_t I, int32_t k, int32_t H1, int32_t E) {
  if (!sizes_ok(U, I, k, H1, E)) return 0;
  return make_plan(U, I, k, H1, E).total;
}

int32_t mi_pair_topk(const float* a_q, const float* s_q, const float* w_q, int64_t U,
                     const float* a_c, const float* s_c, const float* w_c, int64_t I, int32_t H1, int32_t E,
                     const float* dense, const int64_t* layer_off, const int32_t* widths, int32_t n_layers,
                     int32_t activation, const int64_t* excl_off, const int32_t* excl_idx, int32_t k,
                     float* top_score, int32_t* top_idx, float* scores, void* workspace, size_t workspace_bytes,
                     mi_stream_t stream) {
  LayerTable lt{};
  int maxw = 0;
  const int32_t rc = check_model(U, I, k, a_q, s_q, a_c, s_c, H1, E, dense, layer_off, widths, n_layers, activation,
                                 top_score && top_idx, !excl_off == !excl_idx, lt, maxw);
  if (rc != MI_OK) return rc;
  const Plan pl = make_plan(U, I, k, H1, E);
  const Split& sp = pl.sp;
  MI_REQUIRE(workspace && workspace_bytes >= pl.total, "pair_topk: workspace %zu < %zu bytes", workspace_bytes, pl.total);
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  float* aqT = H1 ? reinterpret_cast<float*>(ws + pl.off_aq) : nullptr;
  float* sqT = E ? reinterpret_cast<float*>(ws + pl.off_sq) : nullptr;
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + pl.off_mask) : nullptr;
  Layer* layers = reinterpret_cast<Layer*>(ws + pl.off_layers);
  if (n_layers) layer_table_k<<<dim3(1), dim3(64), 0, st>>>(lt, n_layers, layers);
  if (aqT) transpose_pad_k<<<dim3(grid_blocks(static_cast<int64_t>(H1) * sp.Upad)), dim3(256), 0, st>>>(a_q, U, H1, (int)sp.Upad, aqT);
  if (sqT) transpose_pad_k<<<dim3(grid_blocks(static_cast<int64_t>(E) * sp.Upad)), dim3(256), 0, st>>>(s_q, U, E, (int)sp.Upad, sqT);
  prepare_mask(excl_off, excl_idx, U, I, sp.words, mask, st);
  MI_CHECK_LAUNCH("pair_topk (prepare)");
  uint64_t* part = reinterpret_cast<uint64_t*>(ws + pl.off_part);
  const PairArgs a{aqT, a_c, sqT, s_c, w_q, w_c, dense, mask, scores, part, U, I, sp.chunk, layers,
                   static_cast<int32_t>(sp.Upad), H1, E, k, sp.splits, sp.words, activation, n_layers};
  const size_t lds = select_lds(k);
  const dim3 grid(static_cast<unsigned>(sp.qblocks), static_cast<unsigned>(sp.splits));
  int32_t rl;
  if (takes_mfma(n_layers, maxw)) {
    if (maxw <= 32) rl = launch_pair<true, 1, 1>(a, grid, lds, st);
    else if (maxw <= 64) rl = launch_pair<true, 2, 2>(a, grid, lds, st);
    else if (maxw <= 128) rl = launch_pair<true, 4, 4>(a, grid, lds, st);
    else rl = launch_pair<true, 8, 4>(a, grid, lds, st);
  } else {
    rl = launch_pair<false, 1, 1>(a, grid, lds, st);
  }
  if (rl != MI_OK) return rl;
  MI_CHECK_LAUNCH("pair_score_topk_k");
  return finish_topk(part, U, sp.splits, k, top_score, top_idx, st);
}

size_t mi_pair_topk_group_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, int32_t k) {
  if (!group_sizes_ok(members, n_members, U, I, k)) return 0;
  return make_group_plan(members, n_members, U, I, k).total;
}

int32_t mi_pair_topk_group(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                           const int32_t* excl_idx, int32_t k, float* top_score, int32_t* top_idx, float* scores,
                           float* member_scores, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  const char* who = "pair_topk_group";
  int32_t rc = check_member_count(who, members, n_members);
  if (rc != MI_OK) return rc;
  MI_REQUIRE(top_score && top_idx, "pair_topk_group: top_score / top_idx");
  MI_REQUIRE(!excl_off == !excl_idx, "pair_topk_group: excl_off and excl_idx go together");
  rc = check_members(who, "the group kernel", members, n_members, U, I, k);
  if (rc != MI_OK) return rc;
  const GroupPlan gp = make_group_plan(members, n_members, U, I, k);
  const Split& sp = gp.pl.sp;
  MI_REQUIRE(workspace && workspace_bytes >= gp.total, "pair_topk_group: workspace %zu < %zu bytes", workspace_bytes, gp.total);
  const size_t lds = select_lds(k);                                               // (the lists; no member data lives in LDS)
  if (lds > kMaxGroupLds) return unsupported("pair_topk_group: %zu bytes of LDS for k=%d (at most %zu)", lds, k, kMaxGroupLds);
  const int32_t rl = mi::raise_lds(&pair_score_topk_group_k, lds, who);
  if (rl != MI_OK) return rl;
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + gp.pl.off_mask) : nullptr;
  const GroupMember* tab = write_member_table(members, n_members, U, sp.Upad, ws, gp.tp, st);
  prepare_mask(excl_off, excl_idx, U, I, sp.words, mask, st);
  MI_CHECK_LAUNCH("pair_topk_group (prepare)");
  uint64_t* part = reinterpret_cast<uint64_t*>(ws + gp.pl.off_part);
  pair_score_topk_group_k<<<dim3(static_cast<unsigned>(sp.qblocks), static_cast<unsigned>(sp.splits)), dim3(kThreads), lds, st>>>(
      tab, n_members, mask, scores, member_scores, part, U, I, sp.chunk, k, sp.splits, sp.words);
  MI_CHECK_LAUNCH("pair_score_topk_group_k");
  return finish_topk(part, U, sp.splits, k, top_score, top_idx, st);
}

size_t mi_pair_target_ranks_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, int32_t Tq) {
  return target_ranks_bytes(kEachMember, members, n_members, U, I, Tq);
}

int32_t mi_pair_target_ranks(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                             const int32_t* excl_idx, const int32_t* targets, int32_t Tq, int32_t* ranks, float* target_scores,
                             void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return target_ranks_call(kEachMember, members, n_members, U, I, excl_off, excl_idx, targets, Tq, ranks, target_scores,
                           workspace, workspace_bytes, stream);
}

size_t mi_pair_target_ranks_mean_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                                                 int32_t Tq) {
  return target_ranks_bytes(kMembersMean, members, n_members, U, I, Tq);
}

int32_t mi_pair_target_ranks_mean(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                                  const int64_t* excl_off, const int32_t* excl_idx, const int32_t* targets, int32_t Tq,
                                  int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes,
                                  mi_stream_t stream) {
  return target_ranks_call(kMembersMean, members, n_members, U, I, excl_off, excl_idx, targets, Tq, ranks, target_scores,
                           workspace, workspace_bytes, stream);
}

}  // extern "C"
