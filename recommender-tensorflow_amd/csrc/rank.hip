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
//   pair_target_ranks_k  grid (query blocks) x (candidate splits) x (members): the exact rank of named target candidates
//                      by each member's own score — the targets' keys in LDS, the candidate loop above, integer counters;
//                      rank_sum_k adds the splits' counts (mi_pair_target_ranks).
//   pair_target_ranks_mean_k  grid (query blocks) x (candidate splits): the same count under the members' MEAN score — the
//                      members are a loop in the lane, as in pair_score_topk_group_k (mi_pair_target_ranks_mean).
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

struct PairArgs {
  const float* aqT;                     // [H1][Upad] (workspace: a_q transposed, zero columns past U)
  const float* a_c;                     // [I][H1]
  const float* sqT;                     // [E][Upad]
  const float* s_c;                     // [I][E]
  const float* w_q;                     // [U] or NULL
  const float* w_c;                     // [I] or NULL
  const float* dense;
  const uint32_t* excl;                 // [U][words] bitmask or NULL
  float* scores;                        // [U][I] or NULL
  uint64_t* part;                       // [U][splits][K]
  int64_t U, I, chunk;
  const Layer* l;                       // [n_layers] (workspace; a table in the kernel arguments would be copied to
                                        // scratch by the runtime-indexed reads)
  int32_t Upad, H1, E, K, splits, words, act, n_layers;
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
template <int NB>
__device__ __forceinline__ void layer2_mfma(const PairArgs& p, const float* __restrict__ ac, int64_t qcol, int h,
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
template <int NI, int NO>
__device__ __forceinline__ void layer_mfma(const PairArgs& p, const Layer L, const f32x16 (&x)[NI], f32x16 (&y)[NO],
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

template <int NB>
__device__ __forceinline__ float logits_mfma(const PairArgs& p, const Layer L, const f32x16 (&x)[NB], int h) {
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
template <int NP, int NQ>
__device__ __forceinline__ float dnn_mfma(const PairArgs& p, const float* __restrict__ ac, int64_t qcol, int h) {
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

__device__ __forceinline__ void layer_valu(const PairArgs& p, const Layer L, const float (&x)[kValuW], float (&y)[kValuW]) {
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

__device__ __forceinline__ float logits_valu(const PairArgs& p, const Layer L, const float (&x)[kValuW]) {
  const float* __restrict__ W = p.dense + L.w_off;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kValuW; ++k)
    if (k < L.fan_in) s = fmaf(x[k], W[k], s);
  return s + p.dense[L.b_off];
}

__device__ __forceinline__ float dnn_valu(const PairArgs& p, const float* __restrict__ ac, int64_t qcol) {
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
// (NULL without the FM term).  Both pair kernels call this: a group member's score is its own kernel's, bit for bit
// (every product is an explicit fmaf and no multiply feeds an add, so there is nothing for the compiler to contract).
template <bool MFMA, int NP, int NQ>
__device__ __forceinline__ float pair_score(const PairArgs& p, int64_t c, int64_t qcol, int h, float wq,
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
    // (__syncthreads_or evaluates its argument BEFORE its barrier: the counts are read only after every wave's appends of
    // this round are in — a stale count could skip a merge the next round's appends need, and overflow the slots)
    __syncthreads();
    if (__syncthreads_or(tid < kQB && nsurv[tid] > kSurv - kWaves)) merge_survivors(list, surv, nsurv, K, wave, lane);
  }
  __syncthreads();
  if (__syncthreads_or(tid < kQB && nsurv[tid] > 0)) merge_survivors(list, surv, nsurv, K, wave, lane);
  for (int i = tid; i < kQB * K; i += kThreads) {
    const int qq = i / K;
    if (q0 + qq < p.U) p.part[((q0 + qq) * p.splits + split) * K + (i - qq * K)] = list[i];
  }
}

// ---- an ensemble: M models, one selection (mi_pair_topk_group) ------------------------------------------------------
// A member of the group as the kernels see it, in device memory (workspace): the scoring arguments of its own
// pair_score_topk_k (p.l points at l below, p.aqT / p.sqT at the member's transposes in the workspace) and the caller's
// query-side tensors the transposes are made from.
struct GroupMember {
  PairArgs p;
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

__device__ __forceinline__ PairArgs load_member(const GroupMember* __restrict__ gm) {
  const MemberWords m{reinterpret_cast<const uint32_t*>(&gm->p)};
  PairArgs p{};                                  // (the fields pair_score reads; the selection's are the group's)
  p.aqT = m.ptr<float>(offsetof(PairArgs, aqT)); p.a_c = m.ptr<float>(offsetof(PairArgs, a_c));
  p.sqT = m.ptr<float>(offsetof(PairArgs, sqT)); p.s_c = m.ptr<float>(offsetof(PairArgs, s_c));
  p.w_q = m.ptr<float>(offsetof(PairArgs, w_q)); p.w_c = m.ptr<float>(offsetof(PairArgs, w_c));
  p.dense = m.ptr<float>(offsetof(PairArgs, dense)); p.l = m.ptr<Layer>(offsetof(PairArgs, l));
  p.Upad = static_cast<int32_t>(m.u32(offsetof(PairArgs, Upad))); p.H1 = static_cast<int32_t>(m.u32(offsetof(PairArgs, H1)));
  p.E = static_cast<int32_t>(m.u32(offsetof(PairArgs, E))); p.act = static_cast<int32_t>(m.u32(offsetof(PairArgs, act)));
  p.n_layers = static_cast<int32_t>(m.u32(offsetof(PairArgs, n_layers)));
  return p;
}

// The grid, the LDS lists and the selection of pair_score_topk_k; what enters the selection is the mean logit
//   z = (((z_0 + z_1) + z_2) + ... + z_{M-1}) / (float)M    ascending member order, one rounding per operation
// (mi_predict_group's definition), z_m = pair_score on member m's arguments (the VALU path: mi_pair_topk_group refuses a
// member whose own call would take the MFMA path).  The member table is read from device memory with wave-uniform
// addresses; nothing of it lives in LDS.
__global__ __launch_bounds__(kThreads) void pair_score_topk_group_k(const GroupMember* __restrict__ tab, int M,
                                                                   const uint32_t* __restrict__ excl, float* __restrict__ scores,
                                                                   float* __restrict__ member_scores, uint64_t* __restrict__ part,
                                                                   int64_t U, int64_t I, int64_t chunk, int K, int splits,
                                                                   int words) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* list = reinterpret_cast<uint64_t*>(lds);             // [kQB][K], descending, 0 = empty
  uint64_t* surv = list + kQB * K;                                // [kQB][kSurv]
  int* nsurv = reinterpret_cast<int*>(surv + kQB * kSurv);        // [kQB]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQB;
  const int split = blockIdx.y;
  const int64_t c_begin = split * chunk;
  const int64_t c_end = c_begin + chunk < I ? c_begin + chunk : I;
  for (int i = tid; i < kQB * K; i += kThreads) list[i] = 0;
  if (tid < kQB) nsurv[tid] = 0;
  __syncthreads();
  const int64_t q = q0 + col;
  const bool q_ok = q < U;
  const float fM = static_cast<float>(M);
  for (int64_t base = c_begin; base < c_end; base += kWaves) {
    const int64_t c = base + wave;
    if (c < c_end) {                                              // (wave-uniform)
      float acc = 0.f;
      for (int m = 0; m < M; ++m) {
        const PairArgs p = load_member(tab + m);
        const float wq = (p.w_q && q_ok) ? p.w_q[q] : 0.f;
        const float* __restrict__ sq = p.sqT ? p.sqT + q0 + col : nullptr;
        const float z = pair_score<false, 1, 1>(p, c, q0 + col, h, wq, sq);
        if (member_scores && h == 0 && q_ok) member_scores[(static_cast<int64_t>(m) * U + q) * I + c] = z;
        acc = m == 0 ? z : acc + z;
      }
      const float s = acc / fM;
      if (h == 0 && q_ok) {
        if (scores) scores[q * I + c] = s;
        const bool excluded = excl && ((excl[q * words + (c >> 5)] >> (c & 31)) & 1u);
        if (!excluded) {
          const uint64_t key = rank_key(s, static_cast<uint32_t>(c));
          if (key > list[col * K + K - 1]) {
            const int slot = atomicAdd(&nsurv[col], 1);
            surv[col * kSurv + slot] = key;
          }
        }
      }
    }
    // (as in pair_score_topk_k: the counts are read only after every wave's appends of this round are in)
    __syncthreads();
    if (__syncthreads_or(tid < kQB && nsurv[tid] > kSurv - kWaves)) merge_survivors(list, surv, nsurv, K, wave, lane);
  }
  __syncthreads();
  if (__syncthreads_or(tid < kQB && nsurv[tid] > 0)) merge_survivors(list, surv, nsurv, K, wave, lane);
  for (int i = tid; i < kQB * K; i += kThreads) {
    const int qq = i / K;
    if (q0 + qq < U) part[((q0 + qq) * splits + split) * K + (i - qq * K)] = list[i];
  }
}

// ---- exact ranks of named targets, every member for itself (mi_pair_target_ranks) ----------------------------------
// Grid (query blocks of 32) x (candidate splits) x (members).  A workgroup first scores its 32 queries' targets with its
// member's pair_score (the candidate differs per lane: a_c, s_c and w_c become per-lane loads) and keeps their keys in LDS,
// then runs pair_score_topk_k's candidate loop over its chunk — a wave scores ONE candidate against the 32 queries — and
// counts, per target of the query, whether the candidate's key is larger.  Keys of one query are distinct and a target's
// own pair scores to the target's own bits, so the count never includes the target.
//   tkey [Tq][kQB]          the targets' keys; ~0 (above every key) where the target has no rank
//   cnt  [kWaves][Tq][kQB]  one set of counters per wave: lane (col, h) alone adds to targets j = h, h + 2, ... of query
//                           col in its wave's set, so the adds are plain LDS read-modify-writes — no atomics, no barrier in
//                           the candidate loop, and the idle half of the VALU path's wave does half of the compares
// The split's counts go plainly to part [M][splits][U][Tq] (-1: no rank); rank_sum_k adds the splits.  Integers only: the
// result depends neither on the split count nor on timing, and no workgroup waits for another.
constexpr uint64_t kNoRank = ~static_cast<uint64_t>(0);

__global__ __launch_bounds__(kThreads) void pair_target_ranks_k(const GroupMember* __restrict__ tab,
                                                               const uint32_t* __restrict__ excl,
                                                               const int32_t* __restrict__ targets,
                                                               float* __restrict__ target_scores, int32_t* __restrict__ part,
                                                               int64_t U, int64_t I, int64_t chunk, int Tq, int splits, int words) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* tkey = reinterpret_cast<uint64_t*>(lds);             // [Tq][kQB]
  int* cnt = reinterpret_cast<int*>(tkey + Tq * kQB);             // [kWaves][Tq][kQB]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQB;
  const int split = blockIdx.y, m = blockIdx.z;
  const int64_t c_begin = split * chunk;
  const int64_t c_end = c_begin + chunk < I ? c_begin + chunk : I;
  const PairArgs p = load_member(tab + m);
  const int64_t q = q0 + col;
  const bool q_ok = q < U;
  const float wq = (p.w_q && q_ok) ? p.w_q[q] : 0.f;
  const float* __restrict__ sq = p.sqT ? p.sqT + q0 + col : nullptr;
  for (int i = tid; i < kWaves * Tq * kQB; i += kThreads) cnt[i] = 0;
  // the targets: thread (col, j0 = tid / 32) takes targets j0, j0 + 8, ... of query col
  for (int j = tid >> 5; j < Tq; j += kThreads / kQB) {
    uint64_t key = kNoRank;
    float s = __uint_as_float(0x7fc00000u);
    if (q_ok) {
      const int64_t t = targets[q * Tq + j];
      if (t >= 0 && t < I && !(excl && ((excl[q * words + (t >> 5)] >> (t & 31)) & 1u))) {
        s = pair_score<false, 1, 1>(p, t, q0 + col, 0, wq, sq);
        key = rank_key(s, static_cast<uint32_t>(t));
      }
      if (split == 0 && target_scores) target_scores[(static_cast<int64_t>(m) * U + q) * Tq + j] = s;
    }
    tkey[j * kQB + col] = key;
  }
  __syncthreads();
  int* mine = cnt + wave * Tq * kQB + col;
  for (int64_t c = c_begin + wave; c < c_end; c += kWaves) {     // (c is wave-uniform)
    const float s = pair_score<false, 1, 1>(p, c, q0 + col, h, wq, sq);
    if (q_ok && !(excl && ((excl[q * words + (c >> 5)] >> (c & 31)) & 1u))) {
      const uint64_t key = rank_key(s, static_cast<uint32_t>(c));
      for (int j = h; j < Tq; j += 2) mine[j * kQB] += key > tkey[j * kQB + col];
    }
  }
  __syncthreads();
  // thread i = (query i / Tq, target i % Tq): the block's rows of part are contiguous
  int32_t* out = part + ((static_cast<int64_t>(m) * splits + split) * U + q0) * Tq;
  const int64_t rows = U - q0 < kQB ? U - q0 : kQB;
  for (int i = tid; i < rows * Tq; i += kThreads) {
    const int qq = i / Tq, j = i - qq * Tq, at = j * kQB + qq;
    int n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += cnt[w * Tq * kQB + at];
    out[i] = tkey[at] == kNoRank ? -1 : n;
  }
}

// ---- exact ranks of named targets under the members' mean score (mi_pair_target_ranks_mean) -------------------------
// The mean logit of pair (q, c) as pair_score_topk_group_k forms it: ascending member order, one rounding per operation,
//   z = (((z_0 + z_1) + z_2) + ... + z_{M-1}) / (float)M
// c may differ per lane (a target) or be the wave's one candidate; q_ok: the lane's query exists (qcol < U).
__device__ __forceinline__ float mean_pair_score(const GroupMember* __restrict__ tab, int M, float fM, int64_t c, int64_t qcol,
                                                 bool q_ok, int h) {
  float acc = 0.f;
  for (int m = 0; m < M; ++m) {
    const PairArgs p = load_member(tab + m);
    const float wq = (p.w_q && q_ok) ? p.w_q[qcol] : 0.f;
    const float* __restrict__ sq = p.sqT ? p.sqT + qcol : nullptr;
    const float z = pair_score<false, 1, 1>(p, c, qcol, h, wq, sq);
    acc = m == 0 ? z : acc + z;
  }
  return acc / fM;
}

// pair_target_ranks_k with the members as a loop instead of a grid axis: grid (query blocks of 32) x (candidate splits),
// tkey [Tq][kQB] and cnt [kWaves][Tq][kQB] as there, and both the targets' keys and the candidates' keys come from
// mean_pair_score — a target's own pair gives the target's own bits and never counts itself.  Every lane scores a target
// (candidate 0 where it has none, the result dropped): the member loop's wave-uniform reads never run under an empty
// exec mask.  The split's counts go plainly to part [splits][U][Tq] (-1: no rank); rank_sum_k (one "member") adds them.
__global__ __launch_bounds__(kThreads) void pair_target_ranks_mean_k(const GroupMember* __restrict__ tab, int M,
                                                                    const uint32_t* __restrict__ excl,
                                                                    const int32_t* __restrict__ targets,
                                                                    float* __restrict__ target_scores, int32_t* __restrict__ part,
                                                                    int64_t U, int64_t I, int64_t chunk, int Tq, int splits,
                                                                    int words) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* tkey = reinterpret_cast<uint64_t*>(lds);             // [Tq][kQB]
  int* cnt = reinterpret_cast<int*>(tkey + Tq * kQB);             // [kWaves][Tq][kQB]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQB;
  const int split = blockIdx.y;
  const int64_t c_begin = split * chunk;
  const int64_t c_end = c_begin + chunk < I ? c_begin + chunk : I;
  const int64_t q = q0 + col;
  const bool q_ok = q < U;
  const float fM = static_cast<float>(M);
  for (int i = tid; i < kWaves * Tq * kQB; i += kThreads) cnt[i] = 0;
  // the targets: thread (col, j0 = tid / 32) takes targets j0, j0 + 8, ... of query col
  for (int j = tid >> 5; j < Tq; j += kThreads / kQB) {
    int64_t t = q_ok ? targets[q * Tq + j] : -1;
    const bool has = t >= 0 && t < I && !(excl && ((excl[q * words + (t >> 5)] >> (t & 31)) & 1u));
    if (!has) t = 0;
    float s = mean_pair_score(tab, M, fM, t, q, q_ok, 0);
    uint64_t key = rank_key(s, static_cast<uint32_t>(t));
    if (!has) {
      s = __uint_as_float(0x7fc00000u);
      key = kNoRank;
    }
    if (q_ok && split == 0 && target_scores) target_scores[q * Tq + j] = s;
    tkey[j * kQB + col] = key;
  }
  __syncthreads();
  int* mine = cnt + wave * Tq * kQB + col;
  for (int64_t c = c_begin + wave; c < c_end; c += kWaves) {     // (c is wave-uniform)
    const float s = mean_pair_score(tab, M, fM, c, q, q_ok, h);
    if (q_ok && !(excl && ((excl[q * words + (c >> 5)] >> (c & 31)) & 1u))) {
      const uint64_t key = rank_key(s, static_cast<uint32_t>(c));
      for (int j = h; j < Tq; j += 2) mine[j * kQB] += key > tkey[j * kQB + col];
    }
  }
  __syncthreads();
  // thread i = (query i / Tq, target i % Tq): the block's rows of part are contiguous
  int32_t* out = part + (static_cast<int64_t>(split) * U + q0) * Tq;
  const int64_t rows = U - q0 < kQB ? U - q0 : kQB;
  for (int i = tid; i < rows * Tq; i += kThreads) {
    const int qq = i / Tq, j = i - qq * Tq, at = j * kQB + qq;
    int n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += cnt[w * Tq * kQB + at];
    out[i] = tkey[at] == kNoRank ? -1 : n;
  }
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

// The group's member table reaches the workspace through the kernel arguments, kTabChunk members a launch (compile-time
// indices: see PairArgs::l) — no host-to-device copy, so the call neither synchronises nor needs pinned memory.
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
  float* __restrict__ dst = const_cast<float*>(a ? gm.p.aqT : gm.p.sqT);
  if (!dst) return;
  const int W = a ? gm.p.H1 : gm.p.E, Upad = gm.p.Upad;
  const int64_t n = static_cast<int64_t>(W) * Upad;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t k = i / Upad, q = i - k * Upad;
    dst[i] = q < U ? src[q * W + k] : 0.f;
  }
}

struct Plan {
  int64_t Upad, qblocks, chunk;
  int32_t splits, words;
  size_t off_layers, off_aq, off_sq, off_mask, off_part, total;
};

inline size_t align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }

// workgroups of 256 threads for the n elements of a grid-stride kernel (at most 2048)
inline unsigned grid_blocks(int64_t n) { const int64_t b = mi::ceil_div(n, 256); return static_cast<unsigned>(b < 2048 ? b : 2048); }

Plan make_plan(int64_t U, int64_t I, int32_t k, int32_t H1, int32_t E) {
  Plan pl;
  pl.qblocks = mi::ceil_div(U, kQB);
  pl.Upad = pl.qblocks * kQB;
  int64_t s = mi::ceil_div(kTargetBlocks, pl.qblocks);
  const int64_t s_lds = kMergeLds / (8 * static_cast<int64_t>(k));
  const int64_t s_min_chunk = mi::ceil_div(I, 64);                 // at least 64 candidates per split
  if (s > s_lds) s = s_lds;
  if (s > s_min_chunk) s = s_min_chunk;
  if (s < 1) s = 1;
  pl.chunk = mi::ceil_div(I, s);
  pl.splits = static_cast<int32_t>(mi::ceil_div(I, pl.chunk));
  pl.words = static_cast<int32_t>(mi::ceil_div(I, 32));
  size_t o = 0;
  pl.off_layers = o; o += align256(sizeof(Layer) * kMaxLayers);
  pl.off_aq = o; o += align256(sizeof(float) * static_cast<size_t>(H1) * pl.Upad);
  pl.off_sq = o; o += align256(sizeof(float) * static_cast<size_t>(E) * pl.Upad);
  pl.off_mask = o; o += align256(sizeof(uint32_t) * static_cast<size_t>(U) * pl.words);
  pl.off_part = o; o += align256(sizeof(uint64_t) * static_cast<size_t>(U) * pl.splits * k);
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

// What the group shares (query blocks, splits, exclusion mask, partial lists: make_plan with no per-model tensors) and
// where the member table and the members' transposes lie in the workspace.
constexpr size_t kMaxGroupLds = 160 * 1024;      // the dynamic LDS a launch can be raised to on gfx950

struct GroupPlan {
  Plan pl;
  size_t off_table, off_sides, total;
};

inline size_t side_bytes(const Plan& pl, int32_t H1, int32_t E) {
  return align256(sizeof(float) * static_cast<size_t>(H1) * pl.Upad) + align256(sizeof(float) * static_cast<size_t>(E) * pl.Upad);
}

bool group_sizes_ok(const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t k) {
  if (!members || n < 1 || n > MI_PAIR_TOPK_GROUP_MAX_MEMBERS) return false;
  for (int32_t i = 0; i < n; ++i)
    if (!sizes_ok(U, I, k, members[i].H1, members[i].E)) return false;
  return true;
}

GroupPlan make_group_plan(const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t k) {
  GroupPlan gp;
  gp.pl = make_plan(U, I, k, 0, 0);
  size_t o = gp.pl.total;
  gp.off_table = o; o += align256(sizeof(GroupMember) * static_cast<size_t>(n));
  gp.off_sides = o;
  for (int32_t i = 0; i < n; ++i) o += side_bytes(gp.pl, members[i].H1, members[i].E);
  gp.total = o;
  return gp;
}

// mi_pair_target_ranks: make_plan's split rule — at least 64 candidates per split, about kTargetBlocks workgroups — over
// query blocks x members (no selection lists: nothing else bounds the splits), and the workspace: the exclusion mask, the
// splits' partial counts, the member table and the members' transposes.  pl: what side_bytes and the table need of a Plan.
// mi_pair_target_ranks_mean (mean = true): the members are a loop in the kernel, not a grid axis — the member factor drops
// out of the split rule and of the partial counts.
struct RanksPlan {
  Plan pl;
  size_t off_mask, off_part, off_table, off_sides, total;
};

bool ranks_sizes_ok(const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t Tq) {
  return Tq >= 1 && Tq <= MI_PAIR_RANKS_MAX_TARGETS && group_sizes_ok(members, n, U, I, 1);
}

RanksPlan make_ranks_plan(const mi_rank_member_t* members, int32_t n, int64_t U, int64_t I, int32_t Tq, bool mean = false) {
  RanksPlan rp{};
  Plan& pl = rp.pl;
  const int32_t grid_members = mean ? 1 : n;
  pl.qblocks = mi::ceil_div(U, kQB);
  pl.Upad = pl.qblocks * kQB;
  int64_t s = mi::ceil_div(kTargetBlocks, pl.qblocks * grid_members);
  const int64_t s_min_chunk = mi::ceil_div(I, 64);
  if (s > s_min_chunk) s = s_min_chunk;
  if (s < 1) s = 1;
  pl.chunk = mi::ceil_div(I, s);
  pl.splits = static_cast<int32_t>(mi::ceil_div(I, pl.chunk));
  pl.words = static_cast<int32_t>(mi::ceil_div(I, 32));
  size_t o = 0;
  rp.off_mask = o; o += align256(sizeof(uint32_t) * static_cast<size_t>(U) * pl.words);
  rp.off_part = o; o += align256(sizeof(int32_t) * static_cast<size_t>(grid_members) * pl.splits * U * Tq);
  rp.off_table = o; o += align256(sizeof(GroupMember) * static_cast<size_t>(n));
  rp.off_sides = o;
  for (int32_t i = 0; i < n; ++i) o += side_bytes(pl, members[i].H1, members[i].E);
  rp.total = o;
  return rp;
}

// What mi_pair_target_ranks and mi_pair_target_ranks_mean (`who`, for the texts) refuse before anything is launched, in
// their order: the member count, the per-call arguments, then every member — check_model with k = 1, and the VALU scope.
int32_t check_ranks_call(const char* who, const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                         const int64_t* excl_off, const int32_t* excl_idx, const int32_t* targets, int32_t Tq,
                         const int32_t* ranks) {
  MI_REQUIRE(n_members >= 1, "%s: %d members (at least 1)", who, n_members);
  if (n_members > MI_PAIR_TOPK_GROUP_MAX_MEMBERS)
    return unsupported("%s: %d members (at most %d in one launch)", who, n_members, MI_PAIR_TOPK_GROUP_MAX_MEMBERS);
  MI_REQUIRE(members, "%s: members", who);
  MI_REQUIRE(Tq >= 1 && Tq <= MI_PAIR_RANKS_MAX_TARGETS, "%s: Tq=%d targets per query (1 to %d in one call)", who, Tq,
             MI_PAIR_RANKS_MAX_TARGETS);
  MI_REQUIRE(targets && ranks, "%s: targets / ranks", who);
  MI_REQUIRE(!excl_off == !excl_idx, "%s: excl_off and excl_idx go together", who);
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_rank_member_t& m = members[i];
    LayerTable lt{};
    int maxw = 0;
    const int32_t rc = check_model(U, I, 1, m.a_q, m.s_q, m.a_c, m.s_c, m.H1, m.E, m.dense, m.layer_off, m.widths, m.n_layers,
                                   m.activation, true, true, lt, maxw);
    if (rc != MI_OK) {
      mi::member_error(who, i);
      return rc;
    }
    if (takes_mfma(m.n_layers, maxw))
      return unsupported("%s: member %d: %d layers after layer 1 with a hidden width of %d: the kernel takes the "
                         "VALU pair path only (fewer than two layers after layer 1, or every hidden width after layer 1 below "
                         "%d)", who, i, m.n_layers, maxw, kValuW);
  }
  return MI_OK;
}

// The launches in front of a rank entry's scoring launch: the member table, as mi_pair_topk_group writes it (the
// selection's fields of PairArgs stay zero: nothing here reads them), one transpose launch for all members, the mask.
void prepare_ranks(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                   const int32_t* excl_idx, const RanksPlan& rp, char* ws, GroupMember* tab, uint32_t* mask, hipStream_t st) {
  const Plan& pl = rp.pl;
  size_t side = rp.off_sides;
  int maxside = 0;
  MemberChunk ch{};
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_rank_member_t& m = members[i];
    GroupMember& gm = ch.m[i % kTabChunk];
    gm = GroupMember{};
    for (int j = 0; j < m.n_layers; ++j)
      gm.l[j] = Layer{m.layer_off[2 * j], m.layer_off[2 * j + 1], m.widths[j], m.widths[j + 1]};
    PairArgs& a = gm.p;
    a.aqT = m.H1 ? reinterpret_cast<float*>(ws + side) : nullptr;
    a.sqT = m.E ? reinterpret_cast<float*>(ws + side + align256(sizeof(float) * static_cast<size_t>(m.H1) * pl.Upad)) : nullptr;
    side += side_bytes(pl, m.H1, m.E);
    a.a_c = m.a_c; a.s_c = m.s_c; a.w_q = m.w_q; a.w_c = m.w_c; a.dense = m.dense;
    a.l = tab[i].l;                              // (the address of this member's layers in the workspace)
    a.U = U; a.I = I;
    a.Upad = static_cast<int32_t>(pl.Upad); a.H1 = m.H1; a.E = m.E; a.act = m.activation; a.n_layers = m.n_layers;
    gm.a_q = m.a_q; gm.s_q = m.s_q;
    if (m.H1 > maxside) maxside = m.H1;
    if (m.E > maxside) maxside = m.E;
    if (i % kTabChunk == kTabChunk - 1 || i + 1 == n_members) {
      const int first = i - i % kTabChunk;
      member_table_k<<<dim3(1), dim3(64), 0, st>>>(ch, i - first + 1, tab + first);
    }
  }
  if (maxside)
    transpose_pad_group_k<<<dim3(grid_blocks(static_cast<int64_t>(maxside) * pl.Upad), static_cast<unsigned>(n_members), 2), dim3(256), 0,
                            st>>>(tab, U);
  if (mask) {
    zero_u32_k<<<dim3(grid_blocks(U * pl.words)), dim3(256), 0, st>>>(mask, U * pl.words);
    excl_mask_k<<<dim3(static_cast<unsigned>(U)), dim3(256), 0, st>>>(excl_off, excl_idx, I, pl.words, mask);
  }
}

template <bool MFMA, int NP, int NQ>
int32_t launch_pair(const PairArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  const int32_t rl = mi::raise_lds(&pair_score_topk_k<MFMA, NP, NQ>, lds, "pair_topk");
  if (rl != MI_OK) return rl;
  pair_score_topk_k<MFMA, NP, NQ><<<grid, dim3(kThreads), lds, st>>>(a);
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
  PairArgs a{};
  LayerTable lt{};
  int maxw = 0;
  const int32_t rc = check_model(U, I, k, a_q, s_q, a_c, s_c, H1, E, dense, layer_off, widths, n_layers, activation,
                                 top_score && top_idx, !excl_off == !excl_idx, lt, maxw);
  if (rc != MI_OK) return rc;
  a.n_layers = n_layers;
  const Plan pl = make_plan(U, I, k, H1, E);
  MI_REQUIRE(workspace && workspace_bytes >= pl.total, "pair_topk: workspace %zu < %zu bytes", workspace_bytes, pl.total);
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  float* aqT = H1 ? reinterpret_cast<float*>(ws + pl.off_aq) : nullptr;
  float* sqT = E ? reinterpret_cast<float*>(ws + pl.off_sq) : nullptr;
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + pl.off_mask) : nullptr;
  uint64_t* part = reinterpret_cast<uint64_t*>(ws + pl.off_part);
  auto blocks = [](int64_t n) { const int64_t b = mi::ceil_div(n, 256); return static_cast<unsigned>(b < 2048 ? b : 2048); };
  Layer* layers = reinterpret_cast<Layer*>(ws + pl.off_layers);
  if (n_layers) layer_table_k<<<dim3(1), dim3(64), 0, st>>>(lt, n_layers, layers);
  if (aqT) transpose_pad_k<<<dim3(blocks(static_cast<int64_t>(H1) * pl.Upad)), dim3(256), 0, st>>>(a_q, U, H1, (int)pl.Upad, aqT);
  if (sqT) transpose_pad_k<<<dim3(blocks(static_cast<int64_t>(E) * pl.Upad)), dim3(256), 0, st>>>(s_q, U, E, (int)pl.Upad, sqT);
  if (mask) {
    zero_u32_k<<<dim3(blocks(U * pl.words)), dim3(256), 0, st>>>(mask, U * pl.words);
    excl_mask_k<<<dim3(static_cast<unsigned>(U)), dim3(256), 0, st>>>(excl_off, excl_idx, I, pl.words, mask);
  }
  MI_CHECK_LAUNCH("pair_topk (prepare)");
  a.aqT = aqT; a.a_c = a_c; a.sqT = sqT; a.s_c = s_c; a.w_q = w_q; a.w_c = w_c; a.dense = dense;
  a.excl = mask; a.scores = scores; a.part = part; a.l = layers;
  a.U = U; a.I = I; a.chunk = pl.chunk;
  a.Upad = static_cast<int32_t>(pl.Upad); a.H1 = H1; a.E = E; a.K = k; a.splits = pl.splits; a.words = pl.words;
  a.act = activation;
  const size_t lds = sizeof(uint64_t) * kQB * (k + kSurv) + sizeof(int) * kQB;
  const dim3 grid(static_cast<unsigned>(pl.qblocks), static_cast<unsigned>(pl.splits));
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
  topk_merge_k<<<dim3(static_cast<unsigned>(U)), dim3(256), sizeof(uint64_t) * pl.splits * k, st>>>(part, pl.splits, k,
                                                                                                    top_score, top_idx);
  MI_CHECK_LAUNCH("topk_merge_k");
  return MI_OK;
}

size_t mi_pair_topk_group_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, int32_t k) {
  if (!group_sizes_ok(members, n_members, U, I, k)) return 0;
  return make_group_plan(members, n_members, U, I, k).total;
}

int32_t mi_pair_topk_group(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                           const int32_t* excl_idx, int32_t k, float* top_score, int32_t* top_idx, float* scores,
                           float* member_scores, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_REQUIRE(n_members >= 1, "pair_topk_group: %d members (at least 1)", n_members);
  if (n_members > MI_PAIR_TOPK_GROUP_MAX_MEMBERS)
    return unsupported("pair_topk_group: %d members (at most %d in one launch)", n_members, MI_PAIR_TOPK_GROUP_MAX_MEMBERS);
  MI_REQUIRE(members, "pair_topk_group: members");
  MI_REQUIRE(top_score && top_idx, "pair_topk_group: top_score / top_idx");
  MI_REQUIRE(!excl_off == !excl_idx, "pair_topk_group: excl_off and excl_idx go together");
  // every member is checked before anything is launched
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_rank_member_t& m = members[i];
    LayerTable lt{};
    int maxw = 0;
    const int32_t rc = check_model(U, I, k, m.a_q, m.s_q, m.a_c, m.s_c, m.H1, m.E, m.dense, m.layer_off, m.widths, m.n_layers,
                                   m.activation, true, true, lt, maxw);
    if (rc != MI_OK) {
      mi::member_error("pair_topk_group", i);
      return rc;
    }
    if (takes_mfma(m.n_layers, maxw))
      return unsupported("pair_topk_group: member %d: %d layers after layer 1 with a hidden width of %d: the group kernel takes "
                         "the VALU pair path only (fewer than two layers after layer 1, or every hidden width after layer 1 "
                         "below %d)", i, m.n_layers, maxw, kValuW);
  }
  const GroupPlan gp = make_group_plan(members, n_members, U, I, k);
  const Plan& pl = gp.pl;
  MI_REQUIRE(workspace && workspace_bytes >= gp.total, "pair_topk_group: workspace %zu < %zu bytes", workspace_bytes, gp.total);
  const size_t lds = sizeof(uint64_t) * kQB * (k + kSurv) + sizeof(int) * kQB;    // (the lists; no member data lives in LDS)
  if (lds > kMaxGroupLds) return unsupported("pair_topk_group: %zu bytes of LDS for k=%d (at most %zu)", lds, k, kMaxGroupLds);
  const int32_t rl = mi::raise_lds(&pair_score_topk_group_k, lds, "pair_topk_group");
  if (rl != MI_OK) return rl;
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  GroupMember* tab = reinterpret_cast<GroupMember*>(ws + gp.off_table);
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + pl.off_mask) : nullptr;
  uint64_t* part = reinterpret_cast<uint64_t*>(ws + pl.off_part);
  auto blocks = [](int64_t n) { const int64_t b = mi::ceil_div(n, 256); return static_cast<unsigned>(b < 2048 ? b : 2048); };
  size_t side = gp.off_sides;
  int maxside = 0;
  MemberChunk ch{};
  for (int32_t i = 0; i < n_members; ++i) {
    const mi_rank_member_t& m = members[i];
    GroupMember& gm = ch.m[i % kTabChunk];
    gm = GroupMember{};
    for (int j = 0; j < m.n_layers; ++j)
      gm.l[j] = Layer{m.layer_off[2 * j], m.layer_off[2 * j + 1], m.widths[j], m.widths[j + 1]};
    float* aqT = m.H1 ? reinterpret_cast<float*>(ws + side) : nullptr;
    float* sqT = m.E ? reinterpret_cast<float*>(ws + side + align256(sizeof(float) * static_cast<size_t>(m.H1) * pl.Upad)) : nullptr;
    side += side_bytes(pl, m.H1, m.E);
    PairArgs& a = gm.p;
    a.aqT = aqT; a.a_c = m.a_c; a.sqT = sqT; a.s_c = m.s_c; a.w_q = m.w_q; a.w_c = m.w_c; a.dense = m.dense;
    a.l = tab[i].l;                              // (the address of this member's layers in the workspace)
    a.U = U; a.I = I; a.chunk = pl.chunk;
    a.Upad = static_cast<int32_t>(pl.Upad); a.H1 = m.H1; a.E = m.E; a.K = k; a.splits = pl.splits; a.words = pl.words;
    a.act = m.activation; a.n_layers = m.n_layers;
    gm.a_q = m.a_q; gm.s_q = m.s_q;
    if (m.H1 > maxside) maxside = m.H1;
    if (m.E > maxside) maxside = m.E;
    if (i % kTabChunk == kTabChunk - 1 || i + 1 == n_members) {
      const int first = i - i % kTabChunk;
      member_table_k<<<dim3(1), dim3(64), 0, st>>>(ch, i - first + 1, tab + first);
    }
  }
  if (maxside)
    transpose_pad_group_k<<<dim3(blocks(static_cast<int64_t>(maxside) * pl.Upad), static_cast<unsigned>(n_members), 2), dim3(256), 0,
                            st>>>(tab, U);
  if (mask) {
    zero_u32_k<<<dim3(blocks(U * pl.words)), dim3(256), 0, st>>>(mask, U * pl.words);
    excl_mask_k<<<dim3(static_cast<unsigned>(U)), dim3(256), 0, st>>>(excl_off, excl_idx, I, pl.words, mask);
  }
  MI_CHECK_LAUNCH("pair_topk_group (prepare)");
  pair_score_topk_group_k<<<dim3(static_cast<unsigned>(pl.qblocks), static_cast<unsigned>(pl.splits)), dim3(kThreads), lds, st>>>(
      tab, n_members, mask, scores, member_scores, part, U, I, pl.chunk, k, pl.splits, pl.words);
  MI_CHECK_LAUNCH("pair_score_topk_group_k");
  topk_merge_k<<<dim3(static_cast<unsigned>(U)), dim3(256), sizeof(uint64_t) * pl.splits * k, st>>>(part, pl.splits, k,
                                                                                                    top_score, top_idx);
  MI_CHECK_LAUNCH("topk_merge_k");
  return MI_OK;
}

size_t mi_pair_target_ranks_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, int32_t Tq) {
  if (!ranks_sizes_ok(members, n_members, U, I, Tq)) return 0;
  return make_ranks_plan(members, n_members, U, I, Tq).total;
}

int32_t mi_pair_target_ranks(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                             const int32_t* excl_idx, const int32_t* targets, int32_t Tq, int32_t* ranks, float* target_scores,
                             void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  const int32_t rc = check_ranks_call("pair_target_ranks", members, n_members, U, I, excl_off, excl_idx, targets, Tq, ranks);
  if (rc != MI_OK) return rc;
  const RanksPlan rp = make_ranks_plan(members, n_members, U, I, Tq);
  const Plan& pl = rp.pl;
  MI_REQUIRE(workspace && workspace_bytes >= rp.total, "pair_target_ranks: workspace %zu < %zu bytes", workspace_bytes, rp.total);
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  GroupMember* tab = reinterpret_cast<GroupMember*>(ws + rp.off_table);
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + rp.off_mask) : nullptr;
  int32_t* part = reinterpret_cast<int32_t*>(ws + rp.off_part);
  prepare_ranks(members, n_members, U, I, excl_off, excl_idx, rp, ws, tab, mask, st);
  MI_CHECK_LAUNCH("pair_target_ranks (prepare)");
  const size_t lds = (sizeof(uint64_t) + sizeof(int) * kWaves) * kQB * static_cast<size_t>(Tq);      // at most 48 KB
  pair_target_ranks_k<<<dim3(static_cast<unsigned>(pl.qblocks), static_cast<unsigned>(pl.splits), static_cast<unsigned>(n_members)),
                        dim3(kThreads), lds, st>>>(tab, mask, targets, target_scores, part, U, I, pl.chunk, Tq, pl.splits, pl.words);
  MI_CHECK_LAUNCH("pair_target_ranks_k");
  const int64_t n = U * Tq;
  rank_sum_k<<<dim3(grid_blocks(n), static_cast<unsigned>(n_members)), dim3(256), 0, st>>>(part, pl.splits, n, ranks);
  MI_CHECK_LAUNCH("rank_sum_k");
  return MI_OK;
}

size_t mi_pair_target_ranks_mean_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                                                 int32_t Tq) {
  if (!ranks_sizes_ok(members, n_members, U, I, Tq)) return 0;
  return make_ranks_plan(members, n_members, U, I, Tq, true).total;
}

int32_t mi_pair_target_ranks_mean(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                                  const int64_t* excl_off, const int32_t* excl_idx, const int32_t* targets, int32_t Tq,
                                  int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes,
                                  mi_stream_t stream) {
  const int32_t rc = check_ranks_call("pair_target_ranks_mean", members, n_members, U, I, excl_off, excl_idx, targets, Tq, ranks);
  if (rc != MI_OK) return rc;
  const RanksPlan rp = make_ranks_plan(members, n_members, U, I, Tq, true);
  const Plan& pl = rp.pl;
  MI_REQUIRE(workspace && workspace_bytes >= rp.total, "pair_target_ranks_mean: workspace %zu < %zu bytes", workspace_bytes,
             rp.total);
  hipStream_t st = mi::as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  GroupMember* tab = reinterpret_cast<GroupMember*>(ws + rp.off_table);
  uint32_t* mask = excl_off ? reinterpret_cast<uint32_t*>(ws + rp.off_mask) : nullptr;
  int32_t* part = reinterpret_cast<int32_t*>(ws + rp.off_part);
  prepare_ranks(members, n_members, U, I, excl_off, excl_idx, rp, ws, tab, mask, st);
  MI_CHECK_LAUNCH("pair_target_ranks_mean (prepare)");
  const size_t lds = (sizeof(uint64_t) + sizeof(int) * kWaves) * kQB * static_cast<size_t>(Tq);      // at most 48 KB
  pair_target_ranks_mean_k<<<dim3(static_cast<unsigned>(pl.qblocks), static_cast<unsigned>(pl.splits)), dim3(kThreads), lds, st>>>(
      tab, n_members, mask, targets, target_scores, part, U, I, pl.chunk, Tq, pl.splits, pl.words);
  MI_CHECK_LAUNCH("pair_target_ranks_mean_k");
  const int64_t n = U * Tq;
  rank_sum_k<<<dim3(grid_blocks(n), 1), dim3(256), 0, st>>>(part, pl.splits, n, ranks);
  MI_CHECK_LAUNCH("rank_sum_k");
  return MI_OK;
}

}  // extern "C"
