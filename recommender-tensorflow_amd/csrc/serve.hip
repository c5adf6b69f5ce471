// Serving: the whole forward of a request batch — DeepFM.predict_logits followed by mi_binary_predictions — as ONE
// launch (mi_predict_fused, include/mi355x_rec.h).  Ids in, predictions out; no intermediate reaches HBM.
//
//   predict_fused_k   one workgroup of 4 waves per 32 requests.  The 32 requests are the columns of the fp32-input MFMA
//                     (the transposed form Y^T = W^T X^T of rank.hip: a layer's weights are the A operand, the requests'
//                     activations the B operand).
//     0. rows         the requests' table rows field_off[f] + ids[b, f] into LDS ([F][32] int32): the id -> row -> table
//                     chain of dependent loads is paid once, for all fields at a time.
//     1. wide + FM    8 threads per request: the wide part's weights by field, the FM sums by float4 column chunk
//                     (sum and sum of squares over the fields, each product rounded on its own: one field gives 0).
//     2. layer 1      B operand straight from the gathered table rows: a lane holds 4 consecutive embedding columns of
//                     its request's row (one 16-byte load) and spends them in 4 MFMA steps; the two lane halves take
//                     neighbouring float4 chunks of the concat, so A reads kernel_0's rows in the same k order.  Numeric
//                     columns (x V, or the raw values) follow as scalar k steps.
//     3. layers 2..L  input from LDS as [width][32] fp32, output to the other LDS buffer, a barrier between layers.  The
//                     four waves split a layer's 32-row output tiles (tile t -> wave t % 4, at most 4 tiles per wave:
//                     widths up to 512).  The logits layer is the same code with one output row.
//     4. head         logit = ((lin + bias) + fm) + dnn, then the device functions of mi_binary_predictions.
//
//   serve_block       steps 0 to 3 and the sum of the head, as one __device__ function: the ONE definition of a request's
//                     logit, run by both kernels of this file.
//
//   predict_group_k   an ensemble of M models over one request batch in ONE launch (mi_predict_group): grid
//                     (ceil(B / 32), M), blockIdx.y = the member, blockIdx.x = the tile of 32 requests.  A workgroup copies
//                     its member's ServeArgs from the device table mi_predict_group_plan wrote into LDS, thread 0 fills in
//                     what changes per call (ids, x_num, B), and serve_block runs on it: member_logits[y, b] holds the bits
//                     of mi_predict_fused on that member alone.  The members of a tile are then combined inside the launch:
//       ticket        after its logits are stored and published (every wave drains its stores, a barrier, lane 0 issues an
//                     agent-scope release fence and waits again), lane 0 draws a ticket from tickets[tile] with a relaxed
//                     agent-scope fetch_add.  The workgroup that draws M - 1 is the tile's reducer — whichever member it is;
//                     the others are done.  "I am last" reaches the workgroup through red_lin (no further LDS object).
//       reduce        the reducer's lane 0 issues an agent-scope acquire fence, then a barrier; its first 32 threads read the
//                     M logits of their request with plain loads, z = (((z_0 + z_1) + z_2) + ...) / (float)M in ascending
//                     member order, one rounding per operation (this file is compiled -ffp-contract=off), and write the
//                     four outputs with the head of predict_fused_k.  It then stores 0 back to tickets[tile]: the array is
//                     zero again when the launch has completed.
//                     THIS IS THE FIRST KERNEL OF THE PROJECT IN WHICH A WORKGROUP READS WHAT ANOTHER WROTE IN THE SAME
//                     LAUNCH.  The invariant that still holds: NO WORKGROUP WAITS FOR ANOTHER — no spin, no grid barrier, no
//                     cooperative launch, no float atomics.  Every workgroup runs to its end whatever the others do, so the
//                     kernel cannot hang, and since the reducer is defined by the count alone and adds in member order,
//                     the result depends on neither the dispatch order nor the placement of the grid.  A workgroup-scope
//                     fence or a plain flag would not publish the logits to a workgroup on another XCD; the agent-scope
//                     pair does.  M = 1 takes the same path: the only arriver is the reducer and z_0 / 1.0f is z_0.
//
// Arithmetic: fp32 variables, exact fp32 products (v_mfma_f32_32x32x2_f32), fp32 accumulation.  At request sizes the
// kernel waits for weights, not for the matrix pipe: no 16-bit operand split.
#include <memory>
#include <new>

#include "common.h"

namespace {

constexpr int kRB = 32;                 // requests per workgroup = the MFMA's N
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kParts = kThreads / kRB;  // threads per request in the wide + FM phase
constexpr int kTPW = 4;                 // output tiles per wave
constexpr int kMaxWidth = kTPW * kWaves * 32;   // 512
constexpr int kMaxFields = 64;
constexpr int kMaxLayers = 9;           // 8 hidden layers + the logits layer
constexpr size_t kMaxLds = 160 * 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Layer {
  int64_t w_off, b_off;                 // offsets into the flat dense buffer: kernel [fan_in, fan_out], bias [fan_out]
  int32_t fan_in, fan_out;
};

struct ServeArgs {
  const float* table;                   // [R][ts] or NULL
  const float* lin_w;                   // [R] at stride ls, or NULL
  const int64_t* field_off;             // [F]
  const int32_t* ids;                   // [B][F]
  const float* x_num;                   // [B][nd] or NULL
  const float* dense;
  float* logits;
  float* logistic;
  float* probabilities;
  int64_t* class_ids;
  int64_t B, ts;
  int64_t lin_bias_off, num_emb_off, lin_num_off;
  uint64_t wide_fields;
  int32_t F, E, nd, ls, act, n_layers;
  int32_t use_linear, use_fm, raw;      // raw: numeric columns feed the MLP with the value itself
  int32_t buf_a;                        // floats of the first activation buffer (the second follows it)
  Layer l[kMaxLayers];
};

// row of a 32x32 accumulator tile held in register r by lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// one k step (k = the lane half's own k) of every tile this wave owns
template <int NT>
__device__ __forceinline__ void mfma_step(f32x16 (&acc)[NT], const float* __restrict__ W, int k, bool k_ok, int N,
                                          int wave, int col, float hv) {
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int n = (i * kWaves + wave) * 32 + col;
    const float w = (k_ok && n < N) ? W[static_cast<int64_t>(k) * N + n] : 0.f;
    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, hv, acc[i], 0, 0, 0);
  }
}

// The k loops run in blocks of kKB steps, two blocks alternating: the weights (and inputs) of the next block are
// requested before the MFMAs of the current one, so a block's global-load latency hides behind the other block's
// matrix work instead of stalling every step (the loops are bound by the weight stream, not by the matrix pipe).
constexpr int kKB = 8;
template <int NT>
struct Blk {
  float hv[kKB];                        // B operand of step j (this lane half's k), as loaded
  uint32_t on;                          // bit j: step j lies inside the layer's k range (else its B operand counts as 0)
  float w[kKB][NT];                     // A operand of step j, tile i
};

// Loads past the matrix are clamped into it and nothing looks at a loaded value before compute(): straight-line code, so
// a block's loads are all in flight before its MFMAs.  A step past K is switched off through its B operand (0 times a
// finite weight), an output row past N is computed from the clamped column and never stored (epilogue).
template <int NT>
__device__ __forceinline__ void load_w(Blk<NT>& b, int j, const float* __restrict__ W, int k, int K, int N, int wave, int col) {
  const int64_t kr = static_cast<int64_t>(k < K ? k : K - 1) * N;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int n = (i * kWaves + wave) * 32 + col;
    b.w[j][i] = W[kr + (n < N ? n : N - 1)];
  }
}

template <int NT>
__device__ __forceinline__ void compute(f32x16 (&acc)[NT], const Blk<NT>& b, int N, int wave) {
#pragma unroll
  for (int j = 0; j < kKB; ++j) {
    const float hv = (b.on >> j) & 1u ? b.hv[j] : 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w[j][i], hv, acc[i], 0, 0, 0);
  }
}

// steps k0 .. k0 + 2 kKB of a layer whose input is in LDS
template <int NT>
__device__ __forceinline__ void load_hidden(Blk<NT>& b, const float* __restrict__ in, const float* __restrict__ W, int k0, int K,
                                            int N, int wave, int col, int h) {
  b.on = 0;
#pragma unroll
  for (int j = 0; j < kKB; ++j) {
    const int k = k0 + 2 * j + h;
    const bool on = k < K;
    b.hv[j] = in[(on ? k : K - 1) * kRB + col];
    b.on |= static_cast<uint32_t>(on) << j;
    load_w<NT>(b, j, W, k, K, N, wave, col);
  }
}

// layer 1: float4 chunks c0 + h and c0 + 2 + h of the concat (4 steps each); (f, ce) = the lane half's field and chunk
// inside the field, moved on by the call
template <int NT>
__device__ __forceinline__ void load_first(Blk<NT>& b, const float* __restrict__ table, int64_t ts, const int32_t* rows,
                                           const float* __restrict__ W, int c0, int nchunk, int cpf, int& f, int& ce, int F,
                                           int K, int N, int wave, int col, int h) {
  b.on = 0;
#pragma unroll
  for (int u = 0; u < kKB / 4; ++u) {
    const int c = c0 + 2 * u + h;
    const bool on = c < nchunk;
    const float4 v = ld4(table + static_cast<int64_t>(rows[(f < F ? f : F - 1) * kRB + col]) * ts + 4 * ce);   // (ce < cpf always)
    b.hv[4 * u] = v.x; b.hv[4 * u + 1] = v.y; b.hv[4 * u + 2] = v.z; b.hv[4 * u + 3] = v.w;
    b.on |= (on ? 15u : 0u) << (4 * u);
#pragma unroll
    for (int m = 0; m < 4; ++m) load_w<NT>(b, 4 * u + m, W, 4 * c + m, K, N, wave, col);
    ce += 2;
    while (ce >= cpf) { ce -= cpf; ++f; }
  }
}

// out[n][request] = act(acc + bias[n]) for the rows n < N of this wave's tiles
template <int NT>
__device__ __forceinline__ void epilogue(const f32x16 (&acc)[NT], const float* __restrict__ bias, int N, int act,
                                         float* __restrict__ out, int wave, int col, int h) {
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = i * kWaves + wave;
    if (t * 32 < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = t * 32 + acc_row(r, h);
        if (n < N) out[n * kRB + col] = mi_act(act, acc[i][r] + bias[n]);
      }
    }
  }
}

// one layer on this wave's NT tiles (tile i = output rows (i kWaves + wave) 32 ..): layer 1 from the table rows and the
// numeric columns, a later layer from the LDS buffer `in`; the result goes to the LDS buffer `out`
template <int NT>
__device__ __forceinline__ void run_layer(const ServeArgs& p, const Layer ly, bool first, bool last, const int32_t* rows,
                                          const float* __restrict__ xq, const float* __restrict__ in, float* __restrict__ out,
                                          int wave, int col, int h) {
  const float* __restrict__ W = p.dense + ly.w_off;
  const int K = ly.fan_in, N = ly.fan_out;
  const int F = p.F, E = p.E, nd = p.nd;
  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x16{};
  if (first) {
    // the concat's float4 chunks, two per step: chunk 2 i + h = columns 4 (ce) .. of field f
    const int cpf = E / 4, nchunk = p.table ? F * cpf : 0;
    if (nchunk) {
      constexpr int kCB = kKB / 2;                            // chunks a block covers (both lane halves)
      int f = h / cpf, ce = h - f * cpf;
      Blk<NT> ba, bb;
      load_first<NT>(ba, p.table, p.ts, rows, W, 0, nchunk, cpf, f, ce, F, K, N, wave, col, h);
      for (int c0 = 0; c0 < nchunk; c0 += 2 * kCB) {
        load_first<NT>(bb, p.table, p.ts, rows, W, c0 + kCB, nchunk, cpf, f, ce, F, K, N, wave, col, h);
        compute<NT>(acc, ba, N, wave);
        load_first<NT>(ba, p.table, p.ts, rows, W, c0 + 2 * kCB, nchunk, cpf, f, ce, F, K, N, wave, col, h);
        if (c0 + kCB < nchunk) compute<NT>(acc, bb, N, wave);
      }
    }
    // numeric columns: E columns x[b, j] V[j, :] each (numeric embeddings) or the value itself (raw)
    const int kc = 4 * nchunk, kn = nd * (p.raw ? 1 : E);
    const float* __restrict__ V = p.dense + p.num_emb_off;
    for (int k0 = 0; k0 < kn; k0 += 2) {
      const int kk = k0 + h;
      const bool on = kk < kn;
      float hv = 0.f;
      if (on) hv = p.raw ? xq[kk] : __fmul_rn(xq[kk / E], V[kk]);
      mfma_step<NT>(acc, W, kc + kk, on, N, wave, col, hv);
    }
  } else {
    Blk<NT> ba, bb;
    load_hidden<NT>(ba, in, W, 0, K, N, wave, col, h);
    for (int k0 = 0; k0 < K; k0 += 4 * kKB) {
      load_hidden<NT>(bb, in, W, k0 + 2 * kKB, K, N, wave, col, h);
      compute<NT>(acc, ba, N, wave);
      load_hidden<NT>(ba, in, W, k0 + 4 * kKB, K, N, wave, col, h);
      if (k0 + 2 * kKB < K) compute<NT>(acc, bb, N, wave);
    }
  }
  epilogue<NT>(acc, p.dense + ly.b_off, N, last ? 0 : p.act, out, wave, col, h);
}

// Steps 0 to 3 for the 32 requests b0 .. of p and the sum of the head: the logit of request b0 + tid in the threads
// tid < 32 whose request exists (0 elsewhere).  layers: the caller's LDS copy of p.l; lds: F 32 ints + the two buffers.
__device__ __forceinline__ float serve_block(const ServeArgs& p, char* lds, const Layer* layers, float (*red_lin)[kRB],
                                             float (*red_fm)[kRB], int64_t b0) {
  int32_t* rows = reinterpret_cast<int32_t*>(lds);                // [F][32]
  float* buf0 = reinterpret_cast<float*>(lds) + p.F * kRB;
  float* buf1 = buf0 + p.buf_a;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int F = p.F, E = p.E, nd = p.nd;
  // 0. the requests' rows (requests past B repeat the last one: loads stay legal, stores are predicated)
  for (int i = tid; i < F * kRB; i += kThreads) {
    const int f = i >> 5;
    const int64_t b = b0 + (i & 31) < p.B ? b0 + (i & 31) : p.B - 1;
    rows[i] = static_cast<int32_t>(p.field_off[f] + p.ids[b * F + f]);
  }
  __syncthreads();
  const int64_t bq = b0 + col < p.B ? b0 + col : p.B - 1;        // this lane's request
  const float* __restrict__ xq = p.x_num ? p.x_num + bq * nd : nullptr;

  // 1. wide part and FM term: part = tid / 32 of the request tid % 32
  {
    const int part = tid >> 5, c32 = tid & 31;
    float lacc = 0.f, t = 0.f;
    if (p.use_linear) {
      float lw[kMaxFields / kParts];                              // (all of a thread's weights requested at once)
#pragma unroll
      for (int i = 0; i < kMaxFields / kParts; ++i) {
        const int f = part + i * kParts;
        lw[i] = (f < F && ((p.wide_fields >> f) & 1u)) ? p.lin_w[static_cast<int64_t>(rows[f * kRB + c32]) * p.ls] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kMaxFields / kParts; ++i) lacc += lw[i];
      if (nd && !p.raw)                                           // numeric embeddings' linear weights (deep_fm.py:62-70)
        for (int j = part; j < nd; j += kParts) lacc += __fmul_rn(xq[j], p.dense[p.lin_num_off + j]);
    }
    if (p.use_fm) {
      const float* __restrict__ V = p.dense + p.num_emb_off;
      for (int c = part; c < E / 4; c += kParts) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
        constexpr int U = 8;                                      // rows in flight per thread
        for (int f0 = 0; f0 < F; f0 += U) {
          float4 r[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            r[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f0 + u < F) r[u] = ld4(p.table + static_cast<int64_t>(rows[(f0 + u) * kRB + c32]) * p.ts + 4 * c);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {                           // (a zero row adds exact zeros)
            s.x += r[u].x; s.y += r[u].y; s.z += r[u].z; s.w += r[u].w;
            q.x += __fmul_rn(r[u].x, r[u].x); q.y += __fmul_rn(r[u].y, r[u].y);
            q.z += __fmul_rn(r[u].z, r[u].z); q.w += __fmul_rn(r[u].w, r[u].w);
          }
        }
        for (int j = 0; j < nd; ++j) {                            // x[b, j] * V[j, :] is a row like any other
          const float4 v = ld4(V + j * E + 4 * c);
          const float xv = xq[j];
          const float4 r = make_float4(__fmul_rn(xv, v.x), __fmul_rn(xv, v.y), __fmul_rn(xv, v.z), __fmul_rn(xv, v.w));
          s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
          q.x += __fmul_rn(r.x, r.x); q.y += __fmul_rn(r.y, r.y); q.z += __fmul_rn(r.z, r.z); q.w += __fmul_rn(r.w, r.w);
        }
        // deep_fm.py:81-87: tf.square then subtract, products rounded on their own: one field gives exactly 0
        t += ((__fmul_rn(s.x, s.x) - q.x) + (__fmul_rn(s.y, s.y) - q.y)) +
             ((__fmul_rn(s.z, s.z) - q.z) + (__fmul_rn(s.w, s.w) - q.w));
      }
    }
    red_lin[part][c32] = lacc;
    red_fm[part][c32] = t;
  }

  // 2., 3. the MLP
  const int L = p.n_layers;
  float* in = buf1;
  float* out = buf0;
  for (int li = 0; li < L; ++li) {
    const Layer ly = layers[li];
    if (wave * 32 < ly.fan_out) {                                 // (a wave without a tile only keeps the barriers)
      const int nt = (ly.fan_out + 32 * kWaves - 1) / (32 * kWaves);
      if (nt <= 1) run_layer<1>(p, ly, li == 0, li + 1 == L, rows, xq, in, out, wave, col, h);
      else if (nt <= 2) run_layer<2>(p, ly, li == 0, li + 1 == L, rows, xq, in, out, wave, col, h);
      else run_layer<kTPW>(p, ly, li == 0, li + 1 == L, rows, xq, in, out, wave, col, h);
    }
    __syncthreads();
    float* sw = in; in = out; out = sw;
  }
  if (L == 0) __syncthreads();                                    // (red_lin / red_fm)

  // 4. the head's sum: the order of mi_sigmoid_ce_head
  float z = 0.f;
  if (tid < kRB && b0 + tid < p.B) {
    if (p.use_linear) {
      float lin = 0.f;
#pragma unroll
      for (int i = 0; i < kParts; ++i) lin += red_lin[i][tid];
      if (nd && p.raw)                                            // canned estimators: added in column order after the categorical sum
        for (int j = 0; j < nd; ++j) lin = lin + __fmul_rn(xq[j], p.dense[p.lin_num_off + j]);
      z = lin + p.dense[p.lin_bias_off];
    }
    if (p.use_fm) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < kParts; ++i) t += red_fm[i][tid];
      z = z + 0.5f * t;
    }
    if (L) z = z + in[tid];                                       // the logits layer's one row
  }
  return z;
}

// the outputs of mi_binary_predictions for request b with logit z (any pointer may be NULL)
__device__ __forceinline__ void write_head(float z, int64_t b, float* logits, float* logistic, float* probabilities,
                                           int64_t* class_ids) {
  if (logits) logits[b] = z;
  const float pr = mi_sigmoid_stable(z);
  if (logistic) logistic[b] = pr;
  if (probabilities) { probabilities[2 * b] = 1.f - pr; probabilities[2 * b + 1] = pr; }
  if (class_ids) class_ids[b] = pr > 0.5f ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void predict_fused_k(const ServeArgs p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ Layer layers[kMaxLayers];
  __shared__ float red_lin[kParts][kRB], red_fm[kParts][kRB];
  const int tid = threadIdx.x;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kRB;
  // (the layer table: compile-time indices into the kernel arguments, runtime indices into LDS afterwards)
#pragma unroll
  for (int i = 0; i < kMaxLayers; ++i)
    if (tid == i) layers[i] = p.l[i];
  const float z = serve_block(p, lds, layers, red_lin, red_fm, b0);
  if (tid < kRB && b0 + tid < p.B) write_head(z, b0 + tid, p.logits, p.logistic, p.probabilities, p.class_ids);
}

__global__ __launch_bounds__(kThreads) void predict_group_k(const ServeArgs* __restrict__ members, int32_t M,
                                                            const int32_t* __restrict__ ids, const float* __restrict__ x_num,
                                                            int64_t B, float* member_logits, int32_t* tickets,
                                                            float* logits, float* logistic, float* probabilities,
                                                            int64_t* class_ids) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ ServeArgs sp;
  __shared__ Layer layers[kMaxLayers];
  __shared__ float red_lin[kParts][kRB], red_fm[kParts][kRB];
  const int tid = threadIdx.x, y = blockIdx.y;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kRB;
  mi_copy_words<kThreads>(&sp, members + y);
  __syncthreads();
  if (tid == 0) { sp.ids = ids; sp.x_num = x_num; sp.B = B; }
  if (tid < kMaxLayers) layers[tid] = sp.l[tid];
  __syncthreads();
  const float z = serve_block(sp, lds, layers, red_lin, red_fm, b0);
  if (tid < kRB && b0 + tid < B) member_logits[static_cast<int64_t>(y) * B + b0 + tid] = z;

  // publish, then draw the ticket: every wave drains its stores, a barrier, lane 0 releases at agent scope and waits
  // again (the fence before the fetch_add, always), relaxed agent-scope fetch_add.  The last of the M arrivers reduces.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                                // (also: every read of red_lin by the head's sum is over)
  int32_t* last = reinterpret_cast<int32_t*>(&red_lin[0][0]);
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int32_t t = __hip_atomic_fetch_add(&tickets[blockIdx.x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool am_last = t == M - 1;
    if (am_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *last = am_last ? 1 : 0;
  }
  __syncthreads();
  if (!*last) return;                                             // nobody waits: the other M - 1 workgroups are done
  if (tid < kRB && b0 + tid < B) {
    const int64_t b = b0 + tid;
    float acc = member_logits[b];
    for (int m = 1; m < M; ++m) acc = acc + member_logits[static_cast<int64_t>(m) * B + b];
    write_head(acc / static_cast<float>(M), b, logits, logistic, probabilities, class_ids);
  }
  if (tid == 0) __hip_atomic_store(&tickets[blockIdx.x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

using mi::unsupported;

constexpr uint64_t kGroupMagic = 0x6d69707265646772ull;         // "mipredgr"

// The model-side checks of mi_predict_fused and the ServeArgs they describe (ids, x_num, B and the outputs are left to the
// caller); lds: the dynamic LDS of a workgroup.  have_ids / have_x / have_out: whether the call brought them.  One function
// for mi_predict_fused and for every member of mi_predict_group_plan: the same checks, the same messages.
int32_t plan_serve(const mi_serve_member_t& m, const int64_t* field_off, int32_t F, int32_t n_numeric, bool have_ids,
                   bool have_x, bool have_out, ServeArgs& a, size_t& lds) {
  const int32_t E = m.E, n_layers = m.n_layers;
  MI_REQUIRE(F >= 0 && n_numeric >= 0 && F + n_numeric >= 1, "predict_fused: F=%d n_numeric=%d (at least one column)", F, n_numeric);
  if (F > kMaxFields) return unsupported("predict_fused: F=%d categorical fields (at most %d)", F, kMaxFields);
  MI_REQUIRE(m.use_linear || m.use_fm || m.use_dnn, "predict_fused: no part of the model is switched on");
  MI_REQUIRE(have_out, "predict_fused: no output requested");
  MI_REQUIRE(m.activation >= 0 && m.activation <= 3, "predict_fused: activation %d", m.activation);
  MI_REQUIRE(!(m.numeric_raw && m.use_fm), "predict_fused: raw numeric columns belong to the models without an FM term");
  const bool emb = (m.use_fm || m.use_dnn) && F > 0;              // the table is read
  const bool num_emb = n_numeric > 0 && !m.numeric_raw;
  if ((emb || num_emb) && (E < 4 || E > 256 || (E & 3)))
    return unsupported("predict_fused: embedding size %d unsupported (multiple of 4 in [4,256])", E);
  MI_REQUIRE(!emb || (m.table && mi::aligned16(m.table)), "predict_fused: table (16-byte aligned)");
  MI_REQUIRE(m.table_stride == 0 || (m.table_stride >= E && (m.table_stride & 3) == 0),
             "predict_fused: table_stride=%lld (0 = E, else >= E and a multiple of 4)", (long long)m.table_stride);
  MI_REQUIRE(F == 0 || (field_off && have_ids), "predict_fused: field_off / ids");
  MI_REQUIRE(n_numeric == 0 || have_x, "predict_fused: x_num");
  MI_REQUIRE(!(m.use_linear && F > 0 && m.wide_fields) || (m.lin_w && m.lin_stride >= 1), "predict_fused: lin_w / lin_stride=%d",
             m.lin_stride);
  MI_REQUIRE(!(m.use_linear || m.use_dnn || num_emb) || m.dense, "predict_fused: dense");
  MI_REQUIRE(!m.use_linear || m.lin_bias_off >= 0, "predict_fused: lin_bias_off");
  MI_REQUIRE(!(m.use_linear && n_numeric) || m.lin_num_off >= 0, "predict_fused: lin_num_off");
  MI_REQUIRE(!num_emb || (m.num_emb_off >= 0 && (m.num_emb_off & 3) == 0 && mi::aligned16(m.dense)),
             "predict_fused: num_emb_off=%lld (a multiple of 4 floats into a 16-byte aligned buffer)", (long long)m.num_emb_off);
  MI_REQUIRE(!(num_emb && !m.use_fm && !m.use_dnn), "predict_fused: numeric embeddings need the FM term or the DNN");
  MI_REQUIRE(m.use_dnn ? n_layers >= 1 : n_layers == 0, "predict_fused: %d layers (a DNN has at least its logits layer)", n_layers);
  if (n_layers > kMaxLayers)
    return unsupported("predict_fused: %d hidden layers (at most %d)", n_layers - 1, kMaxLayers - 1);
  MI_REQUIRE(n_layers == 0 || (m.layer_off && m.widths), "predict_fused: layer_off / widths");
  int wa = 0, wb = 0;                    // widths of the layer outputs in the first / second LDS buffer
  for (int i = 0; i < n_layers; ++i) {
    const int fi = m.widths[i], fo = m.widths[i + 1];
    MI_REQUIRE(fi >= 1 && fo >= 1, "predict_fused: width %d -> %d", fi, fo);
    MI_REQUIRE(i + 1 < n_layers || fo == 1, "predict_fused: the last layer has %d outputs (1 expected)", fo);
    MI_REQUIRE(m.layer_off[2 * i] >= 0 && m.layer_off[2 * i + 1] >= 0, "predict_fused: layer offsets");
    if (fo > kMaxWidth) return unsupported("predict_fused: hidden width %d (at most %d)", fo, kMaxWidth);
    int& w = (i & 1) ? wb : wa;
    if (fo > w) w = fo;
    a.l[i] = Layer{m.layer_off[2 * i], m.layer_off[2 * i + 1], fi, fo};
  }
  if (n_layers) {
    const int64_t d_in = (emb ? static_cast<int64_t>(F) * E : 0) + static_cast<int64_t>(n_numeric) * (m.numeric_raw ? 1 : E);
    MI_REQUIRE(m.widths[0] >= d_in, "predict_fused: widths[0]=%d below the %lld input columns", m.widths[0], (long long)d_in);
  }
  lds = sizeof(float) * kRB * (static_cast<size_t>(F) + wa + wb);
  if (lds + 4096 > kMaxLds) return unsupported("predict_fused: %zu bytes of LDS for F=%d and widths %d / %d", lds, F, wa, wb);
  a.table = emb ? m.table : nullptr; a.lin_w = m.lin_w; a.field_off = field_off; a.dense = m.dense;
  a.ts = m.table_stride ? m.table_stride : E;
  a.lin_bias_off = m.lin_bias_off; a.num_emb_off = m.num_emb_off; a.lin_num_off = m.lin_num_off;
  a.wide_fields = m.use_linear ? m.wide_fields : 0;
  a.F = F; a.E = E; a.nd = n_numeric; a.ls = m.lin_stride; a.act = m.activation; a.n_layers = n_layers;
  a.use_linear = m.use_linear != 0; a.use_fm = m.use_fm != 0 && (emb || num_emb); a.raw = m.numeric_raw != 0;
  a.buf_a = wa * kRB;
  return MI_OK;
}

}  // namespace

extern "C" {

size_t mi_predict_fused_workspace_bytes(int64_t B, int32_t n_layers) {
  (void)B; (void)n_layers;
  return 0;                              // everything between the ids and the predictions stays in LDS and registers
}

int32_t mi_predict_fused(const float* table, int64_t table_stride, const float* lin_w, int32_t lin_stride,
                         const int64_t* field_off, const int32_t* ids, const float* x_num, int64_t B, int32_t F, int32_t E,
                         int32_t n_numeric, const float* dense, const int64_t* layer_off, const int32_t* widths,
                         int32_t n_layers, int32_t activation, int32_t use_linear, int32_t use_fm, int32_t use_dnn,
                         int32_t numeric_raw, int64_t lin_bias_off, int64_t num_emb_off, int64_t lin_num_off,
                         uint64_t wide_fields, float* logits, float* logistic, float* probabilities, int64_t* class_ids,
                         void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  (void)workspace; (void)workspace_bytes;
  MI_REQUIRE(B >= 1, "predict_fused: B=%lld (at least one request)", (long long)B);
  ServeArgs a{};
  size_t lds = 0;
  mi_serve_member_t m{};
  m.table = table; m.table_stride = table_stride; m.lin_w = lin_w; m.lin_stride = lin_stride; m.E = E; m.dense = dense;
  m.layer_off = layer_off; m.widths = widths; m.n_layers = n_layers; m.activation = activation;
  m.use_linear = use_linear; m.use_fm = use_fm; m.use_dnn = use_dnn; m.numeric_raw = numeric_raw;
  m.lin_bias_off = lin_bias_off; m.num_emb_off = num_emb_off; m.lin_num_off = lin_num_off; m.wide_fields = wide_fields;
  const int32_t rc = plan_serve(m, field_off, F, n_numeric, ids != nullptr, x_num != nullptr,
                                logits || logistic || probabilities || class_ids, a, lds);
  if (rc != MI_OK) return rc;
  const int64_t blocks = mi::ceil_div(B, kRB);
  MI_REQUIRE(blocks <= INT32_MAX, "predict_fused: grid too large");
  a.ids = ids; a.x_num = x_num; a.B = B;
  a.logits = logits; a.logistic = logistic; a.probabilities = probabilities; a.class_ids = class_ids;
  const int32_t rl = mi::raise_lds(&predict_fused_k, lds, "predict_fused");
  if (rl != MI_OK) return rl;
  predict_fused_k<<<dim3(static_cast<unsigned>(blocks)), dim3(kThreads), lds, mi::as_stream(stream)>>>(a);
  MI_CHECK_LAUNCH("predict_fused");
  return MI_OK;
}

size_t mi_predict_group_plan_bytes(int32_t n_members) {
  return n_members < 0 ? 0 : sizeof(ServeArgs) * static_cast<size_t>(n_members);
}

int32_t mi_predict_group_plan(const mi_serve_member_t* members, int32_t n_members, int32_t F, int32_t n_numeric,
                              const int64_t* field_off, void* device_table, mi_serve_group_plan_t* plan, mi_stream_t stream) {
  MI_REQUIRE(plan, "predict_group_plan: plan");
  MI_REQUIRE(n_members >= 1, "predict_group_plan: %d members (at least 1)", n_members);
  if (n_members > MI_PREDICT_GROUP_MAX_MEMBERS)
    return unsupported("predict_group_plan: %d members (at most %d in one launch)", n_members, MI_PREDICT_GROUP_MAX_MEMBERS);
  MI_REQUIRE(members, "predict_group_plan: members");
  MI_REQUIRE(device_table && mi::aligned16(device_table),
             "predict_group_plan: device_table (mi_predict_group_plan_bytes bytes of device memory, 16-byte aligned)");
  const size_t need = mi_predict_group_plan_bytes(n_members);
  const std::unique_ptr<ServeArgs[]> tab(new (std::nothrow) ServeArgs[n_members]());
  MI_REQUIRE(tab, "predict_group_plan: out of host memory");
  size_t lds = 0;
  for (int32_t i = 0; i < n_members; ++i) {
    size_t lds_i = 0;
    // (ids, x_num and the outputs belong to the call: mi_predict_group checks them)
    const int32_t rc = plan_serve(members[i], field_off, F, n_numeric, true, true, true, tab[i], lds_i);
    if (rc != MI_OK) {
      mi::member_error("predict_group_plan", i);
      return rc;
    }
    if (lds_i > lds) lds = lds_i;
  }
  const int32_t rc = mi::upload_table(device_table, tab.get(), need, stream, "predict_group_plan");
  if (rc != MI_OK) return rc;
  plan->device_table = device_table; plan->n_members = n_members; plan->F = F; plan->n_numeric = n_numeric;
  plan->lds_bytes = static_cast<uint32_t>(lds); plan->magic = kGroupMagic;
  return MI_OK;
}

int32_t mi_predict_group(const mi_serve_group_plan_t* plan, int32_t n_members, const int32_t* ids, const float* x_num, int64_t B,
                         float* member_logits, int32_t* tickets, float* logits, float* logistic, float* probabilities,
                         int64_t* class_ids, mi_stream_t stream) {
  MI_REQUIRE(plan && plan->magic == kGroupMagic && plan->device_table, "predict_group: plan (not written by mi_predict_group_plan)");
  MI_REQUIRE(n_members == plan->n_members, "predict_group: %d members, the plan has %d", n_members, plan->n_members);
  MI_REQUIRE(n_members >= 1 && n_members <= MI_PREDICT_GROUP_MAX_MEMBERS && plan->lds_bytes + 4096 <= kMaxLds,
             "predict_group: plan (damaged)");
  MI_REQUIRE(B >= 1, "predict_group: B=%lld (at least one request)", (long long)B);
  MI_REQUIRE(ids, "predict_group: ids");
  MI_REQUIRE(plan->n_numeric == 0 || x_num, "predict_group: x_num (the plan has %d numeric columns)", plan->n_numeric);
  MI_REQUIRE(member_logits, "predict_group: member_logits ([M, B], required: the members meet there)");
  MI_REQUIRE(tickets, "predict_group: tickets (int32 [ceil(B / 32)], zero on entry)");
  MI_REQUIRE(logits || logistic || probabilities || class_ids, "predict_group: no output requested");
  const int64_t blocks = mi::ceil_div(B, kRB);
  MI_REQUIRE(blocks <= INT32_MAX, "predict_group: grid too large");
  const int32_t rl = mi::raise_lds(&predict_group_k, plan->lds_bytes, "predict_group");
  if (rl != MI_OK) return rl;
  predict_group_k<<<dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(n_members)), dim3(kThreads), plan->lds_bytes,
                    mi::as_stream(stream)>>>(static_cast<const ServeArgs*>(plan->device_table), n_members, ids, x_num, B,
                                             member_logits, tickets, logits, logistic, probabilities, class_ids);
  MI_CHECK_LAUNCH("predict_group");
  return MI_OK;
}

}  // extern "C"
