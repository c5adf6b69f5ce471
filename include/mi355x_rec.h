/*
 * mi355x_rec.h — C ABI of libmi355x_rec.so, the MI355X (gfx950 / CDNA4) DeepFM / Wide&Deep
 * training hot path.
 *
 * The reference (leotimus/recommender-tensorflow) has no FFI of its own: every FLOP on the path
 * is executed by TensorFlow 1.12 ops that trainers/deep_fm.py:36-125 strings together.  Each entry
 * point below therefore names the reference *call site* whose arithmetic it replaces (file:line
 * relative to the reference root) and, where TensorFlow supplies the semantics implicitly, the
 * SURVEY.md appendix paragraph that restates them.
 *
 * Conventions
 *   - plain C, no exceptions; every entry returns 0 on success or a negative mi_status; the text
 *     of the last failure on the calling thread is mi_last_error().
 *   - the caller owns every buffer.  Device entries take device pointers (allocated by whoever
 *     owns the HIP context — PyTorch in the shipped host) and a hipStream_t passed as void*;
 *     they only enqueue work on that stream and never synchronise, allocate or free.
 *   - scratch space is an explicit caller-sized workspace: ask mi_*_workspace_bytes() first.
 *   - shapes are validated on the host before any launch (a bad shape returns
 *     MI_ERR_INVALID instead of faulting the GPU).
 *   - variables, activations, gradients and results are IEEE fp32, and so is every accumulation; index work is
 *     int32/int64, bit exact.  ONE family of entries feeds the matrix pipe something other than fp32 operands: the
 *     *_planes entries (and the other GEMM entries in gemm mode 1) split each fp32 operand into fp16 high + low parts
 *     (~22 significant bits per row-scaled operand; three exact 16-bit products per fp32 product, the lo*lo term
 *     dropped, fp32 accumulate) — fp32-LEVEL results (row-relative error < 1e-5, enforced in tests/test_hip_planes.py),
 *     not IEEE fp32 products.  mi_set_gemm_mode(0) runs the same GEMMs on the fp32-input MFMA (exact products).
 *   - PROCESS-WIDE STATE.  Two switches are per process, not per call or per model, because the deployment is one
 *     process per GPU running one model: mi_set_gemm_mode (the matrix-pipe path every GEMM entry takes) and
 *     mi_set_step_state (while set, the entries listed there read the step / lr_t / dropout seed term from a device
 *     record instead of from their arguments: hipGraph capture).  A host that drives TWO models from one process must
 *     set the GEMM mode before each model's calls (the shipped host does: engine._forward sets it every step) and
 *     must not capture one model's step while another thread launches the other's — the registered step state would
 *     be read by both.  Everything else (tables, slots, workspaces, streams) is per call.
 */
#ifndef MI355X_REC_H
#define MI355X_REC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mi_stream_t; /* hipStream_t */

enum mi_status {
  MI_OK = 0,
  MI_ERR_INVALID = -1,     /* bad argument / shape / alignment */
  MI_ERR_UNSUPPORTED = -2, /* legal but not built (e.g. embedding size not a multiple of 4 > 256) */
  MI_ERR_LAUNCH = -3,      /* HIP reported an error at launch */
  MI_ERR_WORKSPACE = -4    /* workspace too small */
};

/* ---- library ---------------------------------------------------------------------------- */
int32_t mi_abi_version(void);       /* bumps when a signature changes (currently 21) */
const char* mi_last_error(void);    /* thread-local, never NULL */
const char* mi_build_info(void);    /* "gfx950 hipcc <ver>" */

/* ---- replayable steps (hipGraph) -------------------------------------------------------------------------
 * A captured train step must not carry per-step values in its launch arguments.  While a device-resident step
 * state is registered (process-wide, like the GEMM mode: one process per GPU), the entries below read them from
 * it AT RUN TIME instead of from their scalar arguments:
 *   mi_sparse_apply[_fused]              step <- state->step, hp->lr_t <- state->lr_t
 *   mi_dense_apply                       hp->lr_t <- state->lr_t
 *   mi_sparse_catchup, mi_catchup_gap_keys, mi_catchup_rows_by_gap   step_to <- state->step - 1
 *   mi_dense_fwd[_gathered|_planes], mi_hidden_logits_head_fused   seed <- seed + state->seed_term   (dropout masks differ every step)
 * mi_step_advance (the first node of the captured step): step += 1, lr_t = lr_table[step], seed_term = step * 1000003.
 * Register the state only while capturing; eager calls between replays keep using their arguments. */
typedef struct mi_step_state {
  int32_t step;        /* the step being executed (1-based, as the global step after it) */
  float lr_t;          /* Adam: lr * sqrt(1 - beta2^step) / (1 - beta1^step) */
  uint64_t seed_term;
} mi_step_state_t;
int32_t mi_set_step_state(const mi_step_state_t* device_state);   /* NULL: off */
int32_t mi_step_advance(mi_step_state_t* device_state, const float* lr_table, mi_stream_t stream);

/* ---- (a1) categorical id transforms, host side --------------------------------------------
 * replaces the column constructors of trainers/ml_100k.py:19-35.
 * All integer work; results are bit exact against oracle/fingerprint.py. */

/* FarmHash Fingerprint64 (farmhashna::Hash64) of len bytes — what
 * tf.feature_column.categorical_column_with_hash_bucket applies (ml_100k.py:19,20,29,30). */
uint64_t mi_fingerprint64(const void* data, size_t len);

/* CRC-32C (Castagnoli) of len bytes, continuing from `crc` (0 to start; unmasked) — the checksum TensorFlow's tensor-bundle
 * checkpoints carry per table block and per tensor (the files tf.estimator writes under conf_utils.py:6-10's RunConfig;
 * read and written by mi355x_rec/tf_bundle.py).  Host function. */
uint32_t mi_crc32c(const void* data, size_t len, uint32_t crc);

/* id = Fingerprint64(decimal ASCII of v) mod num_buckets — hash_bucket column with an integer
 * dtype (user_id, item_id: ml_100k.py:19-20). */
int32_t mi_hash_bucket_i64(const int64_t* values, int64_t n, int64_t num_buckets, int32_t* out_ids);

/* id = Fingerprint64(bytes[offsets[i]:offsets[i+1]]) mod num_buckets — string hash_bucket column
 * (occupation, zipcode: ml_100k.py:29-30).  offsets has n+1 entries. */
int32_t mi_hash_bucket_bytes(const uint8_t* bytes, const int64_t* offsets, int64_t n,
                             int64_t num_buckets, int32_t* out_ids);

/* id = number of boundaries <= x (upper_bound) — bucketized_column (ml_100k.py:23-24,33-34). */
int32_t mi_bucketize_f32(const float* values, int64_t n, const float* boundaries,
                         int32_t num_boundaries, int32_t* out_ids);

/* ---- (a2,a3,a5) embedding gather + wide linear reduce + FM second order, forward ------------
 * replaces tf.feature_column.linear_model (deep_fm.py:39), embedding_column + input_layer
 * (deep_fm.py:52-54) and the mf block (deep_fm.py:79-87) with ONE kernel.
 *
 *   row(b,f)      = field_off[f] + ids[b*F+f]                 (fused row-major table, all fields)
 *   concat[b,f,:] = table[row(b,f), :]                        (deep_fm.py:54; mean of one id = row)
 *   sumv[b,:]     = sum_f concat[b,f,:]                       (saved for the backward)
 *   fm[b]         = 0.5 * sum_e( sumv[b,e]^2 - sum_f concat[b,f,e]^2 )   (deep_fm.py:81-87)
 *   lin[b]        = sum_f lin_w[row(b,f)]                     (deep_fm.py:39; bias is added by the head)
 *
 * table [R,E] f32, lin_w [R] f32 (may be NULL: lin not produced), field_off [F] int64 (device),
 * ids [B,F] int32 (device).  Outputs: concat [B,F*E] with leading dimension ld_concat (floats,
 * >= F*E: numeric-embedding columns may follow, deep_fm.py:73), sumv [B,E], fm [B], lin [B]
 * (any of them may be NULL; amax_rows, if not NULL, is an abs-max vector — see mi_gemm_amax_t — that
 * receives max |table[row(b,f), :]| over the rows read, for the MLP's layer-1 GEMMs; with concat == NULL the kernel only READS rows — the form the
 * single-GPU path uses, where layer 1 gathers its operand itself, and the one bench.py prices
 * against the HBM read roofline; with table == NULL only the wide part lin is produced).  E must be a multiple of 4 and <= 256.  Fields must already be
 * in the reference's sorted-by-column-name order.
 * lin_stride: element stride of the wide part's per-row state, here and in mi_gather_rows / mi_sparse_apply* /
 * mi_sparse_catchup / mi_catchup_gap_keys — 1: lin_w, l_slot0, l_slot1 and last_step are four separate arrays;
 * 4: one 16-byte record per row {weight, slot0, slot1, stamp} (lin_w = rec, l_slot0 = rec + 1, l_slot1 = rec + 2,
 * last_step = (int32_t*)rec + 3): a row's wide-part state then costs one memory sector instead of four
 * (round 1's catchup_lin_k fetched 569 MB for 20 MB of state).
 * table_stride (round 4), here and in every entry that takes the embedding table (mi_embed_fm_planes_fwd, mi_gather_rows,
 * mi_dense_fwd_gathered, mi_dense_bwd_weight_gathered, mi_sparse_apply[_fused], mi_sparse_catchup): floats between
 * consecutive rows of table (and of its slot arrays) — 0 or E: [R, E] arrays; 3 E with t_slot0 = table + E, t_slot1 = table +
 * 2 E: ONE record [w | slot0 | slot1] per row (what the shipped host allocates: a row's weights and optimizer state are one
 * contiguous 12 E-byte run — one DRAM page visit per row and direction in the sparse apply and the catch-up instead of
 * three).  A multiple of 4, >= E.
 * Row + weight records: the entries also take a gathered row and its wide weight as ONE record of S floats (a multiple
 * of 4, >= E + 4) [row | weight | pad] per request (and its gradients likewise) — mi_gather_rows(out_stride = S, out_lin = out_rows + E)
 * writes such records, the forward entries read them with table_stride = lin_stride = S, mi_entry_grads_segsum(rows_stride,
 * out_stride) reads and writes them, mi_sparse_apply(grad_stride = S, d_lin = d_rows + E) applies them.  0 everywhere =
 * separate arrays (what the row-sharded step passes). */
int32_t mi_embed_fm_linear_fwd(const float* table, const float* lin_w, const int64_t* field_off,
                               const int32_t* ids, int64_t B, int32_t F, int32_t E,
                               float* concat, int64_t ld_concat, float* sumv, float* fm, float* lin,
                               float* amax_rows, int32_t lin_stride, int64_t table_stride, mi_stream_t stream);

/* The gather with the concat written as fp16 high/low planes (struct mi_planes, below): the operand of
 * the layer-1 GEMMs mi_dense_fwd_planes / mi_dense_bwd_weight_planes.  One exponent per example, from the
 * example's abs-max over all F*E values (the lane group that gathers an example holds all its rows in
 * registers).  Also sumv / fm as above and amax_rows.  E a multiple of 16 and >= 32, F <= 48; the wide part
 * is mi_embed_fm_linear_fwd(table = NULL).
 * x_num [B, n_numeric], tail_cols (0: none): the canned estimators' raw numeric columns (linear_deep.py:32-39 with
 * numeric_column()s in dnn_feature_columns) — the values themselves follow the embedding columns as columns
 * F*E .. F*E + tail_cols of the concat (n_numeric values, then zeros; tail_cols a multiple of 16, at most 4 E), under the
 * example's one exponent: the fp32 concat, its abs-max pass and its split into planes are never made. */
struct mi_planes;
int32_t mi_embed_fm_planes_fwd(const float* table, const int64_t* field_off, const int32_t* ids, int64_t B, int32_t F,
                               int32_t E, float* sumv, float* fm, const struct mi_planes* concat, float* amax_rows,
                               const float* x_num, int32_t n_numeric, int32_t tail_cols, int64_t table_stride, mi_stream_t stream);

/* Owner-side half of the row-sharded path (multi-GPU): out_rows[i,:] = table[rows[i],:],
 * out_lin[i] = lin_w[rows[i] * lin_stride].  rows [n] int32 local row ids; table (with out_rows) or lin_w
 * (with out_lin) may be NULL. */
int32_t mi_gather_rows(const float* table, const float* lin_w, const int32_t* rows, int64_t n,
                       int32_t E, float* out_rows, float* out_lin, int32_t lin_stride, int64_t table_stride, int64_t out_stride, mi_stream_t stream);

/* (a4) numeric embedding, deep_fm.py:62-70: out[b, j*E+e] = x[b,j] * V[j,e], written at
 * concat[b, col0 + j*E + e]; also accumulates into sumv / fm so the FM term sees the numeric
 * fields (deep_fm.py:79 reshapes the concatenated layer), and lin[b] += sum_j x[b,j]*w_num[j]. */
int32_t mi_numeric_embed_fwd(const float* x, const float* V, const float* w_num, int64_t B,
                             int32_t n_d, int32_t E, float* concat, int64_t ld_concat, int64_t col0,
                             float* sumv, float* fm, float* lin, mi_stream_t stream);

/* Numeric columns of the canned estimators (tf.feature_column.numeric_column handed to
 * DNNLinearCombinedClassifier, trainers/linear_deep.py:32-39): input_layer takes
 * the VALUE as a column of the concat, linear_model multiplies it by a [1,1] weight.
 *   concat[b, col0 + j] = x[b,j] for j < n_d, 0 for n_d <= j < n_cols   (zero pad: whole k-tiles for layer 1)
 *   lin[b] += sum_j x[b,j] * w_num[j]        (ascending j, after the categorical sum; bias added by the head)
 * concat or lin may be NULL.  Backward: dw_num[j] = sum_b d_logit_lin[b] * x[b,j] (two-stage, fixed order). */
int32_t mi_numeric_raw_fwd(const float* x, const float* w_num, int64_t B, int32_t n_d, float* concat,
                           int64_t ld_concat, int64_t col0, int32_t n_cols, float* lin, mi_stream_t stream);
size_t mi_numeric_raw_bwd_workspace_bytes(int64_t B, int32_t n_d);
int32_t mi_numeric_raw_bwd(const float* x, const float* d_logit_lin, int64_t B, int32_t n_d, float* dw_num,
                           void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- (a2,a3,a5) backward: per-entry row gradients -------------------------------------------
 * d_rows[p(b,f), :] = d_concat[b,f,:] + d_logit_fm[b] * (sumv[b,:] - concat[b,f,:])
 * d_lin [p(b,f)]    = d_logit_lin[b]
 * (gradient of deep_fm.py:54,81-87,39 w.r.t. the gathered rows; TF: IndexedSlices values).
 * pos [B*F] int32 gives the destination slot p(b,f) (NULL = identity b*F+f); the sharded path
 * uses it to write straight into all-to-all send order.  d_concat may be NULL (no DNN),
 * d_logit_fm may be NULL (no FM), d_lin/d_logit_lin may be NULL (no linear part).  Instead of concat
 * the gathered rows may be given in slot order (rows [n,E], row of (b,f) at slot pos[b*F+f]: the
 * receive buffer of the row exchange, when the concat was never materialised). */
int32_t mi_embed_fm_linear_bwd(const float* d_concat, int64_t ld_dconcat, const float* concat,
                               int64_t ld_concat, const float* rows, const float* sumv, const float* d_logit_fm,
                               const float* d_logit_lin, const int32_t* pos, int64_t B, int32_t F,
                               int32_t E, float* d_rows, float* d_lin, mi_stream_t stream);

/* Requester-side half of the sparse "reduce-scatter" (multi-GPU): the entries of a chunk that asked for the
 * same row are summed BEFORE the gradient all-to-all, so one gradient row per distinct request travels.
 * For distinct requests u in [u_begin, u_begin + u_count) (segments of mi_sort_unique_rows over the request
 * keys): out_rows[u,:] = sum over the segment's entries e = (b, f), in ascending entry order, of
 *   d_concat[b - b0, f*E:(f+1)*E] + d_logit_fm[b - b0] * (sumv[b - b0,:] - rows[u,:])
 * and out_lin[u] = sum of d_logit_lin[b - b0]; rows [*,E] = the exchange's receive buffer (slot u), the
 * per-example arrays belong to examples b0.. (one chunk).  Segments longer than 48 entries are summed by a
 * workgroup in fixed slices, like mi_sparse_apply's.
 * out_row0 (0 <= out_row0 <= u_begin): the request that row 0 of out_rows / out_lin holds — request u is written at
 * row u - out_row0.  0: the out buffers are the whole send buffer; u_begin: they start at this range (a rank's
 * requests to ITSELF are summed straight into the buffer its own sparse apply reads, no exchange in between). */
int32_t mi_entry_grads_segsum(const float* rows, const int32_t* seg_start, const int32_t* sorted_entry, int64_t u_begin,
                              int64_t u_count, const float* d_concat, int64_t ld_dconcat, const float* sumv,
                              const float* d_logit_fm, const float* d_logit_lin, int64_t b0, int32_t F, int32_t E,
                              float* out_rows, float* out_lin, int64_t out_row0, int64_t rows_stride, int64_t out_stride, mi_stream_t stream);

/* (a4) backward of the numeric embedding: dV[j,e] = sum_b x[b,j]*g[b,j,e] with
 * g = d_concat + d_logit_fm*(sumv - concat);  dw_num[j] = sum_b d_logit_lin[b]*x[b,j].
 * Deterministic two-stage reduction; workspace from mi_numeric_embed_bwd_workspace_bytes. */
size_t mi_numeric_embed_bwd_workspace_bytes(int64_t B, int32_t n_d, int32_t E);
int32_t mi_numeric_embed_bwd(const float* x, const float* d_concat, int64_t ld_dconcat,
                             const float* concat, int64_t ld_concat, int64_t col0, const float* sumv,
                             const float* d_logit_fm, const float* d_logit_lin, int64_t B,
                             int32_t n_d, int32_t E, float* dV, float* dw_num, void* workspace,
                             size_t workspace_bytes, mi_stream_t stream);

/* ---- row bookkeeping for sparse updates -----------------------------------------------------
 * Sorts the n requested rows (stable LSD radix sort, key = row, payload = entry index) and
 * compacts duplicates — the device analogue of TF's unique + unsorted_segment_sum that
 * precedes every sparse optimizer apply.  Outputs (all device):
 *   sorted_entry [n]   entry index (into rows / d_rows) in ascending (row, entry) order
 *   uniq_rows    [n]   first U slots hold the distinct rows in ascending order
 *   seg_start    [n+1] segment u covers sorted_entry[seg_start[u] .. seg_start[u+1])
 *   num_uniq     [1]   U (int32) — stays on the device; later kernels read it there
 * num_rows_total bounds the key range (picks the number of radix passes).
 * With uniq_rows == NULL only the stable sort permutation is produced (sorted_entry); seg_start and
 * num_uniq are then ignored. */
size_t mi_sort_unique_workspace_bytes(int64_t n);
int32_t mi_sort_unique_rows(const int32_t* rows, int64_t n, int64_t num_rows_total,
                            int32_t* sorted_entry, int32_t* uniq_rows, int32_t* seg_start,
                            int32_t* num_uniq, void* workspace, size_t workspace_bytes,
                            mi_stream_t stream);

/* mi_sort_unique_rows + mi_segment_slots in one entry (round 5): additionally slot_of_entry [n] = the segment u of every entry
 * (the row-sharded step's "slot of my row in the receive buffer"), written by the compaction as it goes — the separate
 * binary-search entry costs 112 us at 1.7 M entries. */
int32_t mi_sort_unique_rows_slots(const int32_t* rows, int64_t n, int64_t num_rows_total,
                                  int32_t* sorted_entry, int32_t* uniq_rows, int32_t* seg_start,
                                  int32_t* num_uniq, int32_t* slot_of_entry, void* workspace, size_t workspace_bytes,
                                  mi_stream_t stream);

/* mi_global_rows + mi_sort_unique_rows in one entry for the single-GPU step: ids [B][F] (local ids, field f's rows are
 * field_off[f] + id: disjoint ranges in ascending field order), max_vocab >= every field's id range, 0 < max_vocab <= 2^30
 * (above it the call is refused, in either form; every admitted max_vocab is sorted by both forms).  Same outputs,
 * bit for bit (equal rows keep ascending example order): sorted_entry [B*F] (entry = b * F + f), uniq_rows (global
 * rows), seg_start, num_uniq.  Every field's ids are sorted on their own, so the radix passes cover the bits of
 * max_vocab, not of the whole table.  B a multiple of 4096, F <= 64 (anything else: the two-entry form).
 * workspace: mi_sort_unique_fields_workspace_bytes(B, F), 256-byte aligned.
 * beside (round 5, ABI 21): how the work is cut into launches — same results either way.  0: the stream has the GPU to itself
 * (a step that was not told its next batch sorts at its head): ONE launch per radix pass and one for the compaction, the
 * tiles of a field exchanging their digit counts inside the launch (5 launches, 130 us at config 3 against 145).  1: the
 * call runs on a side stream BESIDE the step's bandwidth-bound kernels (the next batch's sort, beside this batch's Adam
 * catch-up): short launches that hold no resources while they wait (9 at config 3, 113 us) — beside the catch-up the fused
 * form's resident, waiting workgroups cost the step 0.03 ms more than they save (profiles/r05_sort_and_side_streams.md). */
size_t mi_sort_unique_fields_workspace_bytes(int64_t B, int32_t F);
int32_t mi_sort_unique_fields(const int32_t* ids, const int64_t* field_off, int64_t B, int32_t F, int64_t max_vocab,
                              int32_t* sorted_entry, int32_t* uniq_rows, int32_t* seg_start, int32_t* num_uniq,
                              void* workspace, size_t workspace_bytes, int32_t beside, mi_stream_t stream);

/* Routing helpers of the row-sharded multi-GPU path (row r lives on rank r % world as local row
 * r / world; the reference's own multi-worker mode is TF's parameter-server placement of whole
 * variables, distributed.md:58-82 — see DESIGN.md "Multi-GPU").
 *   mi_shard_keys     : keys[i] = ((i / entries_per_chunk) * world + pos(rows[i] % world)) * rows_per_rank + rows[i] / world
 *                       (chunk-major request key of a pipelined step; entries_per_chunk == 0: one chunk).  n need not be
 *                       a multiple of entries_per_chunk: the last of the ceil(n / entries_per_chunk) chunks may be short.
 *                       chunks * world * rows_per_rank <= INT32_MAX (the key is an int32), else the call is refused.
 *                       pos: the owner's place in the send order — the rank itself (self_rank = -1), or, with
 *                       self_rank >= 0, the other ranks in rank order and the asking rank LAST (o -> o below
 *                       self_rank, o - 1 above, world - 1 for self_rank): a rank's requests to itself then end every
 *                       chunk's run, outside the part an all-to-all with a zero self split ships.
 *                       mi_sort_unique_rows of the keys orders the entries by (chunk, owner, row); its unique
 *                       keys are the DISTINCT rows each chunk needs from each owner — what travels.
 *   mi_route_requests : per distinct request u < *num_uniq: send_rows[u] = owner-local row;
 *                       counts[chunk * world + owner] = number of distinct requests of that group (device;
 *                       zeroed here) — the all-to-all split sizes
 *   mi_segment_slots  : slot_of_entry[e] = u, the distinct request entry e belongs to (the received row's
 *                       slot in the exchange buffer)
 *   mi_gather_u32     : out[i] = src[idx[i]] for 4-byte elements (int32 ids or f32 values) */
int32_t mi_shard_keys(const int32_t* rows, int64_t n, int32_t world, int64_t entries_per_chunk, int64_t rows_per_rank,
                      int32_t self_rank, int32_t* keys, mi_stream_t stream);
int32_t mi_route_requests(const int32_t* uniq_keys, const int32_t* num_uniq, int64_t n_max, int64_t rows_per_rank,
                          int32_t n_groups, int32_t* send_rows, int32_t* counts, mi_stream_t stream);
int32_t mi_segment_slots(const int32_t* seg_start, const int32_t* sorted_entry, const int32_t* num_uniq, int64_t n,
                         int32_t* slot_of_entry, mi_stream_t stream);
int32_t mi_gather_u32(const void* src, const int32_t* idx, int64_t n, void* out, mi_stream_t stream);

/* rows[b*F+f] = field_off[f] + ids[b*F+f]  (int32 global row per entry) */
int32_t mi_global_rows(const int32_t* ids, const int64_t* field_off, int64_t B, int32_t F,
                       int32_t* rows, mi_stream_t stream);

/* ---- (a9) optimizers ------------------------------------------------------------------------
 * get_optimizer (model_utils.py:57-66) -> tf.train.{Adam,Adagrad,Ftrl,RMSProp,GradientDescent}
 * Optimizer(learning_rate), applied by head.create_estimator_spec (deep_fm.py:119-125).
 * SURVEY Appendix A.6/A.7 restate the TF-1.12 update rules the kernels follow op for op
 * (compiled with -ffp-contract=off so the fp32 sequence equals the oracle's). */

enum mi_optimizer {
  MI_OPT_ADAM = 0,     /* tf.train.AdamOptimizer: beta1 .9 beta2 .999 eps 1e-8 */
  MI_OPT_ADAGRAD = 1,  /* tf.train.AdagradOptimizer: initial_accumulator_value .1 */
  MI_OPT_FTRL = 2,     /* tf.train.FtrlOptimizer: lr_power -.5, init accum .1, l1=l2=0 */
  MI_OPT_RMSPROP = 3,  /* tf.train.RMSPropOptimizer: decay .9 momentum 0 eps 1e-10 */
  MI_OPT_SGD = 4       /* tf.train.GradientDescentOptimizer */
};

typedef struct mi_opt_hparams {
  int32_t kind;      /* enum mi_optimizer */
  float lr;          /* learning_rate as given to the TF constructor */
  float beta1, beta2, epsilon;          /* Adam */
  float lr_t;        /* Adam: lr*sqrt(1-beta2^t)/(1-beta1^t) for THIS step, computed by the host in fp32 */
  float decay, momentum;                /* RMSProp */
  float lr_power, l1, l2;               /* Ftrl */
} mi_opt_hparams;

/* Dense apply over a flat parameter buffer (all MLP kernels/biases, numeric embeddings, linear
 * bias live in one buffer).  slot0/slot1: Adam m,v | Adagrad accum,- | Ftrl accum,linear |
 * RMSProp ms,mom | SGD -,-.  Fused ApplyAdam / ApplyAdagrad / ApplyFtrl / ApplyRMSProp /
 * ApplyGradientDescent semantics. */
/* y[i] += alpha * x[i]: dense-gradient accumulation over the chunks of a pipelined multi-GPU step */
int32_t mi_axpy(float* y, const float* x, int64_t n, float alpha, mi_stream_t stream);

int32_t mi_dense_apply(float* param, float* slot0, float* slot1, const float* grad, int64_t n,
                       const mi_opt_hparams* hp, mi_stream_t stream);

/* Sparse apply on the U distinct rows found by mi_sort_unique_rows: segment-sums the entry
 * gradients in ascending entry order (== TF's unsorted_segment_sum order on CPU) for every segment of at most 48
 * entries; a longer segment of c entries is cut into G slices of ceil(c / G) consecutive entries, each summed in
 * ascending order, and the slice sums are added in slice order (a fixed order: results are reproducible; it differs
 * from the one-pass order in fp32 association only).  G = 256 / LPR with LPR = the smallest power of two >= E / 4, and
 * G = 256 in a call without the table (lin_w alone) — here, in mi_sparse_apply_fused and in mi_entry_grads_segsum
 * (there: without out_rows).  tests/sparse_cases.py restates both orders; tests/test_hip_sparse_sums.py holds the
 * entries to them bit for bit and to fp64 within (c + 3) 2^-24 sum |terms|.  Then applies
 * the optimizer's sparse rule to table row r (width E) and, when lin_w != NULL, to lin_w[r]
 * (width 1) with d_lin.  For Adam the rule is TF's dense-equivalent one: see mi_sparse_catchup.
 * last_step[r] is set to step.  slot arrays mirror the parameter arrays' shapes. */
int32_t mi_sparse_apply(float* table, float* t_slot0, float* t_slot1, float* lin_w, float* l_slot0,
                        float* l_slot1, int32_t* last_step, const int32_t* uniq_rows,
                        const int32_t* seg_start, const int32_t* sorted_entry,
                        const int32_t* num_uniq, int64_t n_max, const float* d_rows,
                        const float* d_lin, int32_t E, int32_t step, const mi_opt_hparams* hp,
                        int32_t lin_stride, int64_t table_stride, int64_t grad_stride, mi_stream_t stream);

/* Single-GPU form of mi_sparse_apply with mi_embed_fm_linear_bwd folded in: the gradient of entry
 * e = (b, f) = (e / F, e % F) is rebuilt inside the kernel as
 *   d_concat[b, f*E:(f+1)*E] + d_logit_fm[b] * (sumv[b,:] - w)     (w = the row itself, not yet updated;
 *   equals the concat slice the forward used)  and  d_logit_lin[b] for the linear weight,
 * so the [B*F, E] per-entry gradient matrix is never written.  Same summation order, same bits.
 * (sumv == NULL with d_logit_fm set: d_concat already carries d_logit_fm * sumv; the kernel subtracts d_logit_fm * row only.) */
int32_t mi_sparse_apply_fused(float* table, float* t_slot0, float* t_slot1, float* lin_w, float* l_slot0,
                              float* l_slot1, int32_t* last_step, const int32_t* uniq_rows,
                              const int32_t* seg_start, const int32_t* sorted_entry, const int32_t* num_uniq,
                              int64_t n_max, const float* d_concat, int64_t ld_dconcat, const float* sumv,
                              const float* d_logit_fm, const float* d_logit_lin, int32_t F, int32_t E,
                              int32_t step, const mi_opt_hparams* hp, int32_t lin_stride, int64_t table_stride, mi_stream_t stream);

/* TF-1.12 AdamOptimizer._apply_sparse decays m and v of EVERY row and moves EVERY row each step
 * (SURVEY Appendix A.6).  Instead of sweeping the table, rows carry last_step[r] and are brought
 * up to date lazily: for s in (last_step[r], step_to]: m*=b1; v*=b2; w -= lr_t[s]*m/(sqrt(v)+eps)
 * — the same fp32 op sequence as the sweep, hence the same bits.  lr_table[s] (device, f32) holds
 * lr_t of step s.  Runs on the U distinct rows about to be gathered (step_to = step-1), or on all
 * rows (uniq_rows == NULL, n_max = R) before evaluation / checkpoint.
 * flags: any of MI_CATCHUP_DEFER_SLOTS | MI_CATCHUP_BOUNDED | MI_CATCHUP_KEEP_STAMPS (0 = none), or exactly
 * MI_CATCHUP_LOCAL_ORDER | MI_CATCHUP_BOUNDED | MI_CATCHUP_DEFER_SLOTS.
 * MI_CATCHUP_DEFER_SLOTS (with uniq_rows): only w is written; m, v and last_step keep their old values and
 * the mi_sparse_apply[_fused] of the same step — which reads and writes m, v anyway and MUST then be
 * given last_step — decays them from the old stamp (same multiply chain, same bits).  Saves a third
 * of this kernel's HBM traffic; every row passed here must be applied in the same step.
 * MI_CATCHUP_BOUNDED: the replay with a stated error bound instead of TF's bits (the parity bar is 1e-5 on the
 * logits, not bit equality): m_j and lr_t[s] * m_j are still the reference's chain, bit for bit; sqrt(v_j) is taken as
 * sqrtf(v_0) * beta2^(j/2) (a per-row scalar chain with a two-float multiplier) and the division as a reciprocal good to
 * 1 ulp (v_rcp_f32 for the wide part; for the rows one carried from step to step and corrected against each denominator),
 * w is rounded once per step like the reference's.  Every replayed update is within a few 2^-24 (relative) of the
 * reference's, i.e. ~1e-10 |w|.  Enforced against the literal sweep after 150-200 replayed steps, for EVERY variable:
 * |w - w_sweep| <= 3 ulp(w) + 2e-6 * sum_j |t_j| (t_j: the replayed updates) — and in distribution >= 95 % of the variables
 * bit-identical, >= 98 % within 1e-7 relative (measured 96.7 % / 98.7 %; a 1-ulp difference alone is up to 1.19e-7, so
 * "1e-7 for every variable" is NOT claimed): tests/test_hip_kernels.py::test_bounded_catchup_stays_within_its_bound_of_the_sweep.  m, v and the
 * stamps are written exactly as in the exact mode.  7 packed VALU operations per element and step (no transcendental)
 * instead of 16 + 2, and no range conditions on the state (v = 0, denormal m, any gap).  The bound is a statement about the
 * HYPERPARAMETERS, though: the bounded form runs where mi_catchup_bounded_runs(beta1, beta2, epsilon) is 1, that is for
 * 1e-30 <= epsilon <= 1e30, 0 < beta2 <= 1, beta1 >= 0, q = beta1 / sqrt(beta2) < 1 and
 *   (8 + 2.5 / (1 - q)) * 2^-24 + (1 - sqrt(beta2))^3 <= 2e-6
 * (the per-step error terms weighted over a replay whose updates shrink by q per step, plus the carried reciprocal's
 * third-order term: csrc/optim.hip, catchup_bounded_runs).  TF's defaults are inside (beta1 up to 0.9017 at beta2 = 0.999;
 * beta1 = 0.5 down to beta2 = 0.98); beta1 = 0.9 with beta2 <= 0.99, or beta1 = 0.99, are not.  Outside that region the
 * flag is IGNORED and the exact form runs — the sweep's bits, error 0 — so the bound above holds wherever the entry
 * accepts the flag (tests/test_hip_optimizer_hparams.py).
 * MI_CATCHUP_KEEP_STAMPS: the rows' stamps are left as they are (m, v ARE written) — for a model whose tables and wide part
 * follow two different Adam optimizers (two lr_t tables: two calls; the first must not move the stamps the second reads).
 * MI_CATCHUP_LOCAL_ORDER (only together with MI_CATCHUP_BOUNDED | MI_CATCHUP_DEFER_SLOTS, uniq_rows and table; lin_w or not;
 * anything else: MI_ERR_INVALID before any launch; so are hyperparameters for which mi_catchup_bounded_runs is 0 — this form
 * has no exact counterpart to fall back to, the caller runs the ordinary sequence instead): the train step's catch-up in ONE launch.  uniq_rows comes in the
 * sort's row order, NOT ordered by staleness: every workgroup orders windows of up to mi_catchup_local_chunk_rows() of its rows
 * by staleness in LDS (within 1-2 % of the replayed steps per wave of the global order of mi_catchup_rows_by_gap, which
 * is then not needed), replays the wide part's scalars from the very {w, m, v, stamp} records it reads the stamps from
 * (the wide part's own kernel is not launched) and then the rows.  The results are, bit for bit, those of
 * mi_catchup_rows_by_gap + this entry with the wide part alone + this entry with the rows alone: the per-row code is the same. */
enum mi_catchup_flags { MI_CATCHUP_DEFER_SLOTS = 1, MI_CATCHUP_BOUNDED = 2, MI_CATCHUP_KEEP_STAMPS = 4, MI_CATCHUP_LOCAL_ORDER = 8 };
/* The shape of an MI_CATCHUP_LOCAL_ORDER launch (host-side queries): the largest window a workgroup orders, and for a call
 * with n_max slots of which num_uniq hold rows plan[0..2] = {workgroups, chunks per workgroup, rows per chunk}: workgroup g
 * takes the chunks g, g + workgroups, ... of the list; the last chunks may be short or empty. */
int32_t mi_catchup_local_chunk_rows(void);
/* 1 where mi_sparse_catchup runs the bounded form when MI_CATCHUP_BOUNDED is set, 0 where it ignores the flag (and refuses
 * MI_CATCHUP_LOCAL_ORDER): the one definition of the region, for callers that choose between the two sequences (host-side query). */
int32_t mi_catchup_bounded_runs(float beta1, float beta2, float epsilon);
int32_t mi_catchup_local_plan(int64_t n_max, int64_t num_uniq, int64_t* plan);
/* keys[u] = how many steps row uniq_rows[u] will be replayed over by mi_sparse_catchup(step_to) (0..62,
 * clamped), 63 for the slots u >= *num_uniq.  Sorting the rows by it (mi_sort_unique_rows with
 * key_range 64, then mi_gather_u32 of uniq_rows through the permutation) groups rows of equal
 * staleness, which halves the catch-up's divergence; the valid rows stay in front. */
int32_t mi_catchup_gap_keys(const int32_t* uniq_rows, const int32_t* num_uniq, const int32_t* last_step, int64_t n_max,
                            int32_t step_to, int32_t* keys, int32_t lin_stride, mi_stream_t stream);

/* The three steps above in one entry: rows_out[0 .. *num_uniq) = uniq_rows stably sorted by that key (slots past
 * *num_uniq: unspecified), with the key computed inside the sort's histogram kernel and the row ids carried as the
 * sort's values — two launches fewer than mi_catchup_gap_keys + mi_sort_unique_rows + mi_gather_u32.
 * workspace: mi_sort_unique_workspace_bytes(n_max), 256-byte aligned. */
int32_t mi_catchup_rows_by_gap(const int32_t* uniq_rows, const int32_t* num_uniq, const int32_t* last_step, int64_t n_max,
                               int32_t step_to, int32_t lin_stride, int32_t* rows_out, void* workspace,
                               size_t workspace_bytes, mi_stream_t stream);


/* Self-test of the catch-up's fast square root (no reference analogue; the exactness claim above rests on it): for the
 * `count` fp32 bit patterns from first_bits on, mismatches[0] += how many give different bits in the replay loop's
 * in-range sqrt (v_rsq_f32 + coupled Newton step + residual correction) than in hipcc's correctly rounded sqrtf,
 * mismatches[1] += the same for the v_sqrt_f32 + one-ulp-test form.  mismatches: 2 x uint64 on the device, zeroed by the
 * caller.  The fast loop is only entered with v in [2^-93, 2^20]; the test sweeps [2^-100, 2^24] and demands 0. */
int32_t mi_selftest_sqrt(uint32_t first_bits, int64_t count, uint64_t* mismatches, mi_stream_t stream);

/* Self-test of the GEMM epilogues' division by a host-known constant (tf.nn.dropout divides by keep_prob: deep_fm.py:102-103;
 * no reference analogue: the claim that the 3-instruction form q = x r; e = fma(-d, q, x); fma(e, r, q) with r = RN(1 / d)
 * returns the bits of x / d rests on it): for the `count` fp32 bit patterns x from first_bits on, out[0] += how many with
 * 2^-100 <= |x| <= 2^100 give different bits than '/', out[1] += how many of all of them do (below 2^-100 the residual of a
 * quotient is not exactly representable any more, above 2^100 x r can overflow where x / d does not, and an infinite x gives
 * inf - inf).  out: 2 x uint64 on the device, zeroed by the caller.  The test sweeps all 2^32 patterns for a set of dropout
 * rates and demands out[0] == 0. */
int32_t mi_selftest_div(float d, uint32_t first_bits, int64_t count, uint64_t* out, mi_stream_t stream);

int32_t mi_sparse_catchup(float* table, float* t_m, float* t_v, float* lin_w, float* l_m, float* l_v,
                          int32_t* last_step, const int32_t* uniq_rows, const int32_t* num_uniq,
                          int64_t n_max, int32_t E, int32_t step_to, const float* lr_table,
                          float beta1, float beta2, float epsilon, int32_t flags, int32_t lin_stride,
                          int64_t table_stride, mi_stream_t stream);

/* ---- (a6) the [hidden_units] MLP: fp32 GEMMs on the matrix cores with fused epilogues -----------
 * replaces tf.layers.dense / tf.layers.dropout (deep_fm.py:98-108).  Row-major everywhere.
 * fp32 in, fp32 accumulate, fp32 out; error at the level of an fp32 GEMM (the 1e-5 logit bar). */

/* Matrix-pipe path of the GEMMs below (process-wide switch):
 *   1 (default) 16-bit operand split.  On CDNA4 the fp32-input MFMA runs at 1/16 of the f16/bf16
 *      rate; a product of two 16-bit floats is exact in fp32 and the MFMA accumulates in fp32.
 *      - "f16x2", mi_dense_bwd_weight[_gathered] only, when the call carries both operands' abs-max
 *        (mi_gemm_amax_t): each operand is scaled by ONE power of two (largest magnitude -> [2^14, 2^15))
 *        and split into fp16 high + low parts; three products per k-step (dropped terms <= 2^-21 |ab|).
 *        A matrix-wide scale loses the low bits of rows far below the matrix abs-max — harmless where the
 *        reduction runs over those rows (the weight gradient), not for a forward pass or a data gradient,
 *        whose per-row form is mi_dense_fwd_planes / mi_dense_bwd_data_planes;
 *      - "bf16x3" otherwise: three bf16 parts, six products (dropped <= 3*2^-24 |ab|), any input, no scale.
 *      Both measure the same max error against fp64 as the fp32-input MFMA on the layer shapes.
 *   0 "fp32": v_mfma_f32_32x32x2_f32 (exact fp32 products).
 * Operands that cannot be read as float4 (e.g. the N = 1 logits layer) always take path 0. */
int32_t mi_set_gemm_mode(int32_t mode);
int32_t mi_get_gemm_mode(void);

/* Abs-max vectors.  An abs-max "scalar" is MI_AMAX_SLOTS floats in device memory whose largest entry
 * is the value (producers spread their atomic max over the slots); zero it (hipMemsetAsync) before
 * the producer runs.  a / b: abs-max of the first / second matrix operand of the call, or an upper
 * bound of it (an under-estimate overflows fp16).  out: receives max |result| — every GEMM epilogue
 * can emit it, so the next layer's operand arrives with its abs-max already known.  A NULL struct, or
 * a NULL a or b, selects the bf16x3 split; out may always be NULL. */
#define MI_AMAX_SLOTS 64
typedef struct mi_gemm_amax {
  const float* a;
  const float* b;
  float* out;
} mi_gemm_amax_t;

/* amax_out[slot] = max(amax_out[slot], max_i |x[i]|) for buffers no kernel here produced (weights
 * after the optimizer step, a concat received from an all-to-all). */
int32_t mi_absmax(const float* x, int64_t n, float* amax_out, mi_stream_t stream);

/* Y[M,N] = act( X[M,K] * W[K,N] + bias[N] ); `relu` selects the activation of tf.layers.dense (deep_fm.py:22,100:
 * params["activation"], default tf.nn.relu): 0 none, 1 relu, 2 sigmoid, 3 tanh.  If keep_prob < 1 the
 * TRAIN-mode dropout of deep_fm.py:102-103 is applied after the activation with a counter-based
 * mask (seed, layer, element index): survivors scaled by 1/keep_prob. */
int32_t mi_dense_fwd(const float* X, int64_t ldx, const float* W, const float* bias, float* Y,
                     int64_t ldy, int64_t M, int32_t N, int32_t K, int32_t relu, float keep_prob,
                     uint64_t seed, const mi_gemm_amax_t* amax, mi_stream_t stream);

/* Layer 1 with the input_layer concat (deep_fm.py:54) read IN PLACE from the embedding table:
 * X[b, f*E + e] = table[field_off[f] + ids[b*F+f], e], K = F*E.  The GEMM's A operand is gathered
 * row by row (ids are fetched one k-tile ahead of the rows), so the [M, F*E] concat is never
 * written to or re-read from HBM.  Otherwise identical to mi_dense_fwd / mi_dense_bwd_weight. */
int32_t mi_dense_fwd_gathered(const float* table, const int64_t* field_off, const int32_t* ids, int32_t F,
                              int32_t E, const float* W, const float* bias, float* Y, int64_t ldy, int64_t M,
                              int32_t N, int32_t relu, float keep_prob, uint64_t seed,
                              const mi_gemm_amax_t* amax, int64_t table_stride, mi_stream_t stream);
int32_t mi_dense_bwd_weight_gathered(const float* table, const int64_t* field_off, const int32_t* ids, int32_t F,
                                     int32_t E, const float* dY, int64_t lddy, float* dW, float* db, int64_t M,
                                     int32_t N, void* workspace, size_t workspace_bytes,
                                     const mi_gemm_amax_t* amax, int64_t table_stride, mi_stream_t stream);

/* dX[M,K] = (dY[M,N] * W[K,N]^T) .* mask.  When Xact != NULL (the previous layer's stored
 * post-relu, post-dropout output) mask = (Xact > 0) / keep_prob — a unit with Xact > 0 was both
 * relu-active and kept, every other unit gets gradient 0 — so dX is the gradient w.r.t. the
 * previous layer's PRE-activation, ready to be that layer's dY.
 * activation (as mi_dense_fwd's): for sigmoid / tanh / none the factor is act'(pre) expressed through the stored
 * output (y (1 - y), 1 - y^2, 1) divided by keep_prob; with dropout a stored output that is exactly 0 counts
 * as dropped. */
int32_t mi_dense_bwd_data(const float* dY, int64_t lddy, const float* W, const float* Xact,
                          int64_t ldxa, float* dX, int64_t lddx, int64_t M, int32_t N, int32_t K,
                          float keep_prob, int32_t activation, const mi_gemm_amax_t* amax, mi_stream_t stream);

/* dW[K,N] = X[M,K]^T * dY[M,N], db[N] = column sums of dY.  Split-K over M with a
 * fixed-order slab reduction (bitwise reproducible). */
size_t mi_dense_bwd_weight_workspace_bytes(int64_t M, int32_t N, int32_t K);
int32_t mi_dense_bwd_weight(const float* X, int64_t ldx, const float* dY, int64_t lddy, float* dW,
                            float* db, int64_t M, int32_t N, int32_t K, void* workspace,
                            size_t workspace_bytes, const mi_gemm_amax_t* amax, mi_stream_t stream);

/* ---- (a6) the same layers with operands held as pre-split 16-bit planes ------------------------------
 * A "planes" matrix [rows][K] stores x * 2^s_r = hi + lo (fp16 high and low parts, RNE) with one power-
 * of-two exponent s_r per row, chosen from the row's abs-max (-> [2^14, 2^15)): ~22 significant bits
 * relative to the ROW's largest element, whatever the spread between rows.  Memory layout, k-block major:
 * for every block of 16 columns, all rows back to back, 64 bytes per row (16 x hi then 16 x lo); block j
 * starts at data + j * blk_stride (blk_stride >= 64 * rows, a multiple of 64; data 16-byte aligned; columns
 * K..ceil16(K) are zero).  The 16-k tile of a range of rows is one contiguous run of full cache lines.
 * Producers: mi_split_rows (fp32 -> planes; the weights once per step, W itself for the data gradient and
 * W transposed for the forward pass), the epilogues of the two GEMMs below (the next layer's operand never
 * exists in fp32) and mi_embed_fm_planes_fwd (the input_layer concat).  The GEMMs run three f16 MFMA
 * products per k-step (hi*hi, hi*lo, lo*hi; fp32 accumulate) fed by LDS-DMA with no arithmetic in the loop;
 * row exponents are undone exactly in the epilogue.  Shapes: N and K multiples of 16; a planes result needs
 * its width <= 512 (one workgroup then owns whole rows and knows their abs-max) — otherwise take the fp32
 * result and mi_split_rows, or the any-shape entries above. */
typedef struct mi_planes {
  void* data;          /* [ceil16(K)/16][blk_stride bytes]: row r of block j at data + j*blk_stride + 64*r */
  int32_t* row_exp;    /* [rows] s_r */
  int64_t blk_stride;  /* bytes between consecutive 16-column blocks */
} mi_planes_t;

size_t mi_planes_bytes(int64_t rows, int32_t K);   /* size of data with blk_stride = 64 * rows */

/* out row r = X[r, 0:K] (transpose == 0) or X[0:K, r] (transpose != 0: X is [K][rows], ldx >= rows).
 * amax_out (may be NULL): abs-max vector (MI_AMAX_SLOTS floats) receiving max |X|. */
int32_t mi_split_rows(const float* X, int64_t ldx, int64_t rows, int32_t K, int32_t transpose,
                      const mi_planes_t* out, float* amax_out, mi_stream_t stream);
/* Every hidden layer's kernel as planes, both orientations, in one launch (once per training step).
 * Job q: W = dense + offset, [K][N] row-major; w (rows = K, the data gradient's operand) and / or wt (rows
 * = N, W transposed: the forward pass's) — a NULL data pointer skips one.  All rows get ONE exponent, from
 * amax (abs-max vector of the parameter block, mi_absmax): weights more than 2^-17 below the block's
 * largest lose low bits. */
#define MI_MAX_WEIGHT_JOBS 8
typedef struct mi_weight_job {
  int64_t offset;
  int32_t K, N;
  mi_planes_t w, wt;
} mi_weight_job_t;
int32_t mi_split_weights(const float* dense, const mi_weight_job_t* jobs, int32_t n_jobs, const float* amax,
                         mi_stream_t stream);
/* X[r, k] = (hi + lo) * 2^-s_r (tests, summaries) */
int32_t mi_merge_rows(const mi_planes_t* in, int64_t rows, int32_t K, float* X, int64_t ldx, mi_stream_t stream);

/* Y[M][N] = act(X[M][K] * W[K][N] + bias) with X as planes and Wt = planes of W TRANSPOSED (rows = N);
 * epilogue as mi_dense_fwd.  Y (fp32) and / or Yp (planes, N <= 512; a positive value keeps a positive high
 * part, so "hi > 0" is the relu/dropout mask of the data gradient) receive the result; amax_out (may be
 * NULL) its abs-max.
 * mask_bits_out (may be NULL; round 4): the same mask as ONE BIT per output — [M][mask_ld] 32-bit words, mask_ld >=
 * ceil(N / 32), bit (n & 31) of word (n >> 5) of row m = "Y[m][n] > 0" (active and kept).  The data gradients below take
 * it instead of the stored activation: 1/32 of the bytes (2 MB instead of the 134 MB high-plane read at 65536 x 512). */
int32_t mi_dense_fwd_planes(const mi_planes_t* X, const mi_planes_t* Wt, const float* bias, float* Y, int64_t ldy,
                            const mi_planes_t* Yp, int64_t M, int32_t N, int32_t K, int32_t relu, float keep_prob,
                            uint64_t seed, float* amax_out, uint32_t* mask_bits_out, int64_t mask_ld, mi_stream_t stream);

/* dX[M][K] = (dY[M][N] * W[K][N]^T) .* mask with dY as planes and W = planes of W as stored (rows = K);
 * mask from Xact (planes of the previous layer's stored output: hi > 0 <=> active and kept; NULL: none),
 * survivors divided by keep_prob.  dX (fp32) and / or dXp (planes, K <= 512).
 * mask_bits / mask_ld (may be NULL): the mask as mi_dense_fwd_planes' mask_bits_out wrote it ([M][mask_ld] words, one bit per
 * element of dX's K columns); taken instead of Xact when both are given — the same decisions, hence the same bits. */
int32_t mi_dense_bwd_data_planes(const mi_planes_t* dY, const mi_planes_t* W, const mi_planes_t* Xact, float* dX,
                                 int64_t lddx, const mi_planes_t* dXp, int64_t M, int32_t N, int32_t K, float keep_prob,
                                 float* amax_out, const uint32_t* mask_bits, int64_t mask_ld, mi_stream_t stream);

/* The logits layer AND the head of a TRAIN step in one pass over the last hidden layer's output X [M][K] (round 4): replaces
 * deep_fm.py:108 (tf.layers.dense(net, 1)), :111 (logits += dnn_logits), :118-125 (the sigmoid cross-entropy head) and
 * their gradients — five launches of the entries above and below (mi_dense_fwd's N = 1 form, mi_sigmoid_ce_head,
 * mi_dense_bwd_weight's N = 1 form, mi_dense_bwd_data_vec_planes) — with two:
 *   dnn[m] = X[m,:] . w + b;  logits[m] = lin[m] + lin_bias + fm[m] + dnn[m]  (lin / fm may be NULL);  loss_out = sum of the
 *   per-example sigmoid cross-entropy * loss_scale;  d_logit[m] = (sigmoid(logits) - label) * loss_scale;  d_logit_sum (may be
 *   NULL) and db = sum d_logit;  dW[k] = sum_m X[m][k] d_logit[m];  dXp (planes, + dX in fp32 if not NULL) = d_logit[m] w[k],
 *   kept where mask_bits says so and divided by keep_prob (mask_bits NULL: no mask) — per example the bits of the unfused
 *   sequence; the sums over examples associate differently (fixed order, reproducible).  K in {64, 128, 256}; X 16-byte
 *   aligned, ldx a multiple of 4. */
size_t mi_logits_head_fused_workspace_bytes(int64_t M, int32_t K);
int32_t mi_logits_head_fused(const float* X, int64_t ldx, const float* w, const float* b, const float* lin, const float* lin_bias,
                             const float* fm, const uint8_t* labels, int64_t M, int32_t K, float loss_scale,
                             const uint32_t* mask_bits, int64_t mask_ld, float keep_prob, float* dnn, float* logits,
                             float* loss_out, float* d_logit, float* d_logit_sum, float* dW, float* db, const mi_planes_t* dXp,
                             float* dX, int64_t lddx, float* amax_out, void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ... and the LAST HIDDEN layer with them (round 4): Y = dropout(relu(X W + bias)) [M][N] from planes as in
 * mi_dense_fwd_planes, then — in the GEMM's epilogue, Y never leaves the chip — everything mi_logits_head_fused does with it:
 * dnn, logits, loss, d_logit, the bias gradient(s), the logits layer's weight gradient dW [N] and its data gradient
 * dXp [M][N] (planes: d_logit[m] w[n], kept where Y[m][n] > 0, divided by keep_prob).  Replaces deep_fm.py:98-125 from the
 * last hidden layer up, forward and backward, with two launches (the GEMM and a fold of its workgroups' N + 2 partial sums);
 * saves the layer's output written and read back (2 x 4 M N bytes) and its mask bits.  N = 128 (one column tile holds the whole
 * layer); K a multiple of 16.  Per example the arithmetic of the two entries it fuses; the sum h . w of the logits layer and the
 * sums over examples associate in its own fixed order (tests: 2e-6 of sum |h w|, everything downstream on its own dnn). */
size_t mi_hidden_logits_head_fused_workspace_bytes(int64_t M, int32_t N);
int32_t mi_hidden_logits_head_fused(const mi_planes_t* X, const mi_planes_t* Wt, const float* bias, int64_t M, int32_t N, int32_t K,
                                    int32_t relu, float keep_prob, uint64_t seed, const float* w, const float* b, const float* lin,
                                    const float* lin_bias, const float* fm, const uint8_t* labels, float loss_scale, float* dnn,
                                    float* logits, float* loss_out, float* d_logit, float* d_logit_sum, float* dW, float* db,
                                    const mi_planes_t* dXp, float* amax_out, void* workspace, size_t workspace_bytes,
                                    mi_stream_t stream);

/* The data gradient of the N = 1 logits layer (deep_fm.py:108 backward) with the result as planes:
 * dX[m][k] = dY[m] * W[k], kept where Xact[m][k] > 0 and divided by keep_prob (Xact == NULL: no mask) — the
 * arithmetic of mi_dense_bwd_data's N = 1 form with ReLU, bit for bit — into dXp (required) and, if not NULL, dX.
 * amax_out as everywhere.  K a multiple of 16.  mask_bits / mask_ld: the one-bit mask (see mi_dense_fwd_planes), taken
 * instead of Xact when given. */
int32_t mi_dense_bwd_data_vec_planes(const float* dY, int64_t lddy, const float* W, const float* Xact, int64_t ldxa,
                                     float keep_prob, float* dX, int64_t lddx, const mi_planes_t* dXp, int64_t M, int32_t K,
                                     float* amax_out, const uint32_t* mask_bits, int64_t mask_ld, mi_stream_t stream);

/* dW[K][N] = X[M][K]^T * dY[M][N] and db[N] = column sums of dY (NULL: skipped), both operands as planes
 * (replaces the same gradients as mi_dense_bwd_weight: model_utils.py:69-72 through tf.layers.dense,
 * deep_fm.py:98-108).  The reduction runs over the examples, so every example's planes are brought to the
 * matrix-wide scales by one power of two (from its two row exponents and amax->a / amax->b, the abs-max vectors
 * of X and dY, both required); examples far below the abs-max lose low bits — invisible in a sum over
 * examples, as in mi_dense_bwd_weight's matrix-wide split.  M % 32 == 0, N % 128 == 0, K % 128 == 0 (anything
 * else: mi_dense_bwd_weight on fp32 copies).  Split-K slabs folded in a fixed order: bitwise reproducible. */
size_t mi_dense_bwd_weight_planes_workspace_bytes(int64_t M, int32_t N, int32_t K);
int32_t mi_dense_bwd_weight_planes(const mi_planes_t* X, const mi_planes_t* dY, float* dW, float* db, int64_t M,
                                   int32_t N, int32_t K, void* workspace, size_t workspace_bytes,
                                   const mi_gemm_amax_t* amax, mi_stream_t stream);

/* The weight gradients of SEVERAL layers from planes in one call (round 4): one launch makes every layer's per-example
 * factors, one launch per layer runs its split-K GEMM, one launch folds every layer's slabs — for the three hidden layers of
 * config 3 five launches instead of nine (the backward then runs all data gradients first: each needs only the layer
 * above's dY, and the factors of every layer need its finished dY planes and abs-max).  Results are those of
 * mi_dense_bwd_weight_planes per job, bit for bit.  workspace: mi_dense_bwd_weight_planes_batch_workspace_bytes, 32-byte
 * aligned (fewer bytes than the query names are refused, as is any bad job: every job is planned before the first launch,
 * so a refused call has written nothing); at most MI_MAX_WEIGHT_JOBS jobs. */
typedef struct mi_wgrad_job {
  mi_planes_t X, dY;        /* the layer's input and the gradient of its output, [M] rows each */
  float* dW; float* db;     /* [K][N], [N] (db may be NULL) */
  int32_t N, K;
  mi_gemm_amax_t amax;      /* a = abs-max vector of X, b = of dY */
} mi_wgrad_job_t;
size_t mi_dense_bwd_weight_planes_batch_workspace_bytes(const mi_wgrad_job_t* jobs, int32_t n_jobs, int64_t M);
int32_t mi_dense_bwd_weight_planes_batch(const mi_wgrad_job_t* jobs, int32_t n_jobs, int64_t M, void* workspace,
                                         size_t workspace_bytes, mi_stream_t stream);

/* ---- (a7,a8) logits sum + sigmoid cross-entropy head -----------------------------------------
 * replaces `logits += ...` (deep_fm.py:36,44,90,111) and
 * tf.contrib.estimator.binary_classification_head (deep_fm.py:118-125).
 *   logits[b] = ((lin[b] + lin_bias) + fm[b]) + dnn[b]        (NULL terms skipped, same order)
 *   loss_b    = max(x,0) - x*y + log1p(exp(-|x|))
 *   loss_out[0] = sum_b loss_b * loss_scale   (loss_scale = 1/B_global for the contrib head's
 *                 SUM_OVER_BATCH_SIZE, 1 for the canned estimators' SUM)
 *   d_logit[b]  = (sigmoid(x) - y) * loss_scale
 *   d_logit_sum[0] = sum_b d_logit[b]   (= gradient of the linear_model bias; fixed-order sum)
 * labels: uint8 0/1 (ml_100k.py:48 rating >= cutoff).  d_logit / d_logit_sum / loss_out may be NULL
 * (eval / predict).  workspace: mi_head_workspace_bytes(B).  Inputs are finite: an infinite or NaN term has no contract. */
size_t mi_head_workspace_bytes(int64_t B);
int32_t mi_sigmoid_ce_head(const float* lin, const float* lin_bias, const float* fm,
                           const float* dnn, const uint8_t* labels, int64_t B, float loss_scale,
                           float* logits, float* loss_out, float* d_logit, float* d_logit_sum,
                           void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* The head's per-example outputs: get_binary_predictions (model_utils.py:9-20; the PREDICT dict of
 * binary_classification_head) and get_binary_losses' unreduced loss (model_utils.py:23-36).
 *   logistic[b] = sigmoid(x)   probabilities[b] = {1 - p, p}   class_ids[b] = p > 0.5   (int64, as TF's)
 *   unreduced_loss[b] = max(x,0) - x*y + log1p(exp(-|x|))      (needs labels)
 * Any output may be NULL.  Inputs are finite: an infinite or NaN logit has no contract. */
int32_t mi_binary_predictions(const float* logits, const uint8_t* labels, int64_t B, float* logistic,
                              float* probabilities, int64_t* class_ids, float* unreduced_loss, mi_stream_t stream);

/* column sums: out[j] = sum_b X[b,j] (used for bias-style gradients), deterministic. */
size_t mi_colsum_workspace_bytes(int64_t M, int32_t N);
int32_t mi_colsum(const float* X, int64_t ldx, int64_t M, int32_t N, float* out, void* workspace,
                  size_t workspace_bytes, mi_stream_t stream);

/* ---- (a10) layer_summary statistics (model_utils.py:4-6) ------------------------------------
 * out[0] = fraction of zeros, out[1] = min, out[2] = max, out[3] = mean. */
size_t mi_layer_stats_workspace_bytes(int64_t n);
int32_t mi_layer_stats(const float* x, int64_t n, float* out4, void* workspace,
                       size_t workspace_bytes, mi_stream_t stream);

/* The histogram of layer_summary (tf.summary.histogram("activation", value), model_utils.py:6): counts[b] += 1
 * for b = number of limits <= x[i] (std::upper_bound over the ascending fp64 bucket limits, as TensorFlow's
 * histogram::Histogram::Add; its default limits are +-1e-12 * 1.1^k up to 1e20, 0 and +-DBL_MAX: 1,551 of
 * them — mi355x_rec/metrics.py builds them), sums[0] += sum x, sums[1] += sum x^2 (fp64).  counts
 * [n_limits + 1] int64 and sums [2] are accumulated into: zero them first.  n_limits <= 2048. */
int32_t mi_layer_histogram(const float* x, int64_t n, const double* limits, int32_t n_limits, int64_t* counts,
                           double* sums, mi_stream_t stream);

/* ---- (f3) streaming eval metrics: tf.metrics.auc confusion counts --------
 * Accumulates (integer atomics, order independent) into device arrays the caller zeroed:
 *   hist   [2*201] int64: hist[y*201+k] = examples with label y whose sigmoid exceeds exactly k of
 *          tf.metrics.auc's 200 ascending thresholds; tp[j] = sum_{k>j} hist[1][k] etc. on the host
 *   counts [8] int64: n, n_pos, n_pred_pos, n_correct, tp@.5, fp@.5, fn@.5, (unused)
 *   sums   [4] f64 : sum(loss_b), sum(sigmoid), sum(label), (unused)
 * Inputs are finite: an infinite or NaN logit has no contract. */
int32_t mi_eval_accumulate(const float* logits, const uint8_t* labels, int64_t B,
                           int64_t* hist /*[2*201]*/, int64_t* counts /*[8]*/,
                           double* sums /*[4]*/, mi_stream_t stream);

/* ---- top-K recommendation: fused pair scoring and selection (csrc/rank.hip) -------------------------------------
 * For U queries and I candidates, the best k candidates of every query by the model's logit, without the [U, I] pair
 * matrix.  The model decomposes over the two sides of a pair: with Q the query fields, C the candidate fields (a
 * partition of the input columns), s_X = sum_{f in X} e_f and fm_X = 0.5 (|s_X|^2 - sum_{f in X} |e_f|^2),
 *   logit(q, c) = w_q + w_c + s_q . s_c + MLP_{2..L}(act(a_q + a_c))
 *   w_X = lin_X + fm_X (the wide part's per-side sum; the candidate side also carries the wide bias),
 *   a_X = concat_X W1[rows of X] (layer 1 on the side's rows of kernel_0; b1 on the candidate side only).
 * The caller computes the per-side tensors (mi_embed_fm_linear_fwd, mi_numeric_*_fwd, layer 1 with identity
 * activation); per pair, act(a_q + a_c), layers 2..L (fp32-input MFMA; a VALU loop when every width after layer 1 is
 * below 32), the E-wide dot and the adds run on the chip and only the selection leaves it.
 *   a_q [U, H1], a_c [I, H1]   layer 1 per side (H1 = 0: no DNN; NULL then)
 *   s_q [U, E],  s_c [I, E]    embedding sums per side (E = 0: no FM cross term; NULL then)
 *   w_q [U],     w_c [I]       lin + fm per side (NULL: 0)
 *   dense, layer_off [2 n_layers] (host), widths [n_layers + 1] (host): layers 2..L, layer i + 2 with kernel
 *     dense[layer_off[2i]] [widths[i], widths[i+1]] and bias dense[layer_off[2i+1]] [widths[i+1]]; widths[0] = H1,
 *     widths[n_layers] = 1.  n_layers = 0 (no hidden layer): layer 1 is the logits layer, H1 = 1.  activation: the
 *     engine's code (0 identity, 1 relu, 2 sigmoid, 3 tanh) on every hidden layer, layer 1 included.
 *   excl_off [U + 1], excl_idx (device, CSR): candidates excluded per query, ascending; entries outside [0, I) are
 *     ignored.  Both NULL: nothing excluded.
 * Outputs: top_score [U, k] fp32 logits, top_idx [U, k] int32 candidate indices.  Order: score descending, equal scores
 * by ascending index, NaN below every number (-0 ranks as +0 and comes back as +0 in top_score, a NaN as the canonical
 * quiet NaN).  Fewer than k eligible candidates: the tail is index -1, score -inf.  scores [U, I] (optional, NULL on the hot path): every raw pair score, excluded pairs included (int64
 * offsets).  Deterministic: the selection is a function of the scores alone, and the scores of the split count.
 * Accuracy: each score is an fp32 evaluation of the same function in another summation order (within 1e-5 of an fp64
 * forward, scaled as max_err_scaled).  Limits: U, I >= 1, I < 2^31, 1 <= k <= 256, H1 <= 4096, E <= 256, at most 8
 * layers after layer 1, widths of layers 2, 4, ... <= 256 and of layers 3, 5, ... <= 128.  workspace: mi_pair_topk_workspace_bytes(U, I, k, H1, E). */
size_t mi_pair_topk_workspace_bytes(int64_t U, int64_t I, int32_t k, int32_t H1, int32_t E);
int32_t mi_pair_topk(const float* a_q, const float* s_q, const float* w_q, int64_t U,
                     const float* a_c, const float* s_c, const float* w_c, int64_t I, int32_t H1, int32_t E,
                     const float* dense, const int64_t* layer_off, const int32_t* widths, int32_t n_layers,
                     int32_t activation, const int64_t* excl_off, const int32_t* excl_idx, int32_t k,
                     float* top_score, int32_t* top_idx, float* scores, void* workspace, size_t workspace_bytes,
                     mi_stream_t stream);

/* ---- top-K recommendation with an ensemble: M models, one selection, one launch (csrc/rank.hip) ---------------------
 * What mi_pair_topk does for one model, for the mean logit of M models (the best members of a trainers.sweep): every
 * pair is scored by every member and
 *   z(q, c) = (((z_0 + z_1) + z_2) + ... + z_{M-1}) / (float)M     fp32, ascending member order, one rounding per
 *   operation, IEEE division (mi_predict_group's definition)
 * enters the selection — the grid, the on-chip running top-k, the order (score descending, equal scores by ascending
 * index, NaN below every number, -0 as +0), the exclusions and the -1 / -inf padding of mi_pair_topk.  z_m is bit for bit
 * the score mi_pair_topk gives member m alone (the same device function).  M = 1 takes the same path (z_0 / 1.0f).
 *
 * mi_rank_member_t: the per-model arguments of mi_pair_topk (same meaning, same checks and messages, prefixed
 *   "member i:"; layer_off / widths on the host).  Members share U, I, k and the exclusions; they may differ in H1, E,
 *   the layers, the activation, the model's parts (NULL w_q / w_c, H1 = 0, E = 0) and dense.
 * Scope: the VALU pair path only — a member qualifies if it has fewer than two layers after layer 1 or every hidden
 *   width after layer 1 is below 32 (any H1 <= 4096); any other member: MI_ERR_UNSUPPORTED.
 * Outputs: top_score / top_idx [U, k] as mi_pair_topk; optional (NULL on the hot path) scores [U, I], the mean, and
 *   member_scores [M, U, I], every member's own score.
 * workspace: mi_pair_topk_group_workspace_bytes(members, n_members, U, I, k) (only H1 and E of a member are read; 0 for
 *   arguments out of range) — it holds the member table, the transposes, the exclusion mask and the partial lists.
 * Launches: the member table (through the kernel arguments, 8 members a launch), one transpose launch for all members,
 *   the exclusion mask, ONE pair scoring and selection launch and the final merge; no copy, no synchronisation.  No
 *   workgroup reads what another writes in a launch and none waits for another; two calls give the same bits.
 * Refused on the host before anything is launched: n_members < 1 (MI_ERR_INVALID) or above
 *   MI_PAIR_TOPK_GROUP_MAX_MEMBERS (MI_ERR_UNSUPPORTED), a member outside the scope (MI_ERR_UNSUPPORTED) or failing
 *   mi_pair_topk's checks, a short workspace, NULL top_score / top_idx, excl_off without excl_idx (MI_ERR_INVALID). */
#define MI_PAIR_TOPK_GROUP_MAX_MEMBERS 256 /* = MI_PREDICT_GROUP_MAX_MEMBERS */
typedef struct mi_rank_member {
  const float* a_q; const float* s_q; const float* w_q;
  const float* a_c; const float* s_c; const float* w_c;
  const float* dense;
  const int64_t* layer_off;
  const int32_t* widths;
  int32_t H1, E, n_layers, activation;
} mi_rank_member_t;

size_t mi_pair_topk_group_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, int32_t k);
int32_t mi_pair_topk_group(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                           const int32_t* excl_idx, int32_t k, float* top_score, int32_t* top_idx, float* scores,
                           float* member_scores, void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- exact ranks of named candidates, every member for itself, one launch (csrc/rank.hip) ---------------------------
 * For M models, U queries and up to Tq named target candidates per query, where each target stands among ALL eligible
 * candidates of its query in each model's own order — the [U, I] pair matrix never leaves the chip.  For member m, query
 * q and target t = targets[q, j]:
 *   ranks[m, q, j] = #{c in [0, I), c != t, c not excluded for q : key(z_m(q, c), c) > key(z_m(q, t), t)}
 * with mi_pair_topk's order as the key (score descending, equal scores by ascending index, NaN below every number, -0 as
 * +0) and z_m bit for bit the score mi_pair_topk gives member m: the 0-based position t would take in that member's
 * mi_pair_topk list were k unbounded.  ranks[m, q, j] = -1 where t < 0 (padding), t >= I or t is excluded for q.  Other
 * targets of the query count as ordinary candidates; duplicate targets each get their own, equal, answer.
 *   members, n_members, U, I, excl_off, excl_idx: as mi_pair_topk_group (same scope: the VALU pair path; same checks and
 *     messages, prefixed "member i:").
 *   targets [U, Tq] int32 (device), 1 <= Tq <= MI_PAIR_RANKS_MAX_TARGETS.
 * Outputs: ranks [M, U, Tq] int32; target_scores [M, U, Tq] (optional, NULL to skip): the bits of z_m(q, t), the canonical
 *   quiet NaN where the rank is -1.
 * workspace: mi_pair_target_ranks_workspace_bytes(members, n_members, U, I, Tq) (only H1 and E of a member are read; 0
 *   for arguments out of range) — the member table, the transposes, the exclusion mask and the splits' partial counts.
 * Launches: the member table (through the kernel arguments), one transpose launch, the exclusion mask, ONE scoring and
 *   counting launch over (query blocks) x (candidate splits) x (members) and the sum of the splits' counts; no copy, no
 *   synchronisation.  The counts are integers written plainly and added in a second launch: the result depends neither on
 *   the split count nor on timing, and no workgroup waits for another.
 * Refused on the host before anything is launched: n_members < 1 (MI_ERR_INVALID) or above
 *   MI_PAIR_TOPK_GROUP_MAX_MEMBERS (MI_ERR_UNSUPPORTED), Tq outside [1, MI_PAIR_RANKS_MAX_TARGETS], NULL targets / ranks,
 *   excl_off without excl_idx (MI_ERR_INVALID), a member outside the scope (MI_ERR_UNSUPPORTED) or failing mi_pair_topk's
 *   checks, a short workspace (MI_ERR_INVALID). */
#define MI_PAIR_RANKS_MAX_TARGETS 64 /* per query and call */
size_t mi_pair_target_ranks_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, int32_t Tq);
int32_t mi_pair_target_ranks(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I, const int64_t* excl_off,
                             const int32_t* excl_idx, const int32_t* targets, int32_t Tq, int32_t* ranks, float* target_scores,
                             void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- exact ranks of named candidates under an ensemble's mean logit, one launch (csrc/rank.hip) ----------------------
 * What mi_pair_target_ranks does for every member's own score, for the MEAN score of the M members — the order
 * mi_pair_topk_group selects by.  For query q and target t = targets[q, j]:
 *   ranks[q, j] = #{c in [0, I), c != t, c not excluded for q : key(z(q, c), c) > key(z(q, t), t)}
 *   z(q, c) = (((z_0 + z_1) + z_2) + ... + z_{M-1}) / (float)M     fp32, ascending member order, one rounding per
 *   operation, IEEE division — mi_pair_topk_group's definition: z is bit for bit what that entry writes to `scores`
 * with mi_pair_topk's order as the key (score descending, equal scores by ascending index, NaN below every number, -0 as
 * +0): the 0-based position t would take in mi_pair_topk_group's list were k unbounded.  ranks[q, j] = -1 where t < 0
 * (padding), t >= I or t is excluded for q.  Other targets of the query count as ordinary candidates; duplicate targets
 * each get their own, equal, answer.  M = 1 takes the same path (z_0 / 1.0f).
 *   members, n_members, U, I, excl_off, excl_idx, targets, Tq: as mi_pair_target_ranks (same scope: the VALU pair path;
 *     same checks and messages, prefixed "member i:").
 * Outputs: ranks [U, Tq] int32; target_scores [U, Tq] (optional, NULL to skip): the bits of z(q, t), the canonical quiet
 *   NaN where the rank is -1.
 * workspace: mi_pair_target_ranks_mean_workspace_bytes(members, n_members, U, I, Tq) (only H1 and E of a member are read;
 *   0 for arguments out of range) — the exclusion mask, the splits' partial counts, the member table and the transposes.
 * Launches: the member table (through the kernel arguments), one transpose launch, the exclusion mask, ONE scoring and
 *   counting launch over (query blocks) x (candidate splits) — the members are a loop inside it: the mean needs every
 *   member's score of a pair in one lane — and the sum of the splits' counts; no copy, no synchronisation.  The counts are
 *   integers written plainly and added in a second launch: the result depends neither on the split count nor on timing,
 *   and no workgroup waits for another.
 * Refused on the host before anything is launched: what mi_pair_target_ranks refuses, with the same codes. */
size_t mi_pair_target_ranks_mean_workspace_bytes(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                                                 int32_t Tq);
int32_t mi_pair_target_ranks_mean(const mi_rank_member_t* members, int32_t n_members, int64_t U, int64_t I,
                                  const int64_t* excl_off, const int32_t* excl_idx, const int32_t* targets, int32_t Tq,
                                  int32_t* ranks, float* target_scores, void* workspace, size_t workspace_bytes,
                                  mi_stream_t stream);

/* ---- serving: the forward of a request batch as one launch (csrc/serve.hip) ---------------------------------------
 * For B requests, what DeepFM.predict_logits followed by mi_binary_predictions computes (deep_fm.py:36-125 in PREDICT
 * mode, model_utils.py:9-20; the requests of ml_100k.py:64-88's receiver after the columns' id transforms):
 *   logits[b] = ((lin[b] + lin_bias) + fm[b]) + dnn[b]     (absent parts skipped; the order of mi_sigmoid_ce_head)
 *   logistic [B], probabilities [B, 2], class_ids [B] int64: mi_binary_predictions' device functions on that logit,
 *   bit for bit.  Any output may be NULL (not all four).
 * Inputs are the engine's arrays, read in place:
 *   table (rows table_stride floats apart, 0 = E), lin_w (weights lin_stride floats apart), field_off [F] (device),
 *   ids [B, F] int32 (trusted to lie inside their field), x_num [B, n_numeric] (NULL without numeric columns);
 *   dense, layer_off [2 n_layers] (host), widths [n_layers + 1] (host): layer i of the MLP, the logits layer included,
 *     has kernel dense[layer_off[2i]] [widths[i], widths[i+1]] and bias dense[layer_off[2i+1]] [widths[i+1]];
 *     widths[0] = rows of kernel_0 as stored (>= the input columns), widths[n_layers] = 1; n_layers = 0 without a DNN.
 *     activation: the engine's code (0 identity, 1 relu, 2 sigmoid, 3 tanh) on every layer but the last;
 *   use_linear / use_fm / use_dnn: the model's parts.  numeric_raw = 0: numeric column j enters as the row
 *     x[b, j] * dense[num_emb_off + j E ..] (mi_numeric_embed_fwd: seen by the FM term and the MLP; linear weight
 *     dense[lin_num_off + j]); 1: as the value itself after the embedding columns (mi_numeric_raw_fwd; no FM term);
 *   lin_bias_off: the wide part's bias in dense;  wide_fields: bit f set = categorical field f has a linear weight.
 *   Narrower embedding columns need nothing: their unused table columns and rows of kernel_0 are zero.
 * Arithmetic: fp32 variables, exact fp32 products (fp32-input MFMA), fp32 accumulation; the FM term rounds each product
 * on its own (a model with one field gives exactly 0).  Within 1e-5 of an fp64 forward, scaled as max_err_scaled.
 * A request's outputs do not depend on the other requests of the call; two calls give the same bits.
 * Limits, checked before anything is launched (MI_ERR_INVALID / MI_ERR_UNSUPPORTED): B >= 1, F in [0, 64] with
 * F + n_numeric >= 1 (F = 0: numeric columns only; table, field_off and ids may be NULL), E a multiple of 4 in [4, 256]
 * wherever a table row or a numeric embedding is read, at most 8 hidden layers, every layer's OUTPUT width
 * widths[1 .. n_layers] <= 512 (widths[0], the rows of kernel_0, is bounded by nothing but the arrays: >= the input
 * columns, rows past them are never multiplied in and must be finite), and 128 (F + the widest output of the layers 0, 2,
 * .. + the widest of the layers 1, 3, ..) + 4096 <= 160 KiB of LDS: F = 64 with 512 / 512 is the largest launch.
 * Enqueues one kernel on the stream; no scratch:
 * mi_predict_fused_workspace_bytes is 0 today and workspace may be NULL (kept in the ABI for later shapes). */
size_t mi_predict_fused_workspace_bytes(int64_t B, int32_t n_layers);
int32_t mi_predict_fused(const float* table, int64_t table_stride, const float* lin_w, int32_t lin_stride,
                         const int64_t* field_off, const int32_t* ids, const float* x_num, int64_t B, int32_t F, int32_t E,
                         int32_t n_numeric, const float* dense, const int64_t* layer_off, const int32_t* widths,
                         int32_t n_layers, int32_t activation, int32_t use_linear, int32_t use_fm, int32_t use_dnn,
                         int32_t numeric_raw, int64_t lin_bias_off, int64_t num_emb_off, int64_t lin_num_off,
                         uint64_t wide_fields, float* logits, float* logistic, float* probabilities, int64_t* class_ids,
                         void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- training small models: one optimizer.minimize(loss) as one launch (csrc/train_fused.hip) ------------------------
 * What trainers/deep_fm.py:36-125 builds and model_utils.py:57-72 minimises, for one batch of a DeepFM with categorical
 * columns only and Adam on every variable (one schedule): gather, wide part, FM term, MLP forward with dropout,
 * sigmoid-CE head, full backward, dense Adam, and TF's dense-equivalent sparse Adam as the LITERAL all-rows sweep
 *  — no sort, no stamps to order, no replay loop.  One kernel: block 0 does everything that depends on the
 * loss and applies the touched rows and the dense variables; the other blocks own disjoint slices of the R rows and give
 * every row the batch does not touch one step of the sweep (m *= beta1; v *= beta2; w -= (lr_t m) / (sqrtf(v) + eps)).
 * No workgroup reads what another writes in the launch and none waits for another.
 *   table / t_m / t_v (rows table_stride floats apart, 0 = E; NULL without FM term and DNN), lin_w / l_m / l_v and
 *   last_step (elements lin_stride apart; lin_* NULL without the wide part), field_off [F] (device), R = rows in all,
 *   ids [B, F] int32 (trusted to lie inside their field), labels [B] uint8;
 *   dense / d_m / d_v [n_dense] with layer_off [2 n_layers] and widths [n_layers + 1] (host) as in mi_predict_fused
 *     (widths[0] = F E); activation: 0 identity, 1 relu, 2 sigmoid, 3 tanh;  lin_bias_off: the wide part's bias;
 *   keep_prob: 1 - dropout; hidden layer i draws the mask of mi_dense_fwd with seed + 7919 i;
 *   scale: 1 / B (mean) or 1 (sum); step: the global step AFTER this call (>= 1); hp: Adam with lr_t of that step.
 * PRECONDITION: every row is current (last_step == step - 1, or 0 with m = v = 0), as after mi_sparse_catchup over all rows.
 * Results: logits [B] (before the update), loss [1]; every variable and slot updated; last_step == step for EVERY row.
 * Entries of one row are summed in ascending entry order (mi_sparse_apply's order); the entry gradient is
 * mi_sparse_apply_fused's.  Untouched rows get the bits of the exact one-step mi_sparse_catchup.  Results do not depend on
 * sweep_blocks (0 = the built-in choice; a test seam) and are bitwise reproducible from equal state.
 * Limits, checked before anything is launched (MI_ERR_UNSUPPORTED / MI_ERR_INVALID): Adam; 1 <= B <= 128; 1 <= F <= 32;
 * E in {4, 8, 12, 16}; B F E <= 16384; at most 3 hidden layers of width <= 64; R <= 2^18; sweep_blocks <= 1024.
 * workspace: mi_train_step_fused_workspace_bytes(B, F, E, n_dense) bytes, 16-byte aligned, touched by block 0 only
 * (the dense gradient, and d_concat when LDS has no room for it). */
size_t mi_train_step_fused_workspace_bytes(int64_t B, int32_t F, int32_t E, int64_t n_dense);
int32_t mi_train_step_fused(float* table, float* t_m, float* t_v, int64_t table_stride, float* lin_w, float* l_m, float* l_v,
                            int32_t lin_stride, int32_t* last_step, const int64_t* field_off, int64_t R, const int32_t* ids,
                            const uint8_t* labels, int64_t B, int32_t F, int32_t E, float* dense, float* d_m, float* d_v,
                            int64_t n_dense, const int64_t* layer_off, const int32_t* widths, int32_t n_layers,
                            int32_t activation, int32_t use_linear, int32_t use_fm, int32_t use_dnn, int64_t lin_bias_off,
                            float keep_prob, uint64_t seed, float scale, int32_t step, const mi_opt_hparams* hp,
                            float* logits, float* loss, int32_t sweep_blocks, void* workspace, size_t workspace_bytes,
                            mi_stream_t stream);

/* ---- training a population of small models: M steps of M models as one launch (csrc/train_fused.hip) ------------------
 * What trainers/deep_fm.py:36-125 builds and model_utils.py:57-72 minimises, run M times (a grid of hyper-parameters, seeds,
 * folds): M INDEPENDENT models of mi_train_step_fused's scope take one step each in ONE kernel, grid (1 + G, M) — row y of
 * the grid is member y's batch workgroup and its G sweep workgroups, running the device code of mi_train_step_fused.
 * Member i's results are bit for bit those of mi_train_step_fused on it alone.  A member's workgroups touch only that
 * member's buffers; no workgroup reads what another writes in the launch and none waits for another.
 *
 * mi_fused_member_t: the per-model arguments of mi_train_step_fused (same meaning, same limits; layer_off / widths on the
 *   host, read by mi_train_group_plan only; hp.lr_t is ignored) and
 *   lr_table [lr_table_len] (device): lr_t of global step s at [s] (index 0 unused) — the member's Adam schedule;
 *   seed_base: the dropout seed of a step is seed_base + step * 1000003 (mod 2^64), hidden layer i adds 7919 i;
 *   workspace: mi_train_step_fused_workspace_bytes(B, F, E, n_dense) bytes of the member's own, 16-byte aligned.
 * Members may differ in everything above; they share B, F and field_off [F] (one set of feature columns). */
#define MI_FUSED_GROUP_MAX_MEMBERS 1024 /* the grid is at most (1 + 1024) x 1024 workgroups */
typedef struct mi_fused_member {
  float* table; float* t_m; float* t_v;
  int64_t table_stride;
  float* lin_w; float* l_m; float* l_v;
  int32_t* last_step;
  int64_t R;
  float* dense; float* d_m; float* d_v;
  int64_t n_dense;
  const int64_t* layer_off;
  const int32_t* widths;
  int64_t lin_bias_off;
  const float* lr_table;
  int64_t lr_table_len;
  uint64_t seed_base;
  void* workspace;
  size_t workspace_bytes;
  int32_t lin_stride, E, n_layers, activation, use_linear, use_fm, use_dnn;
  float keep_prob, scale;
  mi_opt_hparams hp;
} mi_fused_member_t;

/* What mi_train_group_plan leaves on the host for mi_train_group_step (caller-owned; treat as opaque). */
typedef struct mi_fused_group_plan {
  void* device_table;
  uint64_t magic;
  int32_t n_members, B, F, sweep_blocks, max_step;
  uint32_t lds_bytes;
} mi_fused_group_plan_t;

/* mi_train_group_plan: validates every member with the checks and messages of mi_train_step_fused (prefixed
 * "member i:"), refuses two members that share a state or workspace pointer, then writes the members' descriptions into
 * device_table (mi_train_group_plan_bytes(n_members) bytes of device memory, 16-byte aligned; the copy has completed when
 * the call returns) and *plan.  The plan holds the members' pointers: make a new one when a buffer, a schedule table or B
 * changes.  n_members in [1, MI_FUSED_GROUP_MAX_MEMBERS] (MI_ERR_INVALID below, MI_ERR_UNSUPPORTED above).
 *
 * mi_train_group_step: one launch, no host-to-device copy, no synchronisation.  ids [B, F] / labels [B] for all members
 * (member stride 0) or one batch per member ([M, B, F] / [M, B], member stride B F / B); step: the global step AFTER the
 * call, the same for every member (1 <= step < every lr_table_len); member i's lr_t = lr_table[step] and its dropout seed
 * are formed in the kernel.  Results: logits [M, B], loss [M]; each member as after mi_train_step_fused (PRECONDITION as
 * there: every row of every member current).  Dynamic LDS is the largest member's; sweep_blocks (G; 0 = the built-in
 * choice: the largest member's, lowered until (1 + G) M <= 65536) is one value for the launch and no result depends on it.
 * A refused call launches nothing and writes nothing (mi_train_group_plan: neither device_table nor *plan). */
size_t mi_train_group_plan_bytes(int32_t n_members);
int32_t mi_train_group_plan(const mi_fused_member_t* members, int32_t n_members, int64_t B, int32_t F, const int64_t* field_off,
                            void* device_table, size_t device_table_bytes, mi_fused_group_plan_t* plan, mi_stream_t stream);
int32_t mi_train_group_step(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids, int64_t ids_member_stride,
                            const uint8_t* labels, int64_t labels_member_stride, int64_t B, int32_t step, float* logits,
                            float* loss, int32_t sweep_blocks, mi_stream_t stream);

/* ---- the one-launch step under any of the five optimizers, two rules and the canned estimators' columns ------------------
 * What trainers/linear.py, deep.py and linear_deep.py train (LinearClassifier: Ftrl; DNNClassifier: Adagrad;
 * DNNLinearCombinedClassifier: Ftrl on TF's "linear" scope, Adagrad on its "dnn" scope) and what model_utils.get_optimizer
 * offers model_fn (Adagrad, Adam, Ftrl, RMSProp, SGD), as the ONE launch of mi_train_step_fused: the same device code.
 *
 * mi_fused_model_t: mi_fused_member_t's fields with the same meaning, and
 *   two_rules / hp_wide: 0 = every variable follows hp (hp_wide is ignored); 1 = the WIDE part — the lin_w records and the
 *     wide bias at lin_bias_off — follows hp_wide, everything else hp (needs use_linear);
 *   dw_m / dw_v [n_dense]: with two_rules the wide part's dense slots, indexed like dense (the bias's at lin_bias_off);
 *   lr_table_wide / lr_table_wide_len: hp_wide's Adam schedule (plans only), as lr_table is hp's;
 *   wide_fields: bit f set = categorical field f has a linear weight (mi_predict_fused's meaning).  The wide sum, the wide
 *     gradient and the wide record's update skip the other fields; such a field's wide record is never written.
 * Slots: Adam, Ftrl and RMSProp keep two, Adagrad slot 0 only (t_m / l_m / d_m / dw_m), SGD none.  A slot the rule does not
 *   keep is neither read nor written, whatever its pointer (pass NULL); a slot it keeps must be there.  The record strides
 *   are the caller's: table_stride >= E floats for table records, lin_stride for wide records.
 * The sweep: only records under Adam are walked — a sweep workgroup gives an untouched row one replay step on each of its
 *   records whose rule is Adam, with that rule's own lr_t, and stamps it.  Under the other four rules untouched rows are
 *   neither read nor written (TensorFlow's sparse applies of those optimizers touch the batch's rows only).  With no part
 *   under Adam no sweep workgroup is launched (grid (1); in a group a member without Adam returns from its sweep
 *   workgroups at once), last_step may be NULL and no stamp is written; with one it must be there and ends == step on
 *   every row.
 * Embedding columns narrower than E (the canned estimators' per-column dimensions) need nothing here: their padding and the
 *   matching rows of kernel_0 are zero, their gradients are products with those zeros, and every rule leaves them zero.
 * Limits and results otherwise as for mi_train_step_fused; refused in addition (MI_ERR_INVALID, nothing launched or
 * written): an optimizer kind outside the five, a missing slot, last_step NULL with a part under Adam, two_rules without
 * use_linear, a wide_fields bit at or above F, Ftrl with lr_power != -0.5.
 *
 * mi_train_step_model: one step of one model; hp.lr_t and hp_wide.lr_t are the caller's (lr_table* and seed_base unused),
 *   seed as in mi_train_step_fused.  mi_train_group_plan_models: mi_train_group_plan for such models — a schedule table is
 *   required exactly for a rule that is Adam — writing the same plan, which mi_train_group_step and mi_eval_group take;
 *   step <= every table's last index.  Both share mi_train_step_fused's planning: a model that entry accepts gets its bits. */
typedef struct mi_fused_model {
  float* table; float* t_m; float* t_v;
  int64_t table_stride;
  float* lin_w; float* l_m; float* l_v;
  int32_t* last_step;
  int64_t R;
  float* dense; float* d_m; float* d_v;
  int64_t n_dense;
  const int64_t* layer_off;
  const int32_t* widths;
  int64_t lin_bias_off;
  const float* lr_table;
  int64_t lr_table_len;
  uint64_t seed_base;
  void* workspace;
  size_t workspace_bytes;
  int32_t lin_stride, E, n_layers, activation, use_linear, use_fm, use_dnn;
  float keep_prob, scale;
  mi_opt_hparams hp;
  int32_t two_rules;
  mi_opt_hparams hp_wide;
  float* dw_m; float* dw_v;
  const float* lr_table_wide;
  int64_t lr_table_wide_len;
  uint64_t wide_fields;
} mi_fused_model_t;

int32_t mi_train_step_model(const mi_fused_model_t* model, const int64_t* field_off, const int32_t* ids, const uint8_t* labels,
                            int64_t B, int32_t F, uint64_t seed, int32_t step, float* logits, float* loss, int32_t sweep_blocks,
                            mi_stream_t stream);
int32_t mi_train_group_plan_models(const mi_fused_model_t* models, int32_t n_members, int64_t B, int32_t F,
                                   const int64_t* field_off, void* device_table, size_t device_table_bytes,
                                   mi_fused_group_plan_t* plan, mi_stream_t stream);

/* ---- evaluating a population of small models: a whole evaluation set, for every member, as one launch ------------------
 * What Estimator.evaluate does for one model (the EVAL branch of trainers/deep_fm.py:118-125 and model_utils.py:39-54) for
 * the M members of a plan mi_train_group_plan wrote: the forward of mi_train_step_fused — the same device code — WITHOUT
 * dropout (keep_prob = 1 whatever the member's) and without any backward, over ids [N, F] / labels [N] (one set for all
 * members) in tiles of the plan's B examples (tile t = examples [t B, min(N, (t + 1) B)); T = ceil(N / B); the last tile may
 * be short), and mi_eval_accumulate's counters on those logits, kept on the chip.  Grid (X, M): a workgroup walks the tiles
 * t = x, x + X, ... of its member.  Nothing of any member (variable, slot, stamp, workspace) is written.
 *   batch_loss [M, T] fp32: the loss of tile t alone, reduced in the head's order with the member's scale — what
 *     mi_train_step_fused reports as loss for that batch with keep_prob = 1;
 *   tail_scale [M] (device): member i's scale on a SHORT last tile of n = N mod B examples (the fp32 of 1 / n for a mean,
 *     1 for a sum); may be NULL when B divides N;
 *   logits [M, N] fp32, optional (NULL on the hot path);
 *   hist [M, 2*201] and counts [M, 8] int64: per member exactly mi_eval_accumulate's (integer atomics into arrays the
 *     CALLER ZEROED; order independent);
 *   partials [M, T, 3] f64: per tile sum(loss_b), sum(sigmoid), sum(label) with mi_eval_accumulate's terms, reduced inside
 *     the workgroup in a fixed order and written with a plain store; the host adds the tiles in ascending order.
 * No float atomics go to global memory: two calls give the same bits, and no result depends on X.  No workgroup reads
 * what another writes in the launch and none waits for another.  blocks: X (0 = the built-in choice from M, T and the
 * chip's 256 compute units: about 1024 workgroups in all, at most T per member; at most 1024, and X M <= 65536; a test
 * seam).  PRECONDITION as for the step: every row of every member current.  Refused on the host before anything is
 * launched (MI_ERR_INVALID; blocks out of range MI_ERR_UNSUPPORTED): a plan mi_train_group_plan did not write, n_members
 * other than the plan's, N < 1, NULL ids / labels / batch_loss / hist / counts / partials, NULL tail_scale with a short tile.
 * One launch, no copy, no synchronisation. */
int32_t mi_eval_group(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids, const uint8_t* labels, int64_t N,
                      const float* tail_scale, float* logits, float* batch_loss, int64_t* hist, int64_t* counts, double* partials,
                      int32_t blocks, mi_stream_t stream);

/* ---- numeric columns in the one-launch step, the population step and the population evaluation -------------------------
 * The reference's model_fn takes numeric_columns (trainers/deep_fm.py:59-74, :39): numeric column j owns row j of
 * numeric_embeddings [nd, E], enters the concat as that row scaled by the column's value, and the wide part holds one weight
 * per column on the value.  The entries below are mi_train_step_model, mi_train_group_plan_models, mi_train_group_step,
 * mi_eval_group and mi_train_step_fused_workspace_bytes with that: the same kernels, the same device code, one more input.
 * (Raw numeric columns — the canned estimators' form, the value itself an MLP input — are not in their scope.)
 *
 * mi_fused_numeric_t: n_numeric = nd; num_emb_off: numeric_embeddings [nd, E] in dense; lin_num_off: the numeric linear
 *   weights [nd] in dense (read with use_linear only) — the engine's offsets, as mi_predict_fused takes them.  Both are
 *   dense variables: their slots are d_m / d_v at the same offsets, and with two_rules the numeric linear weights belong to
 *   the WIDE part like the wide bias (hp_wide, dw_m / dw_v).  NULL, or n_numeric = 0: no numeric column — the call is the
 *   entry without "_numeric", bit for bit, and x_num may be NULL.
 * x_num [B, nd] fp32 (device): the values, trusted to be finite as ids are trusted to lie inside their field.
 *
 * Forward.  The concat is the F gathered rows followed by the nd rows  x[b, j] * V[j, :]  (widths[0] = (F + nd) E):
 *   sumv and the FM term take the numeric rows after the categorical ones, j ascending, every product rounded on its own;
 *   layer 1 continues over the nd E further inputs against rows F E .. of kernel_0 (fmaf on the rounded product x V);
 *   lin[b] = (the categorical wide sum) + x[b, 0] w_num[0] + x[b, 1] w_num[1] + ..., j ascending, each product rounded on
 *   its own; the wide bias stays with the head.  A numeric row is recomputed wherever it is read and stored nowhere.
 * Backward, for every j, e:
 *   g[b, j, :] = d_concat[b, F + j, :] + dlogit[b] * (sumv[b, :] - x[b, j] V[j, :])        (the categorical entry gradient)
 *   dV[j, e]   = sum_b x[b, j] * g[b, j, e]          dw_num[j] = sum_b dlogit[b] * x[b, j]
 *   each summed by ONE thread over b ascending, one rounding per operation, into the dense-gradient workspace, and applied
 *   by dense_rule with the other dense variables.  No atomics to global memory; no workgroup waits for another; the sweep
 *   workgroups are as before (a numeric column owns no table row).  With x_num all zero, V, w_num and their slots keep
 *   their bits under every rule whose update of a zero gradient on zero slots is zero (Adam from zero slots, SGD, Adagrad).
 * Limits, checked on the host before anything is launched: those of mi_train_step_model with 1 <= F <= 32 unchanged, and
 *   0 <= nd <= 16 and B (F + nd) E <= 16384 — the concat's budget: 26 + 13 columns fit at E = 4, B = 32 — (MI_ERR_UNSUPPORTED);
 *   with nd > 0: use_fm or use_dnn, x_num not NULL, the offsets inside dense (MI_ERR_INVALID).
 * workspace: mi_train_step_fused_workspace_bytes_numeric(B, F, nd, E, n_dense) — the dense gradient and d_concat
 *   [B, (F + nd) E].
 *
 * mi_train_group_plan_models_numeric: numerics [n_members] beside models (NULL: none).  All members share n_numeric, as
 *   they share F (MI_ERR_INVALID, "member i:", otherwise); the offsets are per member.  Writes the same plan struct.
 * mi_train_group_step_numeric / mi_eval_group_numeric: x_num and its member stride — 0 = one [B, nd] ([N, nd]) array for all
 *   members, else [M, B, nd] (B nd) / [M, N, nd] (N nd), as with ids.  They take any plan; without numeric columns x_num is
 *   not read.  mi_train_group_step and mi_eval_group REFUSE a plan that holds numeric columns (MI_ERR_INVALID; nothing is
 *   launched or written): they have no x_num to give it.  A member's bits are those of mi_train_step_model_numeric on it
 *   alone; evaluation logits are the step's logits at keep_prob = 1 on the same state. */
typedef struct mi_fused_numeric {
  int32_t n_numeric;
  int64_t num_emb_off;
  int64_t lin_num_off;
} mi_fused_numeric_t;

size_t mi_train_step_fused_workspace_bytes_numeric(int64_t B, int32_t F, int32_t n_numeric, int32_t E, int64_t n_dense);
int32_t mi_train_step_model_numeric(const mi_fused_model_t* model, const mi_fused_numeric_t* numeric, const int64_t* field_off,
                                    const int32_t* ids, const float* x_num, const uint8_t* labels, int64_t B, int32_t F,
                                    uint64_t seed, int32_t step, float* logits, float* loss, int32_t sweep_blocks,
                                    mi_stream_t stream);
int32_t mi_train_group_plan_models_numeric(const mi_fused_model_t* models, const mi_fused_numeric_t* numerics, int32_t n_members,
                                           int64_t B, int32_t F, const int64_t* field_off, void* device_table,
                                           size_t device_table_bytes, mi_fused_group_plan_t* plan, mi_stream_t stream);
int32_t mi_train_group_step_numeric(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids,
                                    int64_t ids_member_stride, const float* x_num, int64_t x_num_member_stride,
                                    const uint8_t* labels, int64_t labels_member_stride, int64_t B, int32_t step, float* logits,
                                    float* loss, int32_t sweep_blocks, mi_stream_t stream);
int32_t mi_eval_group_numeric(const mi_fused_group_plan_t* plan, int32_t n_members, const int32_t* ids, const float* x_num,
                              int64_t x_num_member_stride, const uint8_t* labels, int64_t N, const float* tail_scale,
                              float* logits, float* batch_loss, int64_t* hist, int64_t* counts, double* partials, int32_t blocks,
                              mi_stream_t stream);

/* ---- serving an ensemble: M models over one request batch, averaged, as one launch (csrc/serve.hip) --------------------
 * The payoff of a sweep (trainers/sweep.py): its best M members scored and averaged as ONE model.  Grid (ceil(B / 32), M):
 * row y of the grid runs the device code of mi_predict_fused on member y (member_logits[y, b] holds the bits of
 * mi_predict_fused on that member alone), and the members of a tile of 32 requests are combined inside the launch by the
 * workgroup that arrives last at the tile's ticket (an integer fetch_add; agent-scope release before it, acquire after it):
 *   logits[b] = (((z_0 + z_1) + z_2) + ... + z_{M-1}) / (float)M     fp32, ascending member order, one rounding per
 *   operation, IEEE division; logistic / probabilities / class_ids: mi_binary_predictions' device functions on that logit.
 * No workgroup waits for another (no spin, no grid barrier, no float atomics): the launch cannot hang, and the bits depend on
 * neither dispatch order nor placement.  M = 1 takes the same path (z_0 / 1.0f).
 *
 * mi_serve_member_t: the per-model arguments of mi_predict_fused (same meaning, same limits; layer_off / widths on the
 *   host, read by mi_predict_group_plan only).  Members may differ in all of them; they share F, n_numeric and
 *   field_off [F] (one set of feature columns). */
#define MI_PREDICT_GROUP_MAX_MEMBERS 256
typedef struct mi_serve_member {
  const float* table;
  int64_t table_stride;
  const float* lin_w;
  const float* dense;
  const int64_t* layer_off;
  const int32_t* widths;
  int64_t lin_bias_off, num_emb_off, lin_num_off;
  uint64_t wide_fields;
  int32_t lin_stride, E, n_layers, activation, use_linear, use_fm, use_dnn, numeric_raw;
} mi_serve_member_t;

/* What mi_predict_group_plan leaves on the host for mi_predict_group (caller-owned; treat as opaque). */
typedef struct mi_serve_group_plan {
  void* device_table;
  uint64_t magic;
  int32_t n_members, F, n_numeric;
  uint32_t lds_bytes;
} mi_serve_group_plan_t;

/* mi_predict_group_plan: validates every member with the checks and messages of mi_predict_fused (prefixed "member i:"),
 * then writes the members' descriptions into device_table (mi_predict_group_plan_bytes(n_members) bytes of device memory,
 * 16-byte aligned; the copy has completed when the call returns) and *plan.  The plan holds the members' pointers: make a
 * new one when a buffer changes.  n_members in [1, MI_PREDICT_GROUP_MAX_MEMBERS] (MI_ERR_INVALID below,
 * MI_ERR_UNSUPPORTED above).  A refused plan writes neither device_table nor *plan.
 *
 * mi_predict_group: one launch, no host-to-device copy, no synchronisation, no workspace.
 *   ids [B, F] int32, x_num [B, n_numeric] (NULL without numeric columns): one request batch for all members;
 *   member_logits [M, B] fp32, required: every member's own logit, and where the members meet;
 *   tickets int32 [ceil(B / 32)], caller-owned: ZERO on entry, zero again when the call has completed (the reducer of a
 *     tile resets it), so one buffer serves call after call on a stream;
 *   logits [B], logistic [B], probabilities [B, 2], class_ids [B] int64: any may be NULL (not all four).
 * Dynamic LDS is the largest member's.  Refused on the host before anything is launched (MI_ERR_INVALID): a plan
 * mi_predict_group_plan did not write, n_members other than the plan's, B < 1, NULL ids / member_logits / tickets, NULL
 * x_num with numeric columns, no output. */
size_t mi_predict_group_plan_bytes(int32_t n_members);
int32_t mi_predict_group_plan(const mi_serve_member_t* members, int32_t n_members, int32_t F, int32_t n_numeric,
                              const int64_t* field_off, void* device_table, mi_serve_group_plan_t* plan, mi_stream_t stream);
int32_t mi_predict_group(const mi_serve_group_plan_t* plan, int32_t n_members, const int32_t* ids, const float* x_num, int64_t B,
                         float* member_logits, int32_t* tickets, float* logits, float* logistic, float* probabilities,
                         int64_t* class_ids, mi_stream_t stream);

/* ---- exact AUC and per-group AUC of a population's logits: pair counts as one launch (csrc/auc.hip) --------------------
 * The "auc" of mi_eval_accumulate is tf.metrics.auc's trapezoid over 200 thresholds in probability: its error depends on
 * the scale of the logits, so it is a poor yardstick BETWEEN the members of a sweep.  These entries count, for every member
 * and every group of examples, the (positive, negative) pairs whose positive scores higher and those that tie:
 *   AUC = (2 gt + eq) / (2 P N-), formed on the host.  Integers only; exact; independent of order, grid and timing.
 * The count is O(P N-) per member on purpose: the entries are meant for the held-out sets of sweeps (20,000 examples are 1e8
 * pairs a member); an evaluation of any size, the large-batch path's among them, gets the same integers from
 * mi_auc_sorted_counts below, which sorts instead.
 *
 * Key of a logit: the 32-bit monotone image of the fp32 that mi_pair_topk's order uses (csrc/score_key.h): NaN is below
 * every number and equal to every other NaN, -0 equals +0.
 *
 * Layout of one evaluation set, built by the host once and shared by all members (the kernel takes no labels):
 *   order [N] int32 (device): a permutation of the examples, segment major, within a segment the negatives first;
 *   seg_off [S + 1], seg_neg [S] int64 (HOST): positions [seg_off[s], seg_off[s] + seg_neg[s]) of `order` are segment s's
 *     negatives, [seg_off[s] + seg_neg[s], seg_off[s + 1]) its positives.  The global AUC is S = 1.
 *
 * mi_auc_plan: cuts every segment that has both classes into work items (segment, a tile of at most 64 positives, a run
 * of at most C negatives; a segment of one class yields none) and copies the item table into device_table
 * (mi_auc_plan_bytes(...) bytes of device memory for the same arguments, 16-byte aligned, never 0 for a layout that is
 * accepted; the copy has completed when the call returns).  neg_run: C (0 = the built-in choice, at most 2^24; a test seam —
 * no count depends on it).  Refused (MI_ERR_INVALID; a short table MI_ERR_WORKSPACE; more than 2^24 items
 * MI_ERR_UNSUPPORTED), writing neither device_table nor *plan: NULL seg_off / seg_neg / device_table / plan,
 * n_segments < 1, seg_off not ascending from 0 to N, seg_neg[s] outside [0, its segment's size], N < 1 or N >= 2^31,
 * neg_run out of range.  mi_auc_plan_bytes returns 0 for a layout mi_auc_plan refuses.
 *
 * mi_auc_pair_counts: ONE launch, grid (items, members); no copy, no synchronisation, no workspace.
 *   logits: member m's logit of example i at logits[m * member_stride + i] (member_stride >= N);
 *   order [N]: as above.  PRECONDITION: every entry in [0, N) — the entry cannot look at device memory;
 *   counts [M, S, 2] int64, ZEROED BY THE CALLER: [m, s, 0] += the pairs of segment s with key_pos > key_neg,
 *     [m, s, 1] += those with equal keys (64-bit integer atomic adds, one per wave and counter: a second call into the same
 *     buffer adds the same numbers again).
 * Two calls on equal input give equal bits.  No workgroup reads what another writes and none waits for another.
 * Refused on the host before anything is launched (MI_ERR_INVALID): a plan mi_auc_plan did not write, NULL logits / order /
 * counts, n_members outside [1, MI_AUC_MAX_MEMBERS], member_stride < N. */
#define MI_AUC_MAX_MEMBERS 1024
typedef struct mi_auc_plan {
  void* device_table;
  uint64_t magic;
  int64_t N;
  int32_t n_segments, n_items;
} mi_auc_plan_t;
size_t mi_auc_plan_bytes(const int64_t* seg_off, const int64_t* seg_neg, int32_t n_segments, int32_t neg_run);
int32_t mi_auc_plan(const int64_t* seg_off, const int64_t* seg_neg, int32_t n_segments, int32_t neg_run, void* device_table,
                    size_t device_table_bytes, mi_auc_plan_t* plan, mi_stream_t stream);
int32_t mi_auc_pair_counts(const mi_auc_plan_t* plan, const float* logits, int64_t member_stride, int32_t n_members,
                           const int32_t* order, int64_t* counts, mi_stream_t stream);

/* ---- the same counts at any evaluation size: sort the examples, count the tie runs (csrc/auc_sort.hip) -------------------
 * mi_auc_sorted_counts gives exactly mi_auc_pair_counts' integers in O(N log N) per member, from labels and groups that lie
 * on the device in the examples' own order: no `order`, no plan, no host layout — what an evaluation loop that meets its
 * data batch by batch can provide.
 *   logits: member m's logit of example i at logits[m * member_stride + i] (member_stride >= N);
 *   labels [N] uint8 (device): positive when non-zero;
 *   groups [N] int32 (device), or NULL with n_groups = 1 (the global AUC): example i's group in [0, n_groups).  An example
 *     whose group lies outside that range is IGNORED (the kernels check: it never causes a write outside counts);
 *   counts [M, S, 2] int64 (S = n_groups), ZEROED BY THE CALLER: [m, s, 0] += the (positive, negative) pairs of group s
 *     with key_pos > key_neg, [m, s, 1] += those with equal keys — the key of csrc/score_key.h, as above (64-bit integer
 *     atomic adds, summed inside a workgroup first: one add per counter, tile of 4,096 sorted examples and group in it;
 *     a second call into the same buffer adds the same numbers again);
 *   workspace: mi_auc_sorted_workspace_bytes(N, n_groups) bytes of device memory, 16-byte aligned (0 for arguments the
 *     entry refuses: N < 1, N >= 2^31, n_groups < 1).  The members are taken one after another on the stream inside the
 *     call and reuse it in stream order.
 * Per member: every example becomes one 64-bit word group : key : label; a stable LSD radix sort of the words over the
 * 33 + ceil(log2 S) bits in use (digits of at most 9 bits: 4 passes for the global AUC; three short launches per pass);
 * then for every tie run r of a group (equal group and key) with P_r positives and N_r negatives, gt += P_r x (the
 * group's negatives in earlier runs), eq += P_r x N_r, by head flags and segmented scans (three launches).
 * Two calls on equal input give equal bits, whatever the tile count.  No workgroup reads what another writes inside a
 * launch and none waits for another; no library but HIP.
 * Refused on the host before anything is launched, writing nothing — MI_ERR_INVALID: NULL logits / labels / counts /
 * workspace, N < 1 or N >= 2^31, n_groups < 1, groups == NULL with n_groups != 1, n_members outside
 * [1, MI_AUC_MAX_MEMBERS], member_stride < N, a workspace that is not 16-byte aligned; MI_ERR_WORKSPACE: a short workspace. */
size_t mi_auc_sorted_workspace_bytes(int64_t N, int32_t n_groups);
int32_t mi_auc_sorted_counts(const float* logits, int64_t member_stride, int32_t n_members, const uint8_t* labels,
                             const int32_t* groups, int32_t n_groups, int64_t N, int64_t* counts, void* workspace,
                             size_t workspace_bytes, mi_stream_t stream);

/* ---- (a1) categorical id transforms on the device: raw feature columns to row ids in one launch (csrc/ids.hip) ----------
 * The device form of the host entries above (the column constructors of trainers/ml_100k.py:19-35):
 * F raw columns of B values become ids int32 [B, ld] (ld >= F; columns F..ld-1 and rows past B are not touched) in the
 * plan's field order.  Integer work only; every id equals what the matching host definition gives.
 *
 * mi_ids_column_t describes one column.  The table of F descriptors lies in HOST memory and travels in the kernel's
 * arguments: the entry makes no allocation, no copy and no synchronisation, and can be captured in a graph.
 *   MI_IDS_HASH_I64 / _I32   values int64 / int32 [B]: Fingerprint64 of the value's decimal ASCII ('-' for negatives, as
 *                            "%lld" prints them) mod num_buckets — mi_hash_bucket_i64;
 *   MI_IDS_HASH_BYTES        values uint8 (the strings, back to back), offsets int64 [B + 1]: Fingerprint64 of
 *                            values[offsets[i] : offsets[i+1]] mod num_buckets — mi_hash_bucket_bytes.  Any length;
 *   MI_IDS_BUCKETIZE_F32     values float [B], table = n_table boundaries (float, device), table_host = the same
 *                            boundaries in host memory (the entry cannot look at device memory: it checks these): the
 *                            number of boundaries <= x, NaN -> 0 — mi_bucketize_f32;
 *   MI_IDS_VOCAB_BYTES       values / offsets as MI_IDS_HASH_BYTES, table = the vocabulary table of n_table entries (below):
 *                            the entry's list index; a value not in the list gives n_table + Fingerprint64 % num_oov, or
 *                            default_value when num_oov == 0;
 *   MI_IDS_IDENTITY_I64/_I32 values int64 / int32 [B]: the value itself, or default_value when it is outside
 *                            [0, num_buckets).
 * The vocabulary table, built by the host once per plan, is ONE block of device memory, 8-byte aligned, n = n_table:
 *   uint64 fingerprint[n]   the entries' Fingerprint64, ascending;
 *   int64  start[n + 1]     entry j's bytes are text[start[j] : start[j+1]];
 *   int32  index[n]         entry j's position in the vocabulary list (followed by 4 bytes of padding when n is odd);
 *   uint8  text[]           the entries' bytes in the fingerprints' order.
 * A value is looked up by a binary search on its fingerprint, then a comparison of the bytes of every entry that carries
 * that fingerprint (a fingerprint match alone is not the contract), then the index.
 * PRECONDITION of the two bytes kinds: wherever 0 <= offsets[i] <= offsets[i+1], offsets[i+1] is at most the length of
 * `values` — the entry cannot look at device memory.  No byte outside a string's own range is read.
 *
 * A BAD value is one whose id would be < 0 or >= num_buckets (a vocabulary miss with default -1, an identity value out of
 * range whose default_value is out of range too — -1 stands for "no default" —, offsets[i+1] < offsets[i] or
 * offsets[i] < 0).  No id outside [0, num_buckets) is ever stored: for a bad value of column f the kernel stores id 0, adds 1
 * to status[2 f] and takes the maximum of 2^31 - 1 - i into status[2 f + 1], i the example's index: in a status the caller
 * ZEROED, 2^31 - 1 - status[2 f + 1] is the lowest bad example of column f where status[2 f] > 0.  status: int32 [F, 2]
 * (device); integer atomics, so the result does not depend on order.  Two calls on equal input give equal bits.  No
 * workgroup reads what another writes and none waits for another.  The mod is exact for every 64-bit fingerprint and
 * every num_buckets in [1, 2^31 - 1].
 * Refused on the host before anything is launched, ids and status untouched, the message naming the column's index
 * (MI_ERR_INVALID): NULL columns / ids / status, F outside [1, MI_IDS_MAX_COLUMNS], B outside [1, 2^31 - 1], ld < F, an
 * unknown kind, NULL values, NULL offsets of a bytes kind, num_buckets outside [1, 2^31 - 1], n_table < 0, NULL table or
 * table_host with n_table > 0, boundaries that are not strictly increasing or more than num_buckets - 1 of them, a
 * vocabulary of n_table < 1 entries or with n_table + num_oov > num_buckets, num_oov < 0.
 *
 * mi_fingerprint64_device: out[i] = Fingerprint64(bytes[offsets[i] : offsets[i+1]]) for i < n, raw, uint64 [n] (device).
 * A range with offsets[i+1] < offsets[i] or offsets[i] < 0 counts as the empty string.  One launch; refused
 * (MI_ERR_INVALID): n outside [1, 2^31 - 1], NULL offsets / out. */
#define MI_IDS_MAX_COLUMNS 64
enum mi_ids_kind {
  MI_IDS_HASH_I64 = 0,
  MI_IDS_HASH_I32 = 1,
  MI_IDS_HASH_BYTES = 2,
  MI_IDS_BUCKETIZE_F32 = 3,
  MI_IDS_VOCAB_BYTES = 4,
  MI_IDS_IDENTITY_I64 = 5,
  MI_IDS_IDENTITY_I32 = 6
};
typedef struct mi_ids_column {
  const void* values;
  const int64_t* offsets;
  const void* table;
  const float* table_host;
  int32_t kind, num_buckets, n_table, num_oov, default_value, reserved;
} mi_ids_column_t;
int32_t mi_ids_transform(const mi_ids_column_t* columns, int32_t F, int64_t B, int32_t* ids, int64_t ld, int32_t* status,
                         mi_stream_t stream);
int32_t mi_fingerprint64_device(const uint8_t* bytes, const int64_t* offsets, int64_t n, uint64_t* out, mi_stream_t stream);

/* ---- (a2) one batch out of a dataset that lives on the device, by an index stream, in one launch (csrc/batch.hip) -------
 * The resident arrays are ids_all int32 [N, ld_ids] (ld_ids >= F), x_all float [N, ld_x] (ld_x >= n_num) and y_all uint8
 * [N]; order int32 [B] names the rows of the batch (the caller passes the pointer already offset into its pass stream;
 * an index may repeat).  The outputs are DENSE:
 *   ids[b, f] = ids_all[order[b] * ld_ids + f]    f < F        int32 [B, F]
 *   x  [b, j] = x_all  [order[b] * ld_x   + j]    j < n_num    float [B, n_num]   (n_num may be 0: x_all and x NULL)
 *   y  [b]    = y_all  [order[b]]                              uint8 [B]          (y_all and y both NULL: no labels)
 * Everything is on the device.  The entry makes no allocation, no copy and no synchronisation, and can be captured in a
 * graph.  No workgroup reads what another writes and none waits for another.
 *
 * A BAD index is order[b] < 0 or order[b] >= N.  The kernel never forms an address from it: it stores a zero row (ids
 * and x) and label 0, adds 1 to status[0] and takes the maximum of 2^31 - 1 - b into status[1] — mi_ids_transform's
 * convention: in a status the caller ZEROED, 2^31 - 1 - status[1] is the lowest bad position where status[0] > 0.  status:
 * int32 [2] (device); integer atomics only, so the result does not depend on order.  Two calls on equal input give equal
 * bits.
 * Refused on the host before anything is launched, the outputs and status untouched, the message naming the argument
 * (MI_ERR_INVALID): NULL ids_all / order / ids / status, N or B outside [1, 2^31 - 1], F outside [1, MI_IDS_MAX_COLUMNS],
 * ld_ids < F, n_num < 0, n_num > 0 with NULL x_all / x or ld_x < n_num, exactly one of y_all / y NULL. */
int32_t mi_batch_gather(const int32_t* ids_all, int64_t ld_ids, const float* x_all, int64_t ld_x, const uint8_t* y_all, int64_t N,
                        const int32_t* order, int64_t B, int32_t F, int32_t n_num, int32_t* ids, float* x, uint8_t* y,
                        int32_t* status, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REC_H */
