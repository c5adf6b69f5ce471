// gemm_wgrad_pl.inc — included by gemm.hip inside its anonymous namespace (after gemm_split.inc).
//
// Weight gradient dW[K][N] = X^T dY (model_utils.py:69-72: optimizer.minimize's gradients of tf.layers.dense,
// deep_fm.py:98-108) with BOTH operands read as the 16-bit high/low planes the forward pass and the data
// gradient already wrote (csrc/gemm_pl.hip), instead of fp32 copies split again in the loop.
//
// The reduction runs over the examples, and a plane row carries its own exponent, so the planes cannot be
// multiplied as they are: example m's products carry 2^(sx[m] + sy[m]).  One power of two per example,
//     2^d[m],  d[m] = (SX - sx[m]) + (SY - sy[m]) <= 0      (SX, SY: the exponents of the matrix abs-max)
// shared out over the two operands (wgrad_scale_k) and applied with v_pk_mul_f16 — exact unless the result is
// subnormal — brings every example to the matrix-wide scales 2^(SX + SY): the products gemm_split_k<f16x2>
// forms from fp32 operands, up to the low bits of examples far below the abs-max, which are invisible in a sum
// over examples (they go subnormal; the MFMA keeps fp16 subnormals).
//
// Same tile, LDS layout, fragment reads, MFMA order, split-K slabs and epilogue as gemm_split_k<F16X2, MC, MC>;
// what changes is the staging: 16-byte loads of eight features x one example of one plane (a wave instruction
// reads whole 512-byte runs of rows), the scale, an 8 x 4 transpose of 16-bit values with v_perm_b32 (the examples
// become the k-contiguous dimension), 8-byte LDS stores.  About 50 VALU per thread and k-tile instead of 128: the loop is bound by the matrix pipe.
// The bias gradient (column sums of dY) rides in the tm == 0 blocks as before, from hi * 2^-sy and lo * 2^-sy.

struct WgPlArgs {
  const char* A; int64_t bsa;         // X planes: [K / 16][examples][64 B]
  const char* B; int64_t bsb;         // dY planes: [N / 16][examples][64 B]
  const uint32_t* scw;                // [examples, slot order] the X rows' factor 2^a as two f16
  const uint32_t* scy;                // [examples, slot order] the dY rows' factor 2^b as two f16
  const float* yf;                    // [examples, slot order] 2^-sy[m] (bias gradient)
  GemmArgs g;                         // C = slab, ldc, M = K (features), N, K = examples, tiles, k_per_split, colsum_part, amax_a / amax_b
};

constexpr int W_PLANE = S_PLANE + 64;

__device__ __forceinline__ uint32_t w_pow2_f16_bits(int d) {      // 2^d, d <= 0: normal down to 2^-14, subnormal down to 2^-24, zero below
  return d >= -14 ? static_cast<uint32_t>(15 + d) << 10 : (d >= -24 ? 1u << (d + 24) : 0u);
}
// per-example factors, once per call.  Example m needs 2^d, d = (SX - sx[m]) + (SY - sy[m]) <= 0, on its products.
// An f16 factor reaches down to 2^-24 only, so d is shared out over the two operands: 2^a on the X rows, 2^b on
// the dY rows, a + b = d, zero below d = -38 (what a direct fp16 conversion at matrix-wide scales loses as well).
//   gemm_wgrad_pl_k: a = max(d, -14); packed pairs in the slot order of its k-tiles (scw, scy) plus 2^-sy[m] in
//                    fp32 (yf, bias gradient);
//   wgrad_pl_k (wgrad_pl.hip): a = max(d, -24), so that b != 0 is rare; f16 in example order: sx16 = 2^a,
//                    sy16 = 2^b, sc16 = 2^(SY - sy[m]) (bias gradient); kflag[m / 16] != 0 where one of the 16
//                    examples of a k-step has b != 0 (the kernel multiplies the dY fragments only there).
// (round 4: the factors of ALL the layers whose weight gradients a backward pass takes from planes are made by one launch —
// mi_dense_bwd_weight_planes_batch; a job per layer, blocks [block0, block0 + ceil(M / 256)) are the job's)
struct WgScaleJob {
  const int32_t* x_exp; const int32_t* y_exp; const float* amax_a; const float* amax_b; int64_t M;
  uint32_t* scw; uint32_t* scy; float* yf; uint16_t* sx16; uint16_t* sy16; uint16_t* sc16; int32_t* kflag;
  int block0;
};
struct WgScaleJobs { WgScaleJob j[MI_MAX_WEIGHT_JOBS]; int n; };

__device__ __forceinline__ void wgrad_scale_body(const int32_t* __restrict__ x_exp, const int32_t* __restrict__ y_exp,
                                                 const float* __restrict__ amax_a, const float* __restrict__ amax_b,
                                                 int64_t M, uint32_t* __restrict__ scw, uint32_t* __restrict__ scy,
                                                 float* __restrict__ yf, uint16_t* __restrict__ sx16,
                                                 uint16_t* __restrict__ sy16, uint16_t* __restrict__ sc16,
                                                 int32_t* __restrict__ kflag, int64_t m) {
  if (m >= M) return;
  const int SX = pl_scale_exp(amax_a), SY = pl_scale_exp(amax_b);
  const int sy = y_exp[m];
  const int dy = min(0, SY - sy);
  const int d = min(0, SX - x_exp[m]) + dy;
  if (sx16) {
    const int a = max(d, -24), b = d - a;
    sx16[m] = static_cast<uint16_t>(w_pow2_f16_bits(a));
    sy16[m] = static_cast<uint16_t>(b >= -14 ? w_pow2_f16_bits(b) : 0u);
    sc16[m] = static_cast<uint16_t>(w_pow2_f16_bits(dy));
    // one flag per 16 consecutive examples = 16 consecutive lanes (M is a multiple of 16: groups are whole)
    const unsigned long long any = __ballot(b != 0);
    const int lane = threadIdx.x & 63;
    if ((lane & 15) == 0) kflag[m >> 4] = ((any >> lane) & 0xffffull) != 0 ? 1 : 0;
    return;
  }
  const int a = max(d, -14), b = d - a;
  const uint32_t bx = w_pow2_f16_bits(a), by = w_pow2_f16_bits(b);
  // slot order of a 32-example k-tile (see the staging map of gemm_wgrad_pl_k): example q + 8 j -> slot 4 q + j
  const int e = static_cast<int>(m & 31);
  const int64_t slot = (m & ~int64_t(31)) + 4 * (e & 7) + (e >> 3);
  scw[slot] = bx | (bx << 16);
  scy[slot] = by | (by << 16);
  yf[slot] = pl_pow2(-sy);
}

__global__ __launch_bounds__(kThreads) void wgrad_scale_k(const WgScaleJobs js) {
  int ji = 0;
#pragma unroll
  for (int q = 1; q < MI_MAX_WEIGHT_JOBS; ++q)
    if (q < js.n && static_cast<int>(blockIdx.x) >= js.j[q].block0) ji = q;
  const WgScaleJob& jb = js.j[ji];
  const int64_t m = static_cast<int64_t>(static_cast<int>(blockIdx.x) - jb.block0) * kThreads + threadIdx.x;
  wgrad_scale_body(jb.x_exp, jb.y_exp, jb.amax_a, jb.amax_b, jb.M, jb.scw, jb.scy, jb.yf, jb.sx16, jb.sy16, jb.sc16, jb.kflag, m);
}

template <bool COLSUM>
__global__ __launch_bounds__(kThreads, 2) void gemm_wgrad_pl_k(const WgPlArgs wa) {
  const GemmArgs& a = wa.g;
  // [operand][plane][row][80 B]; the low plane starts 64 B further (W_PLANE): the 16 lanes of a ds_write_b64
  // group — 8 example quads x 2 planes — then cover all 32 banks
  __shared__ __attribute__((aligned(16))) char smem[2][2 * W_PLANE];

  const int nb = gridDim.x, bid = blockIdx.x;
  const int qq = nb >> 3, rr = nb & 7, xcd = bid & 7, idx = bid >> 3;
  const int lid = (xcd < rr) ? xcd * (qq + 1) + idx : rr * (qq + 1) + (xcd - rr) * qq + idx;
  const int tn = lid % a.tiles_n;
  const int tm = (lid / a.tiles_n) % a.tiles_m;
  const int split = lid / (a.tiles_n * a.tiles_m);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = split * a.k_per_split;
  const int kend = min(a.K, kbeg + a.k_per_split);
  const int nk = (kend - kbeg + BK - 1) / BK;
  const int klast = kbeg + (nk - 1) * BK;          // loads past the last tile re-read it

  const int t = threadIdx.x;
  const int w = t >> 6, lane = t & 63;
  const int wm = w >> 1, wn = w & 1;
  const int i = lane & 31, h = lane >> 5;

  const int sa = pl_scale_exp(a.amax_a), sb = pl_scale_exp(a.amax_b);

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const bool do_colsum = COLSUM && a.colsum_part != nullptr && tm == 0;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // Staging map.  A k-tile of one operand is 8 feature blocks x 32 examples x 64 B; thread t owns one 16-byte
  // piece of a row (pl = t & 1: high / low plane, half = (t >> 4) & 1: features 0-7 / 8-15 of the block), block
  // t >> 5, and the four examples q + 8 j (q = (t >> 1) & 7, j = 0..3).  One load instruction of a wave then
  // reads 8 consecutive rows = 512 contiguous bytes per block.  The examples of a k-tile sit in LDS in the order
  // slot 4 q + j <-> example q + 8 j — the same permutation for both operands, so the products still pair up
  // (wgrad_scale_k writes the per-example factors in slot order).
  const int pl = t & 1, q = (t >> 1) & 7, half = (t >> 4) & 1, blk = t >> 5;
  const int c = pl * 2 + half;                     // 16-byte piece of the 64-byte row
  uint32_t oa[4], ob[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    oa[j] = static_cast<uint32_t>(blk * wa.bsa + (q + 8 * j) * 64 + c * 16);
    ob[j] = static_cast<uint32_t>(blk * wa.bsb + (q + 8 * j) * 64 + c * 16);
  }
  const char* abase = wa.A + static_cast<int64_t>(m0 >> 4) * wa.bsa;
  const char* bbase = wa.B + static_cast<int64_t>(n0 >> 4) * wa.bsb;

  uint4 ra[4], rb[4];
  uint4 rsc, rsy, rye = make_uint4(0u, 0u, 0u, 0u);
  auto load_tile = [&](int k0) {
    const int kc = min(k0, klast);
    const char* ta = abase + static_cast<int64_t>(kc) * 64;
    const char* tb = bbase + static_cast<int64_t>(kc) * 64;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ra[j] = *reinterpret_cast<const uint4*>(ta + oa[j]);
      rb[j] = *reinterpret_cast<const uint4*>(tb + ob[j]);
    }
    rsc = *reinterpret_cast<const uint4*>(wa.scw + kc + 4 * q);
    rsy = *reinterpret_cast<const uint4*>(wa.scy + kc + 4 * q);
    if (COLSUM && do_colsum) rye = *reinterpret_cast<const uint4*>(wa.yf + kc + 4 * q);
  };
  auto mul2 = [](uint32_t x, uint32_t s) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, x) * __builtin_bit_cast(h16x2, s));
  };
  // eight features x four examples (one uint4 per example) -> per feature the four examples (8 bytes, one LDS row each)
  auto put = [&](char* d, const uint4 (&r)[4]) {
    constexpr uint32_t LO = 0x05040100u, HI = 0x07060302u;
#define MI_PUT(wi, F)                                                                                                     \
    *reinterpret_cast<uint2*>(d + (2 * wi) * S_ROWB) =                                                                   \
        make_uint2(__builtin_amdgcn_perm(r[1].F, r[0].F, LO), __builtin_amdgcn_perm(r[3].F, r[2].F, LO));                \
    *reinterpret_cast<uint2*>(d + (2 * wi + 1) * S_ROWB) =                                                               \
        make_uint2(__builtin_amdgcn_perm(r[1].F, r[0].F, HI), __builtin_amdgcn_perm(r[3].F, r[2].F, HI));
    MI_PUT(0, x) MI_PUT(1, y) MI_PUT(2, z) MI_PUT(3, w)
#undef MI_PUT
  };
  const int srow = (blk * 16 + half * 8) * S_ROWB + pl * W_PLANE + q * 8;
  auto stage = [&]() {
    const uint32_t sw[4] = {rsc.x, rsc.y, rsc.z, rsc.w}, yw[4] = {rsy.x, rsy.y, rsy.z, rsy.w};
    uint4 xa[4], xb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xa[j] = make_uint4(mul2(ra[j].x, sw[j]), mul2(ra[j].y, sw[j]), mul2(ra[j].z, sw[j]), mul2(ra[j].w, sw[j]));
      xb[j] = make_uint4(mul2(rb[j].x, yw[j]), mul2(rb[j].y, yw[j]), mul2(rb[j].z, yw[j]), mul2(rb[j].w, yw[j]));
    }
    put(smem[0] + srow, xa);
    put(smem[1] + srow, xb);
    if (COLSUM && do_colsum) {
      const float yf[4] = {__uint_as_float(rye.x), __uint_as_float(rye.y), __uint_as_float(rye.z), __uint_as_float(rye.w)};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t wv[4] = {rb[j].x, rb[j].y, rb[j].z, rb[j].w};
#pragma unroll
        for (int wi = 0; wi < 4; ++wi) {
          const h16x2 v = __builtin_bit_cast(h16x2, wv[wi]);
          cs[2 * wi] += static_cast<float>(v[0]) * yf[j];
          cs[2 * wi + 1] += static_cast<float>(v[1]) * yf[j];
        }
      }
    }
  };
  const char* Ar = smem[0] + (wm * 64 + i) * S_ROWB + h * 16;
  const char* Br = smem[1] + (wn * 64 + i) * S_ROWB + h * 16;
  f16x8 fa[2][2][2], fb[2][2][2];               // [ks][mi|ni][plane]
  auto read_frags = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          fa[ks][mi][p] = *reinterpret_cast<const f16x8*>(Ar + p * W_PLANE + mi * 32 * S_ROWB + ks * 32);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          fb[ks][ni][p] = *reinterpret_cast<const f16x8*>(Br + p * W_PLANE + ni * 32 * S_ROWB + ks * 32);
    }
  };
  auto mfma_tile = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          f32x16 c = acc[mi][ni];              // smallest partial products first
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][mi][1], fb[ks][ni][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][mi][0], fb[ks][ni][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][mi][0], fb[ks][ni][0], c, 0, 0, 0);
          acc[mi][ni] = c;
        }
  };

  // the pipeline of gemm_split_k: tile t's fragments in registers under its MFMAs, the staging of tile t + 1
  // and the global loads of tile t + 2 issued in the gaps between them; branch-free
  if (nk > 0) {
    load_tile(kbeg);
    stage();
    __syncthreads();
    read_frags();
    load_tile(kbeg + BK);
    __syncthreads();
  }
  for (int kt = 0; kt + 1 < nk; ++kt) {
    mfma_tile();
    stage();
    load_tile(kbeg + (kt + 2) * BK);
#pragma unroll
    for (int g = 0; g < 24; ++g) {             // 1 MFMA, then a few VALU, 1 LDS store, 1 global load
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, COLSUM ? 6 : 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
    __syncthreads();
    read_frags();
    __syncthreads();
  }
  if (nk > 0) mfma_tile();

  if (COLSUM && do_colsum) {     // 16 partial sums per column (plane x example group): fold in a fixed order
    float* red = reinterpret_cast<float*>(&smem[0][0]);
    __syncthreads();
    float* d = red + (pl * 8 + q) * BN + blk * 16 + half * 8;
#pragma unroll
    for (int f = 0; f < 8; ++f) d[f] = cs[f];
    __syncthreads();
    if (t < BN) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) v += red[g * BN + t];
      if (n0 + t < a.N) a.colsum_part[static_cast<int64_t>(split) * a.N + n0 + t] = v;
    }
  }
  store_tile_c(a, acc, m0, n0, wm, wn, i, h, split, pl_pow2(-sa), pl_pow2(-sb));
}
