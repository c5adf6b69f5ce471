// gemm_split.inc — included by gemm.hip inside its anonymous namespace.
//
// fp32 GEMM on the 16-bit matrix pipe by an operand split.  On CDNA4 the fp32-input MFMA runs at
// 1/16 of the bf16/f16 rate, so a few 16-bit products per fp32 product win.  A product of two
// 16-bit floats is exact in fp32 and the MFMAs accumulate in fp32, so what is lost is only what
// the split drops:
//
//   FMT_F16X2   x * 2^s = h + l, h and l fp16 (RNE; x*2^s - h is exact in fp32), three products
//               a*b = ah*bh + ah*bl + al*bh  (dropped: al*bl and the two residuals, <= 2^-21 |ab|).
//               fp16 has 5 exponent bits, so each operand is scaled by a power of two that puts its
//               largest magnitude into [2^14, 2^15) — exact to apply and to undo.  The caller passes
//               the operands' abs-max (device memory, written by the kernel that produced the
//               operand: every epilogue here can emit it); elements more than 2^-29 below the
//               largest lose low bits, which is invisible in a dot product.  3 MFMAs per k-step.
//   FMT_BF16X3  x = x1 + x2 + x3, bf16 (8 significant bits each, fp32 exponent range: no scale
//               needed, any input), six products with i + j <= 4 (dropped: <= 3 * 2^-24 |ab|).
//               Taken when the caller has no abs-max for an operand.
//
// Both measure the same max error against fp64 as v_mfma_f32_32x32x2_f32 on the layer shapes
// (accumulation order dominates; tools/gemm_bench.py).
//
// The loop is bound by VALU issue, not by the matrix pipe, unless the split is lean: an MFMA
// 32x32x16 occupies its SIMD's matrix pipe for 32 cycles and holds vector issue for 8 of them;
// both waves of a SIMD share the remaining 24 (six single-issue instructions per MFMA).  The f16x2
// loop has 24 MFMAs per wave and k-tile, so about 140 other instructions fit.  Hence:
//   * EDGE = false kernels for whole tiles (every config-3 shape): no predicates, no zero selects,
//     loop-invariant 32-bit lane offsets from a uniform tile base (one SALU add per k-tile);
//   * the split itself is 8 VALU per pair of values (2 scale, 2 cvt_pk, 2 cvt back, 2 sub);
//   * the gathered operand's row address is one v_mad_u64_u32 per row.
// EDGE = true keeps the predicated, any-shape form.
//
// Staging: operands go HBM -> registers -> split -> LDS planes ([plane][128 rows][32 k + pad] 16-bit,
// k contiguous: every fragment is one ds_read_b128); mn-contiguous operands (weight gradient:
// k = batch) are transposed in registers in 4x4 micro-tiles so both layouts read LDS the same way.
// One LDS buffer, two workgroups per CU; tile t's fragments sit in registers while its MFMAs run,
// the split + LDS stores of tile t+1 and the global loads of tile t+2 are issued between them.

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 s_bf16x2 __attribute__((ext_vector_type(2)));

enum { FMT_BF16X3 = 0, FMT_F16X2 = 1 };
template <int FMT> struct SplitFmt { static constexpr int NPL = (FMT == FMT_BF16X3) ? 3 : 2; };

constexpr int S_ROWB = 80;                 // LDS bytes per row: 32 x 16 bit + 16 B pad (ds_read_b128 conflict-free)
constexpr int S_PLANE = BM * S_ROWB;       // 10,240 B per plane

__device__ __forceinline__ uint32_t s_pk(float a, float b) {
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, s_bf16x2));   // v_cvt_pk_bf16_f32, RNE
}
__device__ __forceinline__ float s_lo(uint32_t p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float s_hi(uint32_t p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// four k-consecutive values -> NPL planes of 4 x 16 bit (8 bytes each) at d, d + PLANE, ...
template <int FMT>
__device__ __forceinline__ void s_split_store(char* __restrict__ d, float x0, float x1, float x2, float x3, float sc) {
  if constexpr (FMT == FMT_F16X2) {
    x0 *= sc; x1 *= sc; x2 *= sc; x3 *= sc;
    const f32x2 v01 = {x0, x1}, v23 = {x2, x3};
    const h16x2 h01 = __builtin_convertvector(v01, h16x2), h23 = __builtin_convertvector(v23, h16x2);  // v_cvt_pk_f16_f32
    const f32x2 r01 = {x0 - static_cast<float>(h01[0]), x1 - static_cast<float>(h01[1])};
    const f32x2 r23 = {x2 - static_cast<float>(h23[0]), x3 - static_cast<float>(h23[1])};
    const h16x2 l01 = __builtin_convertvector(r01, h16x2), l23 = __builtin_convertvector(r23, h16x2);
    uint2 p1, p2;
    p1.x = __builtin_bit_cast(uint32_t, h01); p1.y = __builtin_bit_cast(uint32_t, h23);
    p2.x = __builtin_bit_cast(uint32_t, l01); p2.y = __builtin_bit_cast(uint32_t, l23);
    *reinterpret_cast<uint2*>(d) = p1;
    *reinterpret_cast<uint2*>(d + S_PLANE) = p2;
  } else {
    uint2 p1, p2, p3;
    p1.x = s_pk(x0, x1); p1.y = s_pk(x2, x3);
    const float r0 = x0 - s_lo(p1.x), r1 = x1 - s_hi(p1.x), r2 = x2 - s_lo(p1.y), r3 = x3 - s_hi(p1.y);
    p2.x = s_pk(r0, r1); p2.y = s_pk(r2, r3);
    const float q0 = r0 - s_lo(p2.x), q1 = r1 - s_hi(p2.x), q2 = r2 - s_lo(p2.y), q3 = r3 - s_hi(p2.y);
    p3.x = s_pk(q0, q1); p3.y = s_pk(q2, q3);
    *reinterpret_cast<uint2*>(d) = p1;
    *reinterpret_cast<uint2*>(d + S_PLANE) = p2;
    *reinterpret_cast<uint2*>(d + 2 * S_PLANE) = p3;
  }
}

// thread -> (micro-tile column group nq 0..31, batch quad q 0..7) for mn-contiguous operands: four
// neighbouring lanes read 64 contiguous bytes of one row, a wave-instruction covers 8 rows x 128 B
__device__ __forceinline__ void s_mc_map(int t, int& nq, int& q) {
  const int lane = t & 63, w = t >> 6;
  nq = (lane & 3) + 4 * ((lane >> 5) + 2 * w);
  q = (lane >> 2) & 7;
}

// ======================================================================================
// EDGE = true: any shape.  Branch-free predicated loads (out-of-range slots read the buffer's
// first element and are zeroed just before the LDS store).
// ======================================================================================
template <int L>
__device__ __forceinline__ void s_load(const float* __restrict__ P, int64_t ld, int MN, int mn0, int k0, int kend,
                                       float4 (&r)[4], int t) {
  if constexpr (L == KC) {
    const int kk = k0 + (t & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int mn = mn0 + (t >> 3) + 32 * p;
      const bool ok = mn < MN && kk < kend;
      r[p] = *reinterpret_cast<const float4*>(ok ? P + static_cast<int64_t>(mn) * ld + kk : P);
    }
  } else {
    int nq, q;
    s_mc_map(t, nq, q);
    const int mn = mn0 + 4 * nq;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int kk = k0 + 4 * q + p;
      const bool ok = kk < kend && mn < MN;
      r[p] = *reinterpret_cast<const float4*>(ok ? P + static_cast<int64_t>(kk) * ld + mn : P);
    }
  }
}

// rows of the gathered A operand for the tile at k0 (fetched one tile ahead, see gemm_f32_k)
template <int L>
__device__ __forceinline__ void s_gather_rows(const GemmArgs& a, int MN, int mn0, int k0, int kend, int (&row)[4],
                                              int t) {
  if constexpr (L == KC) {
    const int kk = k0 + (t & 7) * 4;
    const bool k_ok = kk < kend;
    const int f = k_ok ? kk / a.g_E : 0;
    const int64_t off = a.g_off[f];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int m = mn0 + (t >> 3) + 32 * p;
      row[p] = static_cast<int>(off + a.g_ids[(k_ok && m < MN) ? static_cast<int64_t>(m) * a.g_F + f : 0]);
    }
  } else {
    int nq, q;
    s_mc_map(t, nq, q);
    const int mn = mn0 + 4 * nq;
    const bool m_ok = mn < MN;
    const int f = m_ok ? mn / a.g_E : 0;
    const int64_t off = a.g_off[f];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int b = k0 + 4 * q + p;
      row[p] = static_cast<int>(off + a.g_ids[(m_ok && b < kend) ? static_cast<int64_t>(b) * a.g_F + f : 0]);
    }
  }
}

template <int L>
__device__ __forceinline__ void s_load_gathered(const GemmArgs& a, int mn0, int k0, const int (&row)[4],
                                                float4 (&r)[4], int t) {
  int c;
  if constexpr (L == KC) {
    c = k0 + (t & 7) * 4;
  } else {
    int nq, q;
    s_mc_map(t, nq, q);
    c = mn0 + 4 * nq;
  }
  const int e = c % a.g_E;
#pragma unroll
  for (int p = 0; p < 4; ++p)
    r[p] = *reinterpret_cast<const float4*>(a.A + static_cast<int64_t>(row[p]) * a.g_ts + e);
}

// registers -> planes in LDS.  EDGE zero-fills what lies outside the matrix.  COLSUM adds the
// staged values of the mn-contiguous operand into cs (column sums over k, for the bias gradient).
template <int FMT, int L, bool COLSUM, bool EDGE>
__device__ __forceinline__ void s_stage(char* __restrict__ S, int MN, int mn0, int k0, int kend,
                                        const float4 (&r)[4], int t, float sc, float4& cs) {
  if constexpr (L == KC) {
    const int kk = k0 + (t & 7) * 4;
    char* d = S + (t >> 3) * S_ROWB + (t & 7) * 8;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float4 x = r[p];
      if constexpr (EDGE) {
        const bool ok = mn0 + (t >> 3) + 32 * p < MN && kk < kend;
        x = ok ? x : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      s_split_store<FMT>(d + 32 * p * S_ROWB, x.x, x.y, x.z, x.w, sc);
    }
  } else {
    int nq, q;
    s_mc_map(t, nq, q);
    float4 x[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      x[p] = r[p];
      if constexpr (EDGE) x[p] = (k0 + 4 * q + p < kend && mn0 + 4 * nq < MN) ? x[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (COLSUM) {
#pragma unroll
      for (int p = 0; p < 4; ++p) { cs.x += x[p].x; cs.y += x[p].y; cs.z += x[p].z; cs.w += x[p].w; }
    }
    char* d = S + (4 * nq) * S_ROWB + q * 8;        // transposed: row = column of the source, k = source row
    s_split_store<FMT>(d, x[0].x, x[1].x, x[2].x, x[3].x, sc);
    s_split_store<FMT>(d + S_ROWB, x[0].y, x[1].y, x[2].y, x[3].y, sc);
    s_split_store<FMT>(d + 2 * S_ROWB, x[0].z, x[1].z, x[2].z, x[3].z, sc);
    s_split_store<FMT>(d + 3 * S_ROWB, x[0].w, x[1].w, x[2].w, x[3].w, sc);
  }
}

// ======================================================================================
// EDGE = false: whole tiles.  Addresses are (uniform tile base) + (loop-invariant 32-bit lane byte
// offset): the per-tile address arithmetic is scalar.
// ======================================================================================
template <int L>
__device__ __forceinline__ void f_lane_off(int64_t ld, int t, uint32_t (&o)[4]) {
  if constexpr (L == KC) {
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = static_cast<uint32_t>((((t >> 3) + 32 * p) * ld + (t & 7) * 4) * 4);
  } else {
    int nq, q;
    s_mc_map(t, nq, q);
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = static_cast<uint32_t>(((4 * q + p) * ld + 4 * nq) * 4);
  }
}
template <int L>
__device__ __forceinline__ const char* f_tile_base(const float* __restrict__ P, int64_t ld, int mn0, int k0) {
  return reinterpret_cast<const char*>(L == KC ? P + static_cast<int64_t>(mn0) * ld + k0
                                               : P + static_cast<int64_t>(k0) * ld + mn0);
}
__device__ __forceinline__ void f_load(const char* __restrict__ base, const uint32_t (&o)[4], float4 (&r)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) r[p] = *reinterpret_cast<const float4*>(base + o[p]);
}

// -DMI_GEMM_STAMPS: s_memtime stamps at the phase boundaries of every k-tile, from thread 0 of the
// first 64 workgroups of XCD 0 (tools/gemm_stamps.py reads them back).  Not part of the product build.
#ifdef MI_GEMM_STAMPS
__device__ long long g_stamps[64 * 64 * 8];
#define MI_STAMP(slot) do { if (stamp_on && kt < 64) g_stamps[(bid >> 3) * 512 + kt * 8 + slot] = clock64(); } while (0)
#else
#define MI_STAMP(slot) do {} while (0)
#endif

template <int FMT, int LA, int LB, bool COLSUM, bool GATHER, bool EDGE>
__global__ __launch_bounds__(kThreads, 2) void gemm_split_k(const GemmArgs a) {
  constexpr int NPL = SplitFmt<FMT>::NPL;
  __shared__ __attribute__((aligned(16))) char smem[2][NPL * S_PLANE];   // [operand][plane][row][80 B]

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
  const int klast = kbeg + (nk - 1) * BK;          // EDGE = false: loads past the last tile re-read it

  const int t = threadIdx.x;
  const int w = t >> 6, lane = t & 63;
  const int wm = w >> 1, wn = w & 1;
  const int i = lane & 31, h = lane >> 5;

  int sa = 0, sb = 0;                              // f16x2: power-of-two operand scales
  if constexpr (FMT == FMT_F16X2) { sa = pl_scale_exp(a.amax_a); sb = pl_scale_exp(a.amax_b); }
  const float sca = pl_pow2(sa), scb = pl_pow2(sb);

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const bool do_colsum = COLSUM && a.colsum_part != nullptr && tm == 0;
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[4], rb[4];

  // ---- operand fetch state ----
  int grow[4] = {0, 0, 0, 0};                      // EDGE gather: rows of the next A tile
  uint32_t oa[4] = {0, 0, 0, 0}, ob[4] = {0, 0, 0, 0}, oid[4] = {0, 0, 0, 0};
  int64_t gaddr[4] = {0, 0, 0, 0};                 // fast gather: byte address of the next tile's rows (sans column)
  int64_t g_lane_c = 0;                            // fast gather, MC: per-lane (field offset * E + column) bytes
  int gi_k = kbeg, gi_f = 0, gi_e = 0;             // fast gather, KC: tile whose ids are fetched next
  int gl_e = 0;                                    // ... and column inside the field of the tile loaded next
  const uint32_t Eb = GATHER ? static_cast<uint32_t>(a.g_ts) * 4u : 0u;       // bytes between consecutive table rows
  if constexpr (!EDGE) {
    if constexpr (!GATHER) f_lane_off<LA>(a.lda, t, oa);
    f_lane_off<LB>(a.ldb, t, ob);
    if constexpr (GATHER) {
      if constexpr (LA == KC) {
#pragma unroll
        for (int p = 0; p < 4; ++p) oid[p] = static_cast<uint32_t>(((t >> 3) + 32 * p) * a.g_F * 4);
        gi_f = kbeg / a.g_E; gi_e = kbeg % a.g_E; gl_e = gi_e;
      } else {
        int nq, q;
        s_mc_map(t, nq, q);
        const int mn = m0 + 4 * nq;
        const int f = mn / a.g_E;
#pragma unroll
        for (int p = 0; p < 4; ++p) oid[p] = static_cast<uint32_t>(((4 * q + p) * a.g_F + f) * 4);
        g_lane_c = (a.g_off[f] * a.g_ts + mn % a.g_E) * 4;
      }
    }
  }

  // fast gather: fetch the ids of the tile at gi_k and turn them into row byte addresses
  auto fetch_rows = [&]() {
    if constexpr (LA == KC) {
      const char* ib = reinterpret_cast<const char*>(a.g_ids + static_cast<int64_t>(m0) * a.g_F + gi_f);
      const int64_t ub = a.g_off[gi_f] * static_cast<int64_t>(Eb);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t id = *reinterpret_cast<const uint32_t*>(ib + oid[p]);
        gaddr[p] = static_cast<int64_t>(static_cast<uint64_t>(id) * Eb) + ub;
      }
      const bool adv = gi_k < klast;               // advance to the next tile (uniform, scalar)
      int e = gi_e + BK, f = gi_f;
      if (e >= a.g_E) { e -= a.g_E; ++f; }
      gi_k = adv ? gi_k + BK : gi_k; gi_e = adv ? e : gi_e; gi_f = adv ? f : gi_f;
    } else {
      const char* ib = reinterpret_cast<const char*>(a.g_ids + static_cast<int64_t>(gi_k) * a.g_F);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t id = *reinterpret_cast<const uint32_t*>(ib + oid[p]);
        gaddr[p] = static_cast<int64_t>(static_cast<uint64_t>(id) * Eb) + g_lane_c;
      }
      gi_k = gi_k < klast ? gi_k + BK : gi_k;
    }
  };

  auto load_tile = [&](int k0, bool first) {
    if constexpr (EDGE) {
      if constexpr (GATHER) {
        if (first) s_gather_rows<LA>(a, a.M, m0, k0, kend, grow, t);
        s_load_gathered<LA>(a, m0, k0, grow, ra, t);
        s_gather_rows<LA>(a, a.M, m0, k0 + BK, kend, grow, t);
      } else {
        s_load<LA>(a.A, a.lda, a.M, m0, k0, kend, ra, t);
      }
      s_load<LB>(a.B, a.ldb, a.N, n0, k0, kend, rb, t);
    } else {
      const int kc = min(k0, klast);
      if constexpr (GATHER) {
        if (first) fetch_rows();
        const char* tb = reinterpret_cast<const char*>(a.A);
        if constexpr (LA == KC) {
          const int64_t c = (gl_e + (t & 7) * 4) * 4;
#pragma unroll
          for (int p = 0; p < 4; ++p) ra[p] = *reinterpret_cast<const float4*>(tb + gaddr[p] + c);
          int e = gl_e + BK;
          if (e >= a.g_E) e -= a.g_E;
          gl_e = k0 < klast ? e : gl_e;
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p) ra[p] = *reinterpret_cast<const float4*>(tb + gaddr[p]);
        }
        fetch_rows();
      } else {
        f_load(f_tile_base<LA>(a.A, a.lda, m0, kc), oa, ra);
      }
      f_load(f_tile_base<LB>(a.B, a.ldb, n0, kc), ob, rb);
    }
  };
  auto stage = [&](int k0) {
    float4 unused = make_float4(0.f, 0.f, 0.f, 0.f);
    s_stage<FMT, LA, false, EDGE>(smem[0], a.M, m0, k0, kend, ra, t, sca, unused);
    s_stage<FMT, LB, COLSUM, EDGE>(smem[1], a.N, n0, k0, kend, rb, t, scb, cs);   // COLSUM: every block sums, tm == 0 writes
  };
  const char* Ar = smem[0] + (wm * 64 + i) * S_ROWB + h * 16;
  const char* Br = smem[1] + (wn * 64 + i) * S_ROWB + h * 16;
  bf16x8 fa[2][2][NPL], fb[2][2][NPL];          // [ks][mi|ni][plane]
  auto read_frags = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int p = 0; p < NPL; ++p)
          fa[ks][mi][p] = *reinterpret_cast<const bf16x8*>(Ar + p * S_PLANE + mi * 32 * S_ROWB + ks * 32);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int p = 0; p < NPL; ++p)
          fb[ks][ni][p] = *reinterpret_cast<const bf16x8*>(Br + p * S_PLANE + ni * 32 * S_ROWB + ks * 32);
    }
  };

  // Software pipeline: tile t's fragments live in registers while its MFMAs run; the split + LDS
  // stores of tile t+1 and the global loads of tile t+2 are issued in the gaps between the MFMAs
  // (32 matrix-pipe cycles each); then barrier, fragment reads of tile t+1, barrier.
  // Everything in the loop is branch-free on purpose (a branch fences hipcc's scheduler and its
  // waitcnt placement); the loads issued for the tile after the last one re-read the last one
  // (EDGE: the buffer's first element) and are never staged.
  if (nk > 0) {
    load_tile(kbeg, true);
    stage(kbeg);
    __syncthreads();
    read_frags();
    load_tile(kbeg + BK, false);
    __syncthreads();
  }
#ifdef MI_GEMM_STAMPS
  const bool stamp_on = (bid & 7) == 0 && (bid >> 3) < 64 && t == 0;
#endif
  auto mfma_tile = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          f32x16 c = acc[mi][ni];              // smallest partial products first
          if constexpr (FMT == FMT_F16X2) {
#define MI_MF(x, y) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, y), c, 0, 0, 0)
            MI_MF(fa[ks][mi][1], fb[ks][ni][0]);
            MI_MF(fa[ks][mi][0], fb[ks][ni][1]);
            MI_MF(fa[ks][mi][0], fb[ks][ni][0]);
#undef MI_MF
          } else {
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi][2], fb[ks][ni][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi][1], fb[ks][ni][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi][0], fb[ks][ni][2], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi][1], fb[ks][ni][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi][0], fb[ks][ni][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi][0], fb[ks][ni][0], c, 0, 0, 0);
          }
          acc[mi][ni] = c;
        }
  };
  for (int kt = 0; kt + 1 < nk; ++kt) {
    const int k1 = kbeg + (kt + 1) * BK;
    MI_STAMP(0);
    mfma_tile();
    stage(k1);
    load_tile(k1 + BK, false);
    if constexpr (FMT == FMT_F16X2) {
#pragma unroll
      for (int g = 0; g < 24; ++g) {           // 1 MFMA, then up to 6 VALU, 1 LDS store, 1 global load
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    } else {
#pragma unroll
      for (int g = 0; g < 24; ++g) {           // 2 MFMAs, then up to 8 VALU, 1 LDS store, 1 global load
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    MI_STAMP(1);
    __syncthreads();
    MI_STAMP(2);
    read_frags();
    MI_STAMP(3);
    __syncthreads();
    MI_STAMP(4);
  }
  if (nk > 0) mfma_tile();                     // last tile: nothing left to stage

  if (COLSUM && do_colsum) {     // threads sharing a column group differ in q (8 batch quads): fold in q order
    float* red = reinterpret_cast<float*>(&smem[0][0]);
    int nq, q;
    s_mc_map(t, nq, q);
    *reinterpret_cast<float4*>(red + q * BN + 4 * nq) = cs;
    __syncthreads();
    if (t < BN) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v += red[g * BN + t];
      if (n0 + t < a.N) a.colsum_part[static_cast<int64_t>(split) * a.N + n0 + t] = v;
    }
  }
  store_tile_c(a, acc, m0, n0, wm, wn, i, h, split, pl_pow2(-sa), pl_pow2(-sb));
}
