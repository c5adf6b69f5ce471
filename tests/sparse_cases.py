"""Inputs and references for the sparse gradient path — mi_entry_grads_segsum, mi_sparse_apply[_fused] (csrc/optim.hip) and
the gather side, mi_embed_fm_linear_fwd / _bwd, mi_gather_rows, mi_numeric_embed_fwd, mi_numeric_raw_fwd (csrc/embed.hip):
segments of prescribed lengths around every edge of the long-segment kernel's slicing, the per-entry gradient in fp64 and in
the kernels' own fp32 operation order, the two summation orders, the layouts the host ships, and forward tables that span
the exponent range.  No GPU code and no fixtures; the CPU half is test_sparse_cases_cpu.py, the GPU half
test_hip_sparse_sums.py.

What the kernels do (restated here once).  A lane group of LPR = lanes_per_row(E) lanes owns a row, a workgroup holds
G = 256 / LPR lane groups.  The gradient of entry e = (b, f) is, one rounding per operation (the files are built with
-ffp-contract=off):  t = sv - w;  p = gf * t;  v = dc;  v += p  — or, where d_concat already carries gf * sumv,
v -= gf * w — and a segment's sum starts at +0 and adds the v of its entries:
  sum_sequential   in ascending entry order: every segment of at most K_LONG = 48 entries;
  sum_sliced       longer segments: per = ceil(c / G) entries per slice, slice q = entries [q per, min(c, (q + 1) per)) summed
                   in order from +0 by lane group q, then the slice sums added in slice order starting from slice 0's
                   (slices past the end are +0).  A later change of the slicing changes that one function.
Both are vectorised over segments (the loop runs over the position inside a segment).  The wide part's scalar rides with the
rows: lane 0 of slice q's lane group sums d_logit_lin over the same slice.  A launch WITHOUT the rows (table == NULL,
out_rows == NULL) has one lane per request, so its long segments are cut into G = 256 slices whatever E is (l32_alone).

The error bar against fp64 is derived, not measured.  For a segment of c entries, per element,
  bar = (c + 3) * 2^-24 * sum_k a_k,      a_k = |dc_k| + |gf_k| * (|sv_k| + |w|).
Each term carries at most three roundings, each relative to a quantity that a_k bounds: t = sv - w is off by at most
2^-24 (|sv| + |w|), p = gf t adds 2^-24 |p| <= 2^-24 |gf| (|sv| + |w|), v = dc + p adds 2^-24 |v| <= 2^-24 a_k — at most
3 * 2^-24 a_k together (first order).  A sum of c terms in ANY order carries at most c - 1 further roundings, each relative
to a partial sum that sum_k |v_k| <= sum_k a_k bounds.  (c + 2) 2^-24 sum a_k to first order; the last unit covers the
second-order terms ((c + 2)^2 2^-48 is below 2^-24 for every c here).  The same bar with a_k = |d_logit_lin| holds the
wide part's sum, with c = 1 the per-entry gradients of mi_embed_fm_linear_bwd.

The wide forward set: values uniform in (-1, 1) times a per-row scale, log-uniform from 1e-20 to 1e18 (divided by
sqrt(E F / 4): the FM term sums E F squares in fp32, and 256 * 129 squares of 1e18 overflow), with -0.0 and
denormals planted in rows that are read.  The FM term squares values: to keep a whole example from underflowing (squares of
1e-20 are denormal, 1e-5 relative each, which no bar relative to the cancelling magnitude can hold) field 0's rows keep
their scale within [1e-3, 1e3] when there is more than one field; with one field the term is exactly 0 whatever the scale.
fwd_case asserts that twice the cancelling magnitude — a bound of every partial sum of the kernel — stays below 3e38."""
import numpy as np

from oracle import optimizers as OO

F32 = np.float32
U24 = 2.0 ** -24
K_LONG = 48                      # optim.hip's kLongSeg: longer segments go to the workgroup-per-row kernel
LONG_ROW = 2000                  # the one hot row of the prescribed case
SUM_E = [4, 12, 20, 64, 100, 256]                       # LPR 1, 4, 8, 16, 32, 64; 12, 20 and 100 leave lanes idle
FWD_E = [4, 12, 20, 32, 40, 64, 100, 128, 200, 256]
TOL = 1e-5                       # test_hip_kernels.py's bar for sumv and lin (max_err_scaled)
FM_BAR = 2e-6                    # ... and for fm against the magnitude that cancels
BIG = F32(3e38)                  # planted where no kernel may look
NAN = F32(np.nan)
TABLE_LAYOUTS = ["arrays", "rec3", "rowpad"]            # table_stride 0, 3 E, E + 4


def lanes_per_row(E):
    """the smallest power of two >= E / 4 (embed.hip's lanes_per_row)"""
    l = 1
    while l < E // 4:
        l <<= 1
    return l


def groups(E):
    """lane groups of a workgroup of 256 threads: the slices of a long segment, the examples of a forward block"""
    return 256 // lanes_per_row(E)


# ---- segments ----------------------------------------------------------------------------------------------------------------
def prescribed_counts(E):
    G = groups(E)
    return [1, 2, 47, 48, 49, 50, G - 1, G, G + 1, 2 * G + 3, LONG_ROW]


class Segments:
    """keys [n] int32 of n = B * F entries (entry e = b * F + f).  The first b0 examples are a chunk of their own: their keys
    lie in [0, R0), the others' in [R0, R) — sorted, the requests of the second chunk are u in [U0, U)."""

    def __init__(self, keys, B, F, b0, R0, R):
        self.keys, self.B, self.F, self.b0, self.R0, self.R = keys, B, F, b0, R0, R
        self.n = B * F
        assert keys.shape == (self.n,) and keys.dtype == np.int32
        self.order, self.uniq, self.seg = sort_segments(keys)
        self.U = len(self.uniq)
        self.counts = np.diff(self.seg)
        self.U0 = int(np.searchsorted(self.uniq, R0))
        self.seg_of_sorted = np.repeat(np.arange(self.U), self.counts)


def sort_segments(keys):
    """(sorted_entry, distinct keys ascending, seg_start [U + 1]) of the stable sort: what mi_sort_unique_rows gives"""
    order = np.argsort(keys, kind="stable").astype(np.int32)
    sk = keys[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    return order, sk[starts].astype(np.int32), np.r_[starts, len(keys)].astype(np.int32)


def prescribed_segments(E, seed=0):
    """The smallest input that holds every slice edge: distinct rows with 1, 2, 47, 48, 49, 50, G - 1, G, G + 1, 2 G + 3 and
    LONG_ROW entries, neighbours in key order, between two runs of singletons (more than 256 distinct rows: more than one
    workgroup of the lane-group kernel at every E), spread over the entry positions by a seeded permutation; before them a
    chunk of 8 examples with uniform keys."""
    F, B0, R0 = 5, 8, 24
    counts = prescribed_counts(E)
    n_single = 280
    n_single += (-(sum(counts) + n_single)) % F
    lens = np.array([1] * (n_single // 2) + counts + [1] * (n_single - n_single // 2))
    D = len(lens)
    rng = np.random.default_rng([E, seed, 3])
    R1 = D + D // 2                                       # a third of the key range is never asked for
    ids = np.sort(rng.choice(R1, D, replace=False))
    rows1 = np.repeat(ids, lens)
    rows1 = rows1[rng.permutation(len(rows1))]
    rows0 = rng.integers(0, R0, B0 * F)
    keys = np.concatenate([rows0, R0 + rows1]).astype(np.int32)
    assert len(rows1) % F == 0 and len(keys) < 8000
    s = Segments(keys, B0 + len(rows1) // F, F, B0, R0, R0 + R1)
    # the counts it claims
    assert s.U - s.U0 == D and np.array_equal(s.uniq[s.U0:], R0 + ids) and np.array_equal(s.counts[s.U0:], lens)
    assert s.U > 256 + s.U0 and s.U < s.R
    s.run0 = s.U0 + n_single // 2                         # u of the first prescribed row; the run is u in [run0, run0 + 11)
    assert np.array_equal(s.counts[s.run0:s.run0 + len(counts)], counts)
    for c in (49, 2 * groups(E) + 3, LONG_ROW):
        assert c in s.counts
    return s


def uniform_segments(B, F, R, seed=0, b0=0):
    """plain uniform keys with segments of 1 to about 6 entries (n = B F about 3 R): the layout cases"""
    rng = np.random.default_rng([B, F, R, seed, 5])
    keys = rng.integers(0, R - 1, B * F).astype(np.int32)             # (the last row is never asked for)
    if b0:
        keys[:b0 * F] = rng.integers(0, R // 4, b0 * F)
        keys[b0 * F:] = R // 4 + rng.integers(0, R - 1 - R // 4, (B - b0) * F)
    return Segments(keys, B, F, b0, R // 4 if b0 else 0, R)


# ---- per-entry gradients -------------------------------------------------------------------------------------------------------
def grad_inputs(seg, E, seed=0, ld_pad=0):
    """the backward's leavings for seg's batch: dc [B, F E + ld_pad] (pad NaN), sv [B, E], gf [B], gl [B], and w [R, E] (the
    rows, by key), lw [R]"""
    rng = np.random.default_rng([seg.n, E, seed, 7])
    dc = np.full((seg.B, seg.F * E + ld_pad), NAN, F32)
    dc[:, :seg.F * E] = rng.standard_normal((seg.B, seg.F * E))
    return dict(dc=dc, sv=rng.standard_normal((seg.B, E)).astype(F32) * F32(2), gf=rng.standard_normal(seg.B).astype(F32),
                gl=rng.standard_normal(seg.B).astype(F32), w=rng.standard_normal((seg.R, E)).astype(F32),
                lw=rng.standard_normal(seg.R).astype(F32))


def entry_parts(entries, F, E, b0, dc, sv, gf):
    """(dc, sv, gf) of the global entries `entries` from per-example arrays that begin at example b0; a part that is None
    stays None"""
    b, f = entries // F - b0, entries % F
    dce = None if dc is None else dc[:, :F * E].reshape(len(dc), F, E)[b, f]
    return dce, None if sv is None else sv[b], None if gf is None else gf[b]


def values64(dce, sve, gfe, we):
    """d_concat + d_logit_fm * (sumv - w) per entry in fp64, each part optional; sve None with gfe given: the form where
    d_concat carries d_logit_fm * sumv"""
    v = np.zeros(we.shape, np.float64) if dce is None else dce.astype(np.float64)
    if gfe is not None:
        s = 0.0 if sve is None else sve.astype(np.float64)
        v = v + gfe.astype(np.float64)[:, None] * (s - we.astype(np.float64))
    return v


def values32(dce, sve, gfe, we):
    """the same in fp32 in the kernel's operation order, one rounding per operation"""
    v = np.zeros(we.shape, F32) if dce is None else dce.copy()
    if gfe is not None:
        if sve is not None:
            t = sve - we
            p = gfe[:, None] * t
            v = v + p
        else:
            v = v - gfe[:, None] * we
    assert v.dtype == F32
    return v


def magnitudes(dce, sve, gfe, we):
    """a_k of the error bar, fp64"""
    a = np.zeros(we.shape, np.float64) if dce is None else np.abs(dce.astype(np.float64))
    if gfe is not None:
        s = 0.0 if sve is None else np.abs(sve.astype(np.float64))
        a = a + np.abs(gfe.astype(np.float64))[:, None] * (s + np.abs(we.astype(np.float64)))
    return a


# ---- sums ------------------------------------------------------------------------------------------------------------------
def sum_sequential(vals, starts, ends):
    """out[u] = ((0 + vals[starts[u]]) + vals[starts[u] + 1]) + ... in vals' dtype: the order of every short segment"""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    out = np.zeros((len(starts),) + vals.shape[1:], vals.dtype)
    for k in range(int((ends - starts).max()) if len(starts) else 0):
        sel = starts + k < ends
        out[sel] = out[sel] + vals[(starts + k)[sel]]
    return out


def sum_sliced(vals, starts, ends, E):
    """sparse_apply_long_k's order: G slices of per = ceil(c / G) entries, each summed in order, the slice sums added in
    slice order"""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    G = groups(E)
    per = -(-(ends - starts) // G)
    q = np.arange(G)[None, :]
    k0 = np.minimum(ends[:, None], starts[:, None] + q * per[:, None])
    k1 = np.minimum(ends[:, None], k0 + per[:, None])
    part = sum_sequential(vals, k0.ravel(), k1.ravel()).reshape((len(starts), G) + vals.shape[1:])
    out = part[:, 0].copy()
    for j in range(1, G):
        out = out + part[:, j]
    return out


def segment_sums32(vals, seg, E):
    """vals [n, ...] fp32 in sorted-entry order -> [U, ...]: sequential up to K_LONG entries, sliced above"""
    starts, ends = seg[:-1].astype(np.int64), seg[1:].astype(np.int64)
    out = sum_sequential(vals, starts, np.minimum(ends, starts + K_LONG))       # (long ones: overwritten below)
    long = np.flatnonzero(ends - starts > K_LONG)
    if len(long):
        out[long] = sum_sliced(vals, starts[long], ends[long], E)
    assert out.dtype == F32
    return out


def segment_sums64(vals, seg_of_sorted, U):
    out = np.zeros((U,) + vals.shape[1:], np.float64)
    np.add.at(out, seg_of_sorted, vals.astype(np.float64))
    return out


def error_bar(mags, seg_of_sorted, U, counts):
    """(c + 3) 2^-24 sum_k a_k per segment and element (module docstring)"""
    c = np.asarray(counts, np.float64).reshape((U,) + (1,) * (mags.ndim - 1))
    return (c + 3) * U24 * segment_sums64(mags, seg_of_sorted, U)


class RowGrads:
    """Everything the tests need of one (segments, inputs, form): per distinct request u the summed row gradient in the
    kernel's fp32 order (g32), in fp64 (g64) and its bar, the same for the wide part (l32 — l32_alone where the launch
    has no rows — l64, lbar), and the per-entry
    values in entry order (v32: what mi_embed_fm_linear_bwd writes, d_rows of the unfused apply).
    form: fm (FM term on), dc (d_concat on), sumv (False: d_concat carries gf * sumv, added here in fp32 as the host does).
    w_of_u [U, E]: the row of request u.  lo, hi: the requests summed (a chunk: per-example arrays from example b0)."""

    def __init__(self, seg, inp, E, w_of_u, fm=True, dc=True, sumv=True, lo=0, hi=None, b0=0):
        hi = seg.U if hi is None else hi
        F = seg.F
        k0, k1 = int(seg.seg[lo]), int(seg.seg[hi])
        ent = seg.order[k0:k1].astype(np.int64)
        sos = seg.seg_of_sorted[k0:k1] - lo
        sg = (seg.seg[lo:hi + 1] - k0).astype(np.int64)
        U = hi - lo
        d = inp["dc"][b0:] if dc else None
        self.dc_in = None if d is None else d.copy()
        if fm and not sumv:                                 # the planes path: the data gradient's epilogue added gf * sumv
            assert dc
            B = len(d)
            d = d.copy()
            d[:, :F * E] = (d[:, :F * E].reshape(B, F, E) + (inp["gf"][b0:, None] * inp["sv"][b0:])[:, None, :]).reshape(B, F * E)
            self.dc_in = d
        dce, sve, gfe = entry_parts(ent, F, E, b0, d, inp["sv"][b0:] if fm and sumv else None, inp["gf"][b0:] if fm else None)
        we = w_of_u[lo:hi][sos]
        v32 = values32(dce, sve, gfe, we)
        self.g32 = segment_sums32(v32, sg, E)
        self.g64 = segment_sums64(values64(dce, sve, gfe, we), sos, U)
        self.bar = error_bar(magnitudes(dce, sve, gfe, we), sos, U, np.diff(sg))
        gle = inp["gl"][b0:][ent // F - b0]
        self.l32 = segment_sums32(gle, sg, E)
        self.l32_alone = segment_sums32(gle, sg, 4)        # a launch without the rows: one lane per request, G = 256
        self.l64 = segment_sums64(gle, sos, U)
        self.lbar = error_bar(np.abs(gle.astype(np.float64)), sos, U, np.diff(sg))
        self.v32 = v32[np.argsort(ent, kind="stable")]      # (ascending entry order: row i belongs to entry sort(ent)[i])
        self.entries, self.seg, self.seg_of_sorted, self.U = ent, sg, sos, U
        self.gl_entry = inp["gl"][b0:][np.sort(ent) // F - b0]


def worst(got, ref64, bar):
    """max |got - ref| / bar over the elements (0 where both vanish); NaN counts as a miss"""
    err = np.abs(got.astype(np.float64) - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


# ---- the optimizer on the summed gradient ------------------------------------------------------------------------------------------
STEP = 10


def hyper(name):
    return OO.Hyper(name, lr=0.001 if name == "Adam" else 0.05)


def lr_t_of(hp, step):
    """TF's fp32 schedule lr sqrt(1 - beta2^t) / (1 - beta1^t): an input of the entries"""
    p = OO.AdamPowers(hp, F32)
    for _ in range(step - 1):
        p.finish()
    return float(p.lr_t(hp.lr))


def row_state(name, seg, E, step=STEP, seed=0):
    """Slots and stamps of all R rows ([R, E] and [R] for the wide part).  Adam: touched rows with long and with short
    segments have sat out 0, 1 and 5 steps or were never applied (stamp 0, m = v = 0), in turn; the others hold anything."""
    rng = np.random.default_rng([seg.R, E, seed, 9])
    R = seg.R
    if name == "Adam":
        s0 = (rng.standard_normal((R, E)) * 0.1).astype(F32); s1 = rng.uniform(1e-4, 1e-2, (R, E)).astype(F32)
        l0 = (rng.standard_normal(R) * 0.1).astype(F32); l1 = rng.uniform(1e-4, 1e-2, R).astype(F32)
    elif name == "Adagrad":
        s0 = (0.1 + rng.random((R, E))).astype(F32); s1 = None
        l0 = (0.1 + rng.random(R)).astype(F32); l1 = None
    else:
        s0 = s1 = l0 = l1 = None
    stamp = rng.integers(0, step, R).astype(np.int32)
    classes = np.array([step - 1, step - 2, step - 6, 0], np.int32)
    for sel in (seg.counts > K_LONG, seg.counts <= K_LONG):
        rows = seg.uniq[sel]
        stamp[rows] = classes[np.arange(len(rows)) % 4]
    if name == "Adam":
        never = stamp == 0
        s0[never] = 0; s1[never] = 0; l0[never] = 0; l1[never] = 0
    return dict(s0=s0, s1=s1, l0=l0, l1=l1, stamp=stamp)


def apply_rows(hp, w, s0, s1, stamp, g, step, lr_t):
    """The header's sparse rule on the touched rows alone (w, s0, s1, g: [U, width]; stamp [U] or None), through
    oracle.optimizers.sparse_apply with one entry per row; Adam's deferred decay first, as the multiply chain the header
    describes.  Returns new (w, s0, s1)."""
    w = w.copy(); s0 = None if s0 is None else s0.copy(); s1 = None if s1 is None else s1.copy()
    if hp.name == OO.ADAM and stamp is not None:
        missed = np.where(stamp > 0, np.maximum(0, step - 1 - stamp), 0)
        b1, b2 = F32(hp.beta1), F32(hp.beta2)
        for j in range(int(missed.max()) if len(missed) else 0):
            on = (missed > j)[:, None]
            s0 = np.where(on, s0 * b1, s0); s1 = np.where(on, s1 * b2, s1)
    z = np.zeros_like(w)
    OO.sparse_apply(hp, w, z if s0 is None else s0, z.copy() if s1 is None else s1, np.arange(len(w)), g, lr_t)
    assert w.dtype == F32
    return w, s0, s1


# ---- layouts -----------------------------------------------------------------------------------------------------------------
class Packed:
    """flat: the fp32 buffer; off: element offsets of the parts inside it; stride: the entry's stride argument"""

    def __init__(self, flat, off, stride):
        self.flat, self.off, self.stride = flat, off, stride


def pack_table(layout, w, s0=None, s1=None, fill=NAN):
    """table / t_slot0 / t_slot1 as three [R, E] arrays (stride 0), one [w | slot0 | slot1] record of 3 E floats per row,
    or three arrays with rows E + 4 apart.  A slot that is None and every pad hold `fill`."""
    R, E = w.shape
    parts = [w, s0, s1]
    if layout == "arrays":
        flat = np.full((3, R, E), fill, F32)
        for i, p in enumerate(parts):
            if p is not None:
                flat[i] = p
        return Packed(flat.reshape(-1), (0, R * E, 2 * R * E), 0)
    if layout == "rec3":
        flat = np.full((R, 3, E), fill, F32)
        for i, p in enumerate(parts):
            if p is not None:
                flat[:, i] = p
        return Packed(flat.reshape(-1), (0, E, 2 * E), 3 * E)
    assert layout == "rowpad", layout
    flat = np.full((3, R, E + 4), fill, F32)
    for i, p in enumerate(parts):
        if p is not None:
            flat[i, :, :E] = p
    return Packed(flat.reshape(-1), (0, R * (E + 4), 2 * R * (E + 4)), E + 4)


def unpack_table(layout, flat, R, E):
    """(w, s0, s1, pads) of a packed table; pads: a flat array of everything else (empty where the layout has none)"""
    if layout == "arrays":
        a = flat.reshape(3, R, E)
        return a[0], a[1], a[2], np.zeros(0, F32)
    if layout == "rec3":
        a = flat.reshape(R, 3, E)
        return a[:, 0], a[:, 1], a[:, 2], np.zeros(0, F32)
    a = flat.reshape(3, R, E + 4)
    return a[0, :, :E], a[1, :, :E], a[2, :, :E], a[:, :, E:].reshape(-1)


def pack_wide(ls, w, s0=None, s1=None, stamp=None, fill=NAN):
    """lin_w / l_slot0 / l_slot1 / last_step as four arrays (lin_stride 1) or {w, slot0, slot1, stamp} records (4)"""
    R = len(w)
    a = np.full((4, R) if ls == 1 else (R, 4), fill, F32)
    for i, p in enumerate([w, s0, s1, None if stamp is None else stamp.astype(np.int32).view(F32)]):
        if p is not None:
            if ls == 1:
                a[i] = p
            else:
                a[:, i] = p
    return Packed(a.reshape(-1), (0, R, 2 * R, 3 * R) if ls == 1 else (0, 1, 2, 3), ls)


def unpack_wide(ls, flat, R):
    a = flat.reshape(4, R) if ls == 1 else flat.reshape(R, 4).T
    return a[0], a[1], a[2], a[3].copy().view(np.int32)


def pack_records(S, rows, lin, fill=NAN):
    """rows [n, E] and lin [n] as two arrays (S = 0) or one record [row | value | pad] of S floats per request — gradients
    (grad_stride), the exchange's rows (rows_stride) and the sums (out_stride); either part may be None (left as fill)"""
    n, E = rows.shape
    if S == 0:
        flat = np.full(n * E + n, fill, F32)
        flat[:n * E] = rows.reshape(-1)
        if lin is not None:
            flat[n * E:] = lin
        return Packed(flat, (0, n * E), 0)
    assert S >= E + 4 and S % 4 == 0
    a = np.full((n, S), fill, F32)
    a[:, :E] = rows
    if lin is not None:
        a[:, E] = lin
    return Packed(a.reshape(-1), (0, E), S)


def unpack_records(S, flat, n, E):
    """(rows, lin, pads)"""
    if S == 0:
        return flat[:n * E].reshape(n, E), flat[n * E:], np.zeros(0, F32)
    a = flat.reshape(n, S)
    return a[:, :E], a[:, E], a[:, E + 1:].reshape(-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- forward inputs ------------------------------------------------------------------------------------------------------------
FWD_SETS = ["normal", "wide"]
PLANTED = np.array([-0.0, 1e-40, -3e-42, 1.4e-45], F32)   # -0.0 and three denormals


def fwd_shapes(E):
    """(F list, B list) of the forward grid: F around the rounds of rows in flight (8) and of the id shuffle (LPR), B around
    a workgroup's G examples"""
    L, G = lanes_per_row(E), groups(E)
    Fs = sorted({f for f in (1, 7, 8, 9, L - 1, L, L + 1, 2 * L + 1) if f >= 1})
    Bs = sorted({b for b in (1, G - 1, G, G + 1, 3 * G + 1) if b >= 1})
    return Fs, Bs


def fwd_case(E, F, B, which, seed=0):
    """table [R, E], lin_w [R], field_off [F] int64, ids [B, F] int32 and the rows read [B, F].  The last row is read by no
    id and holds BIG; example 0's rows carry PLANTED in the wide set."""
    rng = np.random.default_rng([E, F, B, seed, FWD_SETS.index(which), 13])
    vocab = rng.integers(3, 12, F)
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    R = int(off[-1]) + 1
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    rows = off[:-1][None, :] + ids
    if which == "normal":
        table = rng.standard_normal((R, E)).astype(F32)
    else:
        scale = 10.0 ** rng.uniform(-20, 18, R)
        if F > 1:
            scale[:vocab[0]] = 10.0 ** rng.uniform(-3, 3, vocab[0])
        scale /= max(np.sqrt(E * F / 4.0), 1.0)           # an example's sum of E F squares stays in range
        table = (rng.uniform(-1, 1, (R, E)) * scale[:, None]).astype(F32)
        for f in range(F):
            table[rows[0, f], (f + np.arange(4)) % E if E > 4 else np.arange(4)] = np.roll(PLANTED, f)
    table[R - 1] = BIG
    lin_w = rng.standard_normal(R).astype(F32)
    lin_w[R - 1] = BIG
    assert rows.max() < R - 1
    v = table[rows].astype(np.float64)
    mag = 0.5 * ((v.sum(1) ** 2).sum(1) + (v ** 2).sum((1, 2)))
    assert 2 * mag.max() < 3e38, (E, F, B, which, mag.max())
    return dict(table=table, lin_w=lin_w, off=off[:-1].copy(), ids=ids, rows=rows, R=R, mag=mag + 1e-30)


def fwd_reference(c):
    """fp64 sumv, fm, lin and the exact amax of the rows read"""
    v = c["table"][c["rows"]].astype(np.float64)
    s = v.sum(1)
    fm = 0.5 * ((s * s).sum(1) - (v * v).sum((1, 2)))
    return dict(concat=c["table"][c["rows"]], sumv=s, fm=fm, lin=c["lin_w"][c["rows"]].astype(np.float64).sum(1),
                amax=F32(np.abs(c["table"][c["rows"]]).max()))


def max_err_scaled(a, b):
    """tests.util's: max |a - b| / max(|b|, rms(b))"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    floor = np.sqrt(np.mean(b * b)) + 1e-30
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


# ---- the small entries ---------------------------------------------------------------------------------------------------------
def numeric_inputs(B, nd, E, seed=0):
    rng = np.random.default_rng([B, nd, E, seed, 17])
    return dict(x=rng.standard_normal((B, nd)).astype(F32), V=rng.standard_normal((nd, E)).astype(F32),
                w_num=rng.standard_normal(nd).astype(F32))


def numeric_embed_reference(x, V, w_num, sumv0, fm0, lin0):
    """mi_numeric_embed_fwd on top of what a categorical forward left (sumv0 [B, E], fm0 [B], lin0 [B], fp32): the concat
    columns x[b, j] * V[j, e] as fp32 products (one rounding: exact), and in fp64 the new sumv, fm, lin with the magnitude
    that cancels in fm's increment"""
    r32 = x[:, :, None] * V[None, :, :]
    assert r32.dtype == F32
    r = x.astype(np.float64)[:, :, None] * V.astype(np.float64)[None, :, :]
    sc = sumv0.astype(np.float64)
    st = sc + r.sum(1)
    inc = 0.5 * ((st * st - sc * sc) - (r * r).sum(1)).sum(1)
    mag = 0.5 * ((st * st + sc * sc) + (r * r).sum(1)).sum(1) + np.abs(fm0.astype(np.float64)) + 1e-30
    return dict(concat=r32.reshape(len(x), -1), sumv=st, fm=fm0.astype(np.float64) + inc, mag=mag,
                lin=lin0.astype(np.float64) + x.astype(np.float64) @ w_num.astype(np.float64))


def numeric_raw_reference(x, w_num, lin0, n_cols):
    """mi_numeric_raw_fwd: the values, zero pad up to n_cols; lin0 + x[:, 0] w[0] + ... in fp32, ascending j, products
    rounded on their own"""
    B, nd = x.shape
    cols = np.zeros((B, n_cols), F32)
    cols[:, :nd] = x
    acc = lin0.copy()
    for j in range(nd):
        acc = acc + x[:, j] * w_num[j]
    assert acc.dtype == F32
    return cols, acc


def nan_patterns(n, seed=0):
    """n fp32 bit patterns as uint32: random bits with quiet and signalling NaN payloads, infinities and -0.0 planted"""
    rng = np.random.default_rng([n, seed, 19])
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8FFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32)
    pos = np.arange(0, n, max(n // len(special), 1))[:len(special)]
    bits[pos] = special[:len(pos)]
    return bits
