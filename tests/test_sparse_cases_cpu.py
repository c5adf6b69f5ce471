"""The references of tests/sparse_cases.py checked on the host: the fp32 restatement of the kernels' sums stays within the
derived bar of the fp64 reference, the bar is not vacuous (three planted faults exceed it at every E), the two summation
orders agree where they must, the layout packers round-trip, and the numpy stand-ins of tests/cpu_kernels.py — written from
the header on their own, summing every segment sequentially — agree with both.  Figures are printed (pytest -s): SPARSE ..."""
import numpy as np
import pytest
import torch

from tests import sparse_cases as S
from tests.cpu_kernels import NumpyKernels

F32 = np.float32
FORMS = [dict(fm=True, dc=True, sumv=True), dict(fm=True, dc=False, sumv=True), dict(fm=False, dc=True, sumv=True),
         dict(fm=True, dc=True, sumv=False)]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def cases():
    out = {}
    for E in S.SUM_E:
        seg = S.prescribed_segments(E)
        out[E] = (seg, S.grad_inputs(seg, E))
    return out


@pytest.mark.parametrize("E", S.SUM_E)
def test_restatement_stays_within_the_bar_of_fp64(cases, E):
    seg, inp = cases[E]
    w = inp["w"][seg.uniq]
    worst = 0.0
    for form in FORMS:
        for lo, hi, b0 in ((0, seg.U, 0), (seg.U0, seg.U, seg.b0), (seg.run0 + 7, seg.run0 + 40, 0)):
            g = S.RowGrads(seg, inp, E, w, lo=lo, hi=hi, b0=b0, **form)
            a, b = S.worst(g.g32, g.g64, g.bar), S.worst(g.l32, g.l64, g.lbar)
            assert a <= 1.0 and b <= 1.0, (E, form, lo, a, b)
            worst = max(worst, a, b)
    print("SPARSE host restatement E=%-3d worst |g32 - g64| / bar %.3f" % (E, worst))
    # a chunk's sums are the whole batch's sums of the same requests, bit for bit: b0 only moves the arrays
    full, part = S.RowGrads(seg, inp, E, w), S.RowGrads(seg, inp, E, w, lo=seg.U0, b0=seg.b0)
    assert S.same_bits(full.g32[seg.U0:], part.g32) and S.same_bits(full.l32[seg.U0:], part.l32)


@pytest.mark.parametrize("E", S.SUM_E)
def test_planted_faults_exceed_the_bar(cases, E):
    seg, inp = cases[E]
    F = seg.F
    w = inp["w"][seg.uniq]
    ref = S.RowGrads(seg, inp, E, w, lo=seg.U0, b0=seg.b0)
    ent, sos, sg = ref.entries, ref.seg_of_sorted, ref.seg
    we = w[seg.U0:][sos]
    dc, sv, gf = inp["dc"][seg.b0:], inp["sv"][seg.b0:], inp["gf"][seg.b0:]
    dce, sve, gfe = S.entry_parts(ent, F, E, seg.b0, dc, sv, gf)
    u49 = int(np.flatnonzero(np.diff(sg) == 49)[0])
    # one entry dropped from the 49-entry segment
    v = S.values32(dce, sve, gfe, we)
    v[sg[u49] + 17] = 0
    g = S.segment_sums32(v, sg, E)
    a = S.worst(g[u49], ref.g64[u49], ref.bar[u49])
    # the FM term's sign flipped
    g = S.segment_sums32(S.values32(dce, sve, -gfe, we), sg, E)
    b = np.array([S.worst(g[u], ref.g64[u], ref.bar[u]) for u in range(ref.U)])
    # b0 ignored: the per-example arrays read at b instead of b - b0 (wrapped at the arrays' end)
    bad = (ent // F % len(dc)) * F + ent % F
    dcx, svx, gfx = S.entry_parts(bad, F, E, 0, dc, sv, gf)
    g = S.segment_sums32(S.values32(dcx, svx, gfx, we), sg, E)
    c = np.array([S.worst(g[u], ref.g64[u], ref.bar[u]) for u in range(ref.U)])
    glx = S.segment_sums32(inp["gl"][seg.b0:][ent // F % len(dc)], sg, E)
    d = S.worst(glx[u49], ref.l64[u49], ref.lbar[u49])
    print("SPARSE planted faults E=%-3d dropped entry %.3g, FM sign: min over rows %.3g, b0 ignored: min over rows %.3g, wide part %.3g "
          "(each in bars)" % (E, a, b.min(), c.min(), d))
    assert a > 1 and b.min() > 1 and c.min() > 1 and d > 1


@pytest.mark.parametrize("E", S.SUM_E)
def test_sliced_equals_sequential_while_a_slice_holds_one_entry(E):
    G = S.groups(E)
    rng = np.random.default_rng(E)
    lens = np.arange(1, G + 1)
    seg = np.r_[0, np.cumsum(lens)]
    vals = rng.standard_normal((seg[-1], 8)).astype(F32)
    assert S.same_bits(S.sum_sliced(vals, seg[:-1], seg[1:], E), S.sum_sequential(vals, seg[:-1], seg[1:]))
    # ... and differs in association beyond: c = 3 G in slices of 3
    v = rng.standard_normal((3 * G, 64)).astype(F32)
    a, b = S.sum_sliced(v, [0], [3 * G], E), S.sum_sequential(v, [0], [3 * G])
    assert not S.same_bits(a, b) and np.allclose(a, b, atol=1e-4)
    # slices: per = ceil(c / G); the last ones are empty when c < G per
    c = 2 * G + 3
    v = rng.standard_normal((c, 4)).astype(F32)
    by_hand = np.zeros(4, F32)
    for q in range(G):
        part = np.zeros(4, F32)
        for k in range(min(c, 3 * q), min(c, 3 * q + 3)):
            part = part + v[k]
        by_hand = part if q == 0 else by_hand + part
    assert S.same_bits(S.sum_sliced(v, [0], [c], E)[0], by_hand)


@pytest.mark.parametrize("E", [4, 20])
def test_packers_round_trip(E):
    rng = np.random.default_rng(E)
    R, n = 9, 13
    w, s0, s1 = [rng.standard_normal((R, E)).astype(F32) for _ in range(3)]
    for layout in S.TABLE_LAYOUTS:
        p = S.pack_table(layout, w, s0, s1)
        a, b, c, pads = S.unpack_table(layout, p.flat, R, E)
        assert S.same_bits(a, w) and S.same_bits(b, s0) and S.same_bits(c, s1) and np.isnan(pads).all()
        assert (len(pads) > 0) == (layout == "rowpad") and p.stride == {"arrays": 0, "rec3": 3 * E, "rowpad": E + 4}[layout]
        for i, part in enumerate((w, s0, s1)):               # the offsets and the stride address the parts
            st = p.stride or E
            assert all(S.same_bits(p.flat[p.off[i] + r * st:p.off[i] + r * st + E], part[r]) for r in range(R))
        q = S.pack_table(layout, w, None, None, fill=S.BIG)
        a, b, c, pads = S.unpack_table(layout, q.flat, R, E)
        assert S.same_bits(a, w) and (b == S.BIG).all() and (c == S.BIG).all() and (pads == S.BIG).all()
    lw, l0, l1 = [rng.standard_normal(R).astype(F32) for _ in range(3)]
    stamp = rng.integers(0, 100, R).astype(np.int32)
    for ls in (1, 4):
        p = S.pack_wide(ls, lw, l0, l1, stamp)
        a, b, c, d = S.unpack_wide(ls, p.flat, R)
        assert S.same_bits(a, lw) and S.same_bits(b, l0) and S.same_bits(c, l1) and np.array_equal(d, stamp)
        assert all(p.flat[p.off[0] + r * ls] == lw[r] and p.flat[p.off[3] + r * ls].view(np.int32) == stamp[r] for r in range(R))
    rows, lin = rng.standard_normal((n, E)).astype(F32), rng.standard_normal(n).astype(F32)
    for Srec in (0, E + 4, E + 8):
        p = S.pack_records(Srec, rows, lin)
        a, b, pads = S.unpack_records(Srec, p.flat, n, E)
        assert S.same_bits(a, rows) and S.same_bits(b, lin) and np.isnan(pads).all() and len(pads) == (n * (Srec - E - 1) if Srec else 0)


# ---- the stand-ins of tests/cpu_kernels.py ---------------------------------------------------------------------------------------
def _sorted(seg):
    return _t(seg.seg), _t(seg.order), _t(seg.uniq), _t(np.array([seg.U], np.int32))


def test_stand_in_segsum_against_the_references(cases):
    E = 12
    seg, inp = cases[E]
    k = NumpyKernels()
    sg, se, _, _ = _sorted(seg)
    w = inp["w"][seg.uniq]
    for form, lo, b0 in ((FORMS[0], 0, 0), (FORMS[0], seg.U0, seg.b0), (FORMS[1], 0, 0), (FORMS[2], 0, 0)):
        g = S.RowGrads(seg, inp, E, w, lo=lo, b0=b0, **form)
        out_r, out_l = torch.full((g.U, E), float("nan")), torch.full((g.U,), float("nan"))
        k.mi_entry_grads_segsum(_t(w), sg, se, lo, g.U, _t(inp["dc"][b0:]) if form["dc"] else None, seg.F * E, _t(inp["sv"][b0:]),
                                _t(inp["gf"][b0:]) if form["fm"] else None, _t(inp["gl"][b0:]), b0, seg.F, E, out_r, out_l, lo)
        short = np.diff(g.seg) <= S.K_LONG
        assert S.same_bits(out_r.numpy()[short], g.g32[short]) and S.same_bits(out_l.numpy()[short], g.l32[short])
        assert S.worst(out_r.numpy(), g.g64, g.bar) <= 1 and S.worst(out_l.numpy(), g.l64, g.lbar) <= 1


@pytest.mark.parametrize("name", ["SGD", "Adagrad", "Adam"])
@pytest.mark.parametrize("fused", [False, True])
def test_stand_in_sparse_apply_against_the_references(cases, name, fused):
    from mi355x_rec.engine import OptimizerSpec
    E = 12
    seg, inp = cases[E]
    hp = S.hyper(name)
    lr_t = S.lr_t_of(hp, S.STEP) if name == "Adam" else 0.0
    h = OptimizerSpec(name, hp.lr).hparams(lr_t)
    st = S.row_state(name, seg, E)
    rows = seg.uniq
    g = S.RowGrads(seg, inp, E, inp["w"][rows])
    T, L = inp["w"].copy(), inp["lw"].copy()
    t0, t1, l0, l1 = [None if st[x] is None else st[x].copy() for x in ("s0", "s1", "l0", "l1")]
    stamp = st["stamp"].copy() if name == "Adam" else None
    k = NumpyKernels()
    sg, se, uq, nu = _sorted(seg)
    if fused:
        k.mi_sparse_apply_fused(_t(T), _t(t0), _t(t1), _t(L), _t(l0), _t(l1), _t(stamp), uq, sg, se, nu, seg.n, _t(inp["dc"]),
                                seg.F * E, _t(inp["sv"]), _t(inp["gf"]), _t(inp["gl"]), seg.F, E, S.STEP, h)
    else:
        k.mi_sparse_apply(_t(T), _t(t0), _t(t1), _t(L), _t(l0), _t(l1), _t(stamp), uq, sg, se, nu, seg.n, _t(g.v32),
                          _t(g.gl_entry), E, S.STEP, h)
    short = seg.counts <= S.K_LONG
    sub = lambda a, sel: None if a is None else a[rows[sel]]
    for sel, gr, gl in ((short, g.g32, g.l32), (~short, None, None)):
        if gr is None:          # long segments: the stand-in sums them sequentially — its own fp32 sums, held to the bar
            seq = S.sum_sequential(g.v32[seg.order], seg.seg[:-1], seg.seg[1:])
            assert S.worst(seq, g.g64, g.bar) <= 1
            gr, gl = seq, S.sum_sequential(g.gl_entry[seg.order], seg.seg[:-1], seg.seg[1:])
        ew, e0, e1 = S.apply_rows(hp, inp["w"][rows[sel]], sub(st["s0"], sel), sub(st["s1"], sel),
                                  None if stamp is None else st["stamp"][rows[sel]], gr[sel], S.STEP, lr_t)
        assert S.same_bits(T[rows[sel]], ew), (name, fused)
        assert e0 is None or t0 is None or S.same_bits(t0[rows[sel]], e0)
        assert e1 is None or t1 is None or S.same_bits(t1[rows[sel]], e1)
        lw, f0, f1 = S.apply_rows(hp, inp["lw"][rows[sel], None], None if st["l0"] is None else st["l0"][rows[sel], None],
                                  None if st["l1"] is None else st["l1"][rows[sel], None],
                                  None if stamp is None else st["stamp"][rows[sel]], gl[sel, None], S.STEP, lr_t)
        assert S.same_bits(L[rows[sel]], lw[:, 0])
        assert f0 is None or l0 is None or S.same_bits(l0[rows[sel]], f0[:, 0])
    untouched = np.setdiff1d(np.arange(seg.R), rows)
    assert len(untouched) > 50 and S.same_bits(T[untouched], inp["w"][untouched])
    if stamp is not None:
        assert (stamp[rows] == S.STEP).all() and np.array_equal(stamp[untouched], st["stamp"][untouched])


@pytest.mark.parametrize("which", S.FWD_SETS)
@pytest.mark.parametrize("E,F,B", [(4, 3, 7), (20, 9, 5), (64, 17, 3)])
def test_stand_in_forward_and_backward_against_the_references(E, F, B, which):
    c = S.fwd_case(E, F, B, which)
    ref = S.fwd_reference(c)
    k = NumpyKernels()
    concat, sumv, fm, lin = torch.empty(B, F * E), torch.empty(B, E), torch.empty(B), torch.empty(B)
    amax = torch.zeros(64)
    with np.errstate(all="ignore"):
        k.mi_embed_fm_linear_fwd(_t(c["table"]), _t(c["lin_w"]), _t(c["off"]), _t(c["ids"]), B, F, E, concat, F * E, sumv, fm, lin, amax)
    assert S.same_bits(concat.numpy().reshape(B, F, E), ref["concat"])
    assert S.max_err_scaled(sumv.numpy(), ref["sumv"]) < S.TOL and S.max_err_scaled(lin.numpy(), ref["lin"]) < S.TOL
    assert np.max(np.abs(fm.numpy() - ref["fm"]) / c["mag"]) < S.FM_BAR
    assert float(amax.max()) == float(ref["amax"]) < float(S.BIG)
    out_r, out_l = torch.empty(B * F, E), torch.empty(B * F)
    k.mi_gather_rows(_t(c["table"]), _t(c["lin_w"]), _t(c["rows"].reshape(-1).astype(np.int32)), B * F, E, out_r, out_l)
    assert S.same_bits(out_r.numpy(), ref["concat"].reshape(B * F, E)) and S.same_bits(out_l.numpy(), c["lin_w"][c["rows"].reshape(-1)])
    if which == "wide":
        return
    # the backward's per-entry gradients: c = 1
    seg = S.uniform_segments(B, F, 50)
    inp = S.grad_inputs(seg, E)
    cc = ref["concat"].reshape(B, F * E)
    ent = np.arange(B * F)
    dce, sve, gfe = S.entry_parts(ent, F, E, 0, inp["dc"], inp["sv"], inp["gf"])
    we = cc.reshape(B * F, E)
    d_rows, d_lin = torch.empty(B * F, E), torch.empty(B * F)
    k.mi_embed_fm_linear_bwd(_t(inp["dc"]), F * E, _t(cc), F * E, None, _t(inp["sv"]), _t(inp["gf"]), _t(inp["gl"]), None, B, F, E,
                             d_rows, d_lin)
    assert S.same_bits(d_rows.numpy(), S.values32(dce, sve, gfe, we))
    assert S.worst(d_rows.numpy(), S.values64(dce, sve, gfe, we), 4 * S.U24 * S.magnitudes(dce, sve, gfe, we)) <= 1
    assert S.same_bits(d_lin.numpy(), np.repeat(inp["gl"], F))


def test_stand_in_small_entries_against_the_references():
    k = NumpyKernels()
    B, nd, E, F = 9, 3, 12, 2
    q = S.numeric_inputs(B, nd, E)
    rng = np.random.default_rng(1)
    sumv0, fm0, lin0 = rng.standard_normal((B, E)).astype(F32), rng.standard_normal(B).astype(F32), rng.standard_normal(B).astype(F32)
    ref = S.numeric_embed_reference(q["x"], q["V"], q["w_num"], sumv0, fm0, lin0)
    ld, col0 = F * E + nd * E + 4, F * E
    concat = torch.full((B, ld), float("nan"))
    sumv, fm, lin = _t(sumv0.copy()), _t(fm0.copy()), _t(lin0.copy())
    k.mi_numeric_embed_fwd(_t(q["x"]), _t(q["V"]), _t(q["w_num"]), B, nd, E, concat, ld, col0, sumv, fm, lin)
    got = concat.numpy()
    assert S.same_bits(got[:, col0:col0 + nd * E], ref["concat"]) and np.isnan(got[:, :col0]).all() and np.isnan(got[:, col0 + nd * E:]).all()
    assert S.max_err_scaled(sumv.numpy(), ref["sumv"]) < S.TOL and S.max_err_scaled(lin.numpy(), ref["lin"]) < S.TOL
    assert np.max(np.abs(fm.numpy() - ref["fm"]) / ref["mag"]) < S.FM_BAR
    cols, acc = S.numeric_raw_reference(q["x"], q["w_num"], lin0, 8)
    concat = torch.full((B, 16), float("nan"))
    lin = _t(lin0.copy())
    k.mi_numeric_raw_fwd(_t(q["x"]), _t(q["w_num"]), B, nd, concat, 16, 4, 8, lin)
    assert S.same_bits(concat.numpy()[:, 4:12], cols) and np.isnan(concat.numpy()[:, :4]).all() and S.same_bits(lin.numpy(), acc)
    bits = S.nan_patterns(257)
    idx = rng.integers(0, 257, 300).astype(np.int32)
    out = torch.zeros(300, dtype=torch.int32)
    k.mi_gather_u32(_t(bits.view(np.int32)), _t(idx), 300, out)
    assert np.array_equal(out.numpy().view(np.uint32), bits[idx])
    x, y = rng.standard_normal(257).astype(F32), rng.standard_normal(257).astype(F32)
    yy = _t(y.copy())
    k.mi_axpy(yy, _t(x), 257, 0.3)
    exact = y.astype(np.float64) + float(F32(0.3)) * x.astype(np.float64)
    assert np.all(np.abs(yy.numpy() - exact) <= 2 * S.U24 * (np.abs(y) + np.abs(F32(0.3) * x)))
