"""-m gpu: the sparse gradient path through the C ABI against the references of tests/sparse_cases.py — the per-row sum of the
entry gradients that feeds the optimizer rules (mi_entry_grads_segsum, mi_sparse_apply, mi_sparse_apply_fused), the per-entry
gradients (mi_embed_fm_linear_bwd), the gather in the layouts the host ships (mi_embed_fm_linear_fwd, mi_gather_rows) and the
small entries beside them (mi_numeric_embed_fwd, mi_numeric_raw_fwd, mi_gather_u32, mi_axpy).

The sums are held three ways: to the fp64 reference within the derived bar (c + 3) 2^-24 sum a_k; bit for bit to the fp32
restatement in the kernels' order — sequential up to 48 entries, sliced above; and, through the optimizer rules of
oracle/optimizers.py fed that restated sum, bit for bit to the parameter, both slots and the stamps.  The segments have
prescribed lengths at every edge of the slicing (48 | 49, G - 1, G, G + 1, 2 G + 3, one row of 2,000 entries), at E with and
without idle lanes.  Every buffer a kernel writes sits between NaN guard bands and is compared as a WHOLE with the expected
buffer's bits: pads, rows that were not asked for, slots the optimizer does not have and stamps it does not keep included.
Figures are printed (pytest -s): SPARSE <family> ... worst error as a fraction of its bar."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import sparse_cases as S
from tests.util import _chk, _p, _st, dev, guarded_nan, guards_intact

pytestmark = pytest.mark.gpu

F32 = np.float32
FORMS = {"full": dict(fm=True, dc=True, sumv=True), "no-fm": dict(fm=False, dc=True, sumv=True),
         "no-dc": dict(fm=True, dc=False, sumv=True), "no-sumv": dict(fm=True, dc=True, sumv=False)}
_WORST = {}


def _note(family, value):
    _WORST[family] = max(_WORST.get(family, 0.0), value)


def _flat(a):
    """a host fp32 array on the device between NaN guard bands: (whole buffer, flat view)"""
    a = np.ascontiguousarray(a, F32).reshape(-1)
    buf, v = guarded_nan(max(len(a), 1))
    v[:len(a)].copy_(torch.from_numpy(a))
    return buf, v[:len(a)]


def _at(v, off):
    """the address of element `off` of a device view"""
    return v.data_ptr() + 4 * int(off)


def _host(v):
    return v.cpu().numpy()


def _bits_equal(v, expected, what):
    got = _host(v)
    same = got.view(np.uint32) == np.ascontiguousarray(expected, F32).reshape(-1).view(np.uint32)
    assert same.all(), (what, "first differing element", int(np.flatnonzero(~same)[0]), "of", same.size, "differing", int((~same).sum()))


class _Case:
    """the prescribed-length segments of one E sorted on the device, their inputs, and the summed gradients per form (made
    once, shared by the tests of this module, never written)"""

    def __init__(self, lib, E):
        self.E = E
        self.seg = seg = S.prescribed_segments(E)
        self.inp = S.grad_inputs(seg, E)
        n = seg.n
        r = dev(seg.keys)
        self.se = torch.empty(n, dtype=torch.int32, device="cuda"); self.uq = torch.empty(n, dtype=torch.int32, device="cuda")
        self.sg = torch.empty(n + 1, dtype=torch.int32, device="cuda"); self.nu = torch.empty(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(lib.mi_sort_unique_workspace_bytes(n)) + 256, dtype=torch.uint8, device="cuda")
        _chk(lib.mi_sort_unique_rows(_p(r), n, seg.R, _p(self.se), _p(self.uq), _p(self.sg), _p(self.nu), _p(ws), ws.numel(), _st()))
        torch.cuda.synchronize()
        U = seg.U
        assert int(self.nu.item()) == U < n
        assert np.array_equal(_host(self.se), seg.order) and np.array_equal(_host(self.uq)[:U], seg.uniq)
        assert np.array_equal(_host(self.sg)[:U + 1], seg.seg)
        # slots past *num_uniq: a row nobody asked for with an empty segment — a kernel that looked there would move it
        self.untouched = np.setdiff1d(np.arange(seg.R), seg.uniq)
        assert len(self.untouched) > 50
        self.uq[U:] = int(self.untouched[0])
        self.sg[U + 1:] = n
        self._grads = {}

    def grads(self, form):
        if form not in self._grads:
            self._grads[form] = S.RowGrads(self.seg, self.inp, self.E, self.inp["w"][self.seg.uniq], **FORMS[form])
        return self._grads[form]


@pytest.fixture(scope="module")
def cases(lib):
    made = {}

    def get(E):
        if E not in made:
            made[E] = _Case(lib, E)
        return made[E]
    return get


# ---- mi_entry_grads_segsum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", S.SUM_E)
def test_entry_grads_segsum_against_fp64_and_the_restated_order(lib, cases, E):
    c = cases(E)
    seg, inp = c.seg, c.inp
    F, U = seg.F, seg.U
    w_u = inp["w"][seg.uniq]
    ranges = [("whole", 0, U, 0, 0), ("chunk, out at 0", seg.U0, U, seg.b0, 0), ("chunk, out at its base", seg.U0, U, seg.b0, seg.U0),
              ("inside the long run", seg.run0 + 7, seg.run0 + 40, 0, seg.run0 + 7)]
    assert seg.counts[seg.run0 + 7] == S.groups(E) and seg.counts[seg.run0 + 10] == S.LONG_ROW
    assert seg.b0 > 0 and seg.U0 > 0                         # the chunk: b0 > 0, its requests after the first chunk's
    worst = 0.0
    for form, lin_only, (what, lo, hi, b0, row0), (rs, os_) in itertools.product(
            ("full", "no-fm", "no-dc"), (False, True), ranges, ((0, 0), (E + 4, E + 8))):
        if lin_only and form != "full":
            continue
        g = c.grads(form)
        fm, dc = FORMS[form]["fm"], FORMS[form]["dc"]
        rows_p = S.pack_records(rs, w_u, inp["lw"][seg.uniq])               # the exchange's receive buffer: slot u = request u
        _, d_rows_in = _flat(rows_p.flat)
        _, d_dc = _flat(inp["dc"][b0:])
        d_sv, d_gf, d_gl = dev(inp["sv"][b0:]), dev(inp["gf"][b0:]), dev(inp["gl"][b0:])
        n_out = hi - row0 + 2
        exp_r, exp_l = np.full((n_out, E), S.NAN, F32), np.full(n_out, S.NAN, F32)
        if not lin_only:
            exp_r[lo - row0:hi - row0] = g.g32[lo:hi]
        exp_l[lo - row0:hi - row0] = (g.l32_alone if lin_only else g.l32)[lo:hi]   # (no rows: one lane per request, 256 slices)
        out_p = S.pack_records(os_, np.full((n_out, E), S.NAN, F32), None)
        obuf, out = _flat(out_p.flat)
        _chk(lib.mi_entry_grads_segsum(_at(d_rows_in, rows_p.off[0]) if fm and not lin_only else None, _p(c.sg), _p(c.se), lo, hi - lo,
                                       _p(d_dc) if dc and not lin_only else None, F * E, _p(d_sv) if fm and not lin_only else None,
                                       _p(d_gf) if fm and not lin_only else None, _p(d_gl), b0, F, E,
                                       None if lin_only else _at(out, out_p.off[0]), _at(out, out_p.off[1]), row0, rs, os_, _st()),
             "mi_entry_grads_segsum")
        torch.cuda.synchronize()
        tag = "E=%d %s %s%s rows_stride=%d out_stride=%d" % (E, form, what, ", out_lin alone" if lin_only else "", rs, os_)
        assert guards_intact(obuf), tag
        got_r, got_l, _ = S.unpack_records(os_, _host(out), n_out, E)
        a = 0.0 if lin_only else S.worst(got_r[lo - row0:hi - row0], g.g64[lo:hi], g.bar[lo:hi])
        b = S.worst(got_l[lo - row0:hi - row0], g.l64[lo:hi], g.lbar[lo:hi])
        worst = max(worst, a, b)
        assert a <= 1 and b <= 1, (tag, a, b)
        # sequential up to 48 entries, sliced above; rows outside the range, the records' pads: untouched
        _bits_equal(out, S.pack_records(os_, exp_r, exp_l).flat, tag)
    _note("segsum", worst)
    print("SPARSE segsum E=%-3d worst |sum - sum64| / bar %.3f (rows and out_lin; 4 forms x 4 ranges x 2 layouts)" % (E, worst))


# ---- mi_sparse_apply, mi_sparse_apply_fused ------------------------------------------------------------------------------------------
APPLY_LAYOUTS = [("arrays", 1, 0), ("rec3", 4, 4), ("rowpad", 4, 8)]          # (table layout, lin_stride, grad record = E + this)
FUSED_RUNS = [("full", "arrays", 1), ("full", "rec3", 4), ("full", "rowpad", 1), ("no-sumv", "rec3", 4), ("no-sumv", "arrays", 1),
              ("no-dc", "rowpad", 4), ("wide alone", "arrays", 1), ("wide alone", "arrays", 4)]


def _expected_state(name, c, g, hp, lr_t, st, table_on=True):
    """(table, slot0, slot1 [R, E]; wide w, slot0, slot1 [R]; stamps [R]) after the apply, from the restated sums"""
    seg, inp = c.seg, c.inp
    rows = seg.uniq
    stamps = st["stamp"][rows] if name == "Adam" else None
    T, t0, t1 = inp["w"].copy(), None if st["s0"] is None else st["s0"].copy(), None if st["s1"] is None else st["s1"].copy()
    if table_on:
        w, a, b = S.apply_rows(hp, inp["w"][rows], None if t0 is None else t0[rows], None if t1 is None else t1[rows], stamps,
                               g.g32, S.STEP, lr_t)
        T[rows] = w
        if t0 is not None:
            t0[rows] = a
        if t1 is not None:
            t1[rows] = b
    L, l0, l1 = inp["lw"].copy(), None if st["l0"] is None else st["l0"].copy(), None if st["l1"] is None else st["l1"].copy()
    w, a, b = S.apply_rows(hp, inp["lw"][rows, None], None if l0 is None else l0[rows, None], None if l1 is None else l1[rows, None],
                           stamps, (g.l32 if table_on else g.l32_alone)[:, None], S.STEP, lr_t)
    L[rows] = w[:, 0]
    if l0 is not None:
        l0[rows] = a[:, 0]
    if l1 is not None:
        l1[rows] = b[:, 0]
    stamp = st["stamp"].copy()
    if name == "Adam":
        stamp[rows] = S.STEP
    return T, t0, t1, L, l0, l1, stamp


@pytest.mark.parametrize("name", ["SGD", "Adagrad", "Adam"])
@pytest.mark.parametrize("E", S.SUM_E)
def test_sparse_apply_and_fused_bit_exact_on_the_restated_sum(lib, cases, E, name):
    from mi355x_rec.engine import OptimizerSpec
    c = cases(E)
    seg, inp = c.seg, c.inp
    F, n, R = seg.F, seg.n, seg.R
    hp = S.hyper(name)
    lr_t = S.lr_t_of(hp, S.STEP) if name == "Adam" else 0.0
    h = OptimizerSpec(name, hp.lr).hparams(lr_t)
    st = S.row_state(name, seg, E)
    adam = name == "Adam"
    if adam:                                                 # rows with long and with short segments in every class of staleness
        for sel, never in ((seg.counts > S.K_LONG, set()), (seg.counts <= S.K_LONG, {0})):     # (three long rows at E >= 64)
            assert set(st["stamp"][seg.uniq[sel]][:4]) >= {S.STEP - 1, S.STEP - 2, S.STEP - 6} | never
    need0, need1 = name != "SGD", adam
    expected = {}
    worst = 0.0

    def run(form, layout, ls, fused, grad_pad=0):
        nonlocal worst
        table_on = form != "wide alone"
        g = c.grads(form if table_on else "full")
        key = (form if table_on else "wide alone")
        if key not in expected:
            expected[key] = _expected_state(name, c, g, hp, lr_t, st, table_on)
            if name == "SGD" and table_on:                   # w - lr * g with g from the restatement, and g within the bar of fp64
                assert S.same_bits(expected[key][0][seg.uniq], inp["w"][seg.uniq] - g.g32 * F32(hp.lr))
                worst = max(worst, S.worst(g.g32, g.g64, g.bar), S.worst(g.l32, g.l64, g.lbar))
        T, t0, t1, L, l0, l1, stamp = expected[key]
        tp = S.pack_table(layout, inp["w"], st["s0"], st["s1"])
        wp = S.pack_wide(ls, inp["lw"], st["l0"], st["l1"], st["stamp"])
        assert tp.stride == {"arrays": 0, "rec3": 3 * E, "rowpad": E + 4}[layout] and wp.stride == ls    # table_stride, lin_stride
        tbuf, tv = _flat(tp.flat)
        wbuf, wv = _flat(wp.flat)
        tab = [_at(tv, o) for o in tp.off] if table_on else [None] * 3
        wide = [_at(wv, o) for o in wp.off]
        args = (tab[0], tab[1] if need0 and table_on else None, tab[2] if need1 and table_on else None, wide[0],
                wide[1] if need0 else None, wide[2] if need1 else None, wide[3] if adam else None, _p(c.uq), _p(c.sg), _p(c.se), _p(c.nu), n)
        d_gl = dev(inp["gl"])
        if fused:
            keep = [_flat(g.dc_in)[1] if FORMS.get(form, {}).get("dc") and table_on else None,
                    dev(inp["sv"]) if table_on and FORMS[form]["sumv"] else None, dev(inp["gf"]) if table_on else None]
            _chk(lib.mi_sparse_apply_fused(*args, _p(keep[0]), F * E, _p(keep[1]), _p(keep[2]), _p(d_gl), F, E, S.STEP, C.byref(h), ls,
                                           tp.stride, _st()), "mi_sparse_apply_fused")
        else:
            gp = S.pack_records(E + grad_pad if grad_pad else 0, g.v32, g.gl_entry)
            gbuf, gv = _flat(gp.flat)
            _chk(lib.mi_sparse_apply(*args, _at(gv, gp.off[0]), _at(gv, gp.off[1]), E, S.STEP, C.byref(h), ls, tp.stride, gp.stride, _st()),
                 "mi_sparse_apply")
        torch.cuda.synchronize()
        tag = "E=%d %s %s %s table %s lin_stride %d grad record +%d" % (E, name, "fused" if fused else "unfused", form, layout, ls, grad_pad)
        assert guards_intact(tbuf) and guards_intact(wbuf), tag
        # parameter, both slots, stamps; rows not asked for, slots past *num_uniq, pads, absent slots: the whole buffers
        _bits_equal(tv, S.pack_table(layout, T, t0, t1).flat if table_on else tp.flat, tag + ": table")
        _bits_equal(wv, S.pack_wide(ls, L, l0, l1, stamp).flat, tag + ": wide part")

    for layout, ls, pad in APPLY_LAYOUTS:
        run("full", layout, ls, False, pad)
    run("full", "arrays", 1, False, 0)                       # a second launch on fresh copies: the same bits
    run("full", "arrays", 4, False, 4)
    for form, layout, ls in FUSED_RUNS:
        run(form, layout, ls, True)
    run("full", "rec3", 4, True)                             # ... and of the fused form
    if name == "SGD":
        _note("apply (SGD: the sum itself)", worst)
        print("SPARSE apply E=%-3d restated sum against fp64: worst / bar %.3f; %d launches bit-identical to the rule on it" % (
            E, worst, len(APPLY_LAYOUTS) + 3 + len(FUSED_RUNS)))


# ---- mi_embed_fm_linear_bwd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", S.SUM_E)
def test_embed_fm_linear_bwd_every_subset_against_fp64(lib, E):
    L, G = S.lanes_per_row(E), S.groups(E)
    worst = 0.0
    for F, B in itertools.product(sorted({1, L + 1}), (1, G + 1)):
        n = B * F
        seg = S.uniform_segments(B, F, 40)
        inp = S.grad_inputs(seg, E, ld_pad=8)
        rng = np.random.default_rng([E, F, B])
        cc = np.full((B, F * E + 4), S.NAN, F32)
        cc[:, :F * E] = rng.standard_normal((B, F * E))
        perm = rng.permutation(n).astype(np.int32)
        ent = np.arange(n)
        _, d_dc = _flat(inp["dc"]); _, d_cc = _flat(cc)
        d_sv, d_gf, d_gl = dev(inp["sv"]), dev(inp["gf"]), dev(inp["gl"])
        for use_dc, use_fm, use_lin, use_pos, by_rows in itertools.product((1, 0), (1, 0), (1, 0), (0, 1), (0, 1)):
            if by_rows and not use_fm:
                continue
            pos = perm if use_pos else ent.astype(np.int32)
            dce, sve, gfe = S.entry_parts(ent, F, E, 0, inp["dc"] if use_dc else None, inp["sv"] if use_fm else None,
                                          inp["gf"] if use_fm else None)
            we = cc[:, :F * E].reshape(n, E)
            by_slot = np.empty((n, E), F32); by_slot[pos] = we
            d_slot = dev(by_slot)
            d_pos = dev(pos)
            rbuf, d_rows = guarded_nan(n, E)
            lbuf, d_lin = guarded_nan(n)
            _chk(lib.mi_embed_fm_linear_bwd(_p(d_dc) if use_dc else None, F * E + 8, None if by_rows or not use_fm else _p(d_cc), F * E + 4,
                                            _p(d_slot) if by_rows else None, _p(d_sv) if use_fm else None, _p(d_gf) if use_fm else None,
                                            _p(d_gl) if use_lin else None, _p(d_pos) if use_pos else None, B, F, E, _p(d_rows),
                                            _p(d_lin) if use_lin else None, _st()), "mi_embed_fm_linear_bwd")
            torch.cuda.synchronize()
            tag = (E, F, B, use_dc, use_fm, use_lin, use_pos, by_rows)
            assert guards_intact(rbuf) and guards_intact(lbuf), tag
            got = _host(d_rows)[pos]
            bar = 4 * S.U24 * S.magnitudes(dce, sve, gfe, we)            # c = 1: (c + 3) 2^-24 a_k
            a = S.worst(got, S.values64(dce, sve, gfe, we), bar)
            worst = max(worst, a)
            assert a <= 1, (tag, a)
            assert S.same_bits(got, S.values32(dce, sve, gfe, we)), tag   # the order the fused apply rebuilds it in
            gl = _host(d_lin)
            assert S.same_bits(gl[pos], np.repeat(inp["gl"], F)) if use_lin else np.isnan(gl).all(), tag
        # the wide part alone (d_rows == NULL)
        lbuf, d_lin = guarded_nan(n)
        d_pos = dev(perm)
        _chk(lib.mi_embed_fm_linear_bwd(None, 0, None, 0, None, None, None, _p(d_gl), _p(d_pos), B, F, E, None, _p(d_lin), _st()))
        torch.cuda.synchronize()
        assert guards_intact(lbuf) and S.same_bits(_host(d_lin)[perm], np.repeat(inp["gl"], F))
        # what the header rules out comes back as an error: concat AND rows; d_lin without d_logit_lin; the FM term without sumv
        rbuf, d_rows = guarded_nan(n, E)
        d_slot = dev(cc[:, :F * E].reshape(n, E).copy())
        assert lib.mi_embed_fm_linear_bwd(_p(d_dc), F * E + 8, _p(d_cc), F * E + 4, _p(d_slot), _p(d_sv), _p(d_gf), _p(d_gl), None, B, F, E,
                                          _p(d_rows), _p(d_lin), _st()) != 0
        assert lib.mi_embed_fm_linear_bwd(_p(d_dc), F * E + 8, _p(d_cc), F * E + 4, None, _p(d_sv), _p(d_gf), None, None, B, F, E,
                                          _p(d_rows), _p(d_lin), _st()) != 0
        assert lib.mi_embed_fm_linear_bwd(_p(d_dc), F * E + 8, _p(d_cc), F * E + 4, None, None, _p(d_gf), _p(d_gl), None, B, F, E,
                                          _p(d_rows), _p(d_lin), _st()) != 0
        torch.cuda.synchronize()
        assert torch.isnan(d_rows).all()
    _note("bwd", worst)
    print("SPARSE bwd E=%-3d worst |d_rows - fp64| / (4 * 2^-24 a) %.3f" % (E, worst))


# ---- mi_embed_fm_linear_fwd, mi_gather_rows ------------------------------------------------------------------------------------------
def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("which", S.FWD_SETS)
@pytest.mark.parametrize("E", S.FWD_E)
def test_embed_fm_linear_fwd_in_the_shipped_layouts(lib, E, which):
    Fs, Bs = S.fwd_shapes(E)
    w_sumv = w_fm = w_lin = 0.0
    launches = 0
    for F, B in itertools.product(Fs, Bs):
        c = S.fwd_case(E, F, B, which)
        ref = S.fwd_reference(c)
        fo, di = dev(c["off"]), dev(c["ids"])
        first = None
        combos = [(layout, ls) for layout in S.TABLE_LAYOUTS for ls in (1, 4)] + [("rec3", 4)]
        for i, (layout, ls) in enumerate(combos):
            no_concat = i == len(combos) - 1
            # pads NaN, the slot columns of the records 3e38 (and the unread row, in every layout)
            tp = S.pack_table(layout, c["table"], None, None, fill=S.BIG if layout == "rec3" else S.NAN)
            wp = S.pack_wide(ls, c["lin_w"], fill=S.BIG)
            _, tv = _flat(tp.flat); _, wv = _flat(wp.flat)
            ld = F * E + (8 if i % 2 else 0)
            cbuf, concat = guarded_nan(B, ld)
            sbuf, sumv = guarded_nan(B, E)
            fbuf, fm = guarded_nan(B)
            lbuf, lin = guarded_nan(B)
            amax = torch.zeros(64, device="cuda")
            _chk(lib.mi_embed_fm_linear_fwd(_at(tv, tp.off[0]), _at(wv, wp.off[0]), _p(fo), _p(di), B, F, E, None if no_concat else _p(concat),
                                            0 if no_concat else ld, _p(sumv), _p(fm), _p(lin), _p(amax), ls, tp.stride, _st()),
                 "mi_embed_fm_linear_fwd")
            launches += 1
            tag = (E, F, B, which, layout, ls, ld, no_concat)
            ok = guards_intact(cbuf) and guards_intact(sbuf) and guards_intact(fbuf) and guards_intact(lbuf)
            assert ok, tag
            top = amax.max()
            if first is None:
                got = _host(concat)
                assert S.same_bits(got[:, :F * E].reshape(B, F, E), ref["concat"]), tag          # -0.0 and denormals included
                a = S.max_err_scaled(_host(sumv), ref["sumv"])
                b = float(np.max(np.abs(_host(fm).astype(np.float64) - ref["fm"]) / c["mag"]))
                d = S.max_err_scaled(_host(lin), ref["lin"])
                w_sumv, w_fm, w_lin = max(w_sumv, a / S.TOL), max(w_fm, b / S.FM_BAR), max(w_lin, d / S.TOL)
                assert a < S.TOL and b < S.FM_BAR and d < S.TOL, (tag, a, b, d)
                if F == 1:
                    assert np.all(_host(fm) == 0.0), tag
                # the largest |value| of the rows read, exactly; never the 3e38 of the unread row or of a slot column
                assert float(top) == float(ref["amax"]) < float(S.BIG), (tag, float(top), float(ref["amax"]))
                first = (concat[:, :F * E].clone(), sumv.clone(), fm.clone(), lin.clone(), top.clone())
            else:                                            # the layout moves no bit of any output
                if no_concat:
                    assert torch.isnan(concat).all(), tag
                else:
                    assert torch.equal(_i32(concat[:, :F * E]), _i32(first[0])) and torch.isnan(concat[:, F * E:]).all(), tag
                same = torch.equal(_i32(sumv), _i32(first[1])) and torch.equal(_i32(fm), _i32(first[2])) and \
                    torch.equal(_i32(lin), _i32(first[3])) and torch.equal(top, first[4])
                assert same, tag
    _note("fwd sumv", w_sumv); _note("fwd fm", w_fm); _note("fwd lin", w_lin)
    print("SPARSE fwd E=%-3d %-6s worst / bar: sumv %.3f, fm %.3f, lin %.3f (%d shapes, %d launches)" % (
        E, which, w_sumv, w_fm, w_lin, len(Fs) * len(Bs), launches))


@pytest.mark.parametrize("E", S.FWD_E)
def test_gather_rows_in_the_shipped_layouts(lib, E):
    G = S.groups(E)
    c = S.fwd_case(E, 5, 3, "wide")
    R = c["R"]
    for n in (1, 7, 8, 9, 8 * G + 1):
        rows = np.random.default_rng([E, n]).integers(0, R - 1, n).astype(np.int32)
        rows[0] = c["rows"][0, 0]                              # (a row with -0.0 and denormals)
        d_rows = dev(rows)
        for layout, ls, out_s, part in itertools.product(S.TABLE_LAYOUTS, (1, 4), (0, E + 4), ("both", "table", "wide")):
            tp = S.pack_table(layout, c["table"], None, None, fill=S.BIG if layout == "rec3" else S.NAN)
            wp = S.pack_wide(ls, c["lin_w"], fill=S.BIG)
            _, tv = _flat(tp.flat); _, wv = _flat(wp.flat)
            op = S.pack_records(out_s, np.full((n, E), S.NAN, F32), None)
            obuf, out = _flat(op.flat)
            tab, wide = part != "wide", part != "table"
            _chk(lib.mi_gather_rows(_at(tv, tp.off[0]) if tab else None, _at(wv, wp.off[0]) if wide else None, _p(d_rows), n, E,
                                    _at(out, op.off[0]) if tab else None, _at(out, op.off[1]) if wide else None, ls, tp.stride, out_s, _st()),
                 "mi_gather_rows")
            torch.cuda.synchronize()
            tag = (E, n, layout, ls, out_s, part)
            assert guards_intact(obuf), tag
            exp = S.pack_records(out_s, c["table"][rows] if tab else np.full((n, E), S.NAN, F32), c["lin_w"][rows] if wide else None)
            _bits_equal(out, exp.flat, tag)


# ---- the small entries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [4, 12, 100])
@pytest.mark.parametrize("B", [1, 255, 257])
def test_numeric_embed_fwd_on_top_of_a_categorical_forward(lib, B, E):
    """B across a block edge for E = 4 (256 examples a block); E = 12 and 100 leave lanes idle"""
    nd, F = 3, 2
    B = B if E == 4 else (B + 3) // 4 if E == 12 else (B + 31) // 32        # around G examples a block at every E
    q = S.numeric_inputs(B, nd, E)
    c = S.fwd_case(E, F, B, "normal")
    fo, di, t, lw = dev(c["off"]), dev(c["ids"]), dev(c["table"]), dev(c["lin_w"])
    col0 = F * E
    ld = col0 + nd * E + 4
    cbuf, concat = guarded_nan(B, ld)
    sbuf, sumv = guarded_nan(B, E); fbuf, fm = guarded_nan(B); lbuf, lin = guarded_nan(B)
    _chk(lib.mi_embed_fm_linear_fwd(_p(t), _p(lw), _p(fo), _p(di), B, F, E, _p(concat), ld, _p(sumv), _p(fm), _p(lin), None, 1, 0, _st()))
    torch.cuda.synchronize()
    sumv0, fm0, lin0, cat0 = _host(sumv).copy(), _host(fm).copy(), _host(lin).copy(), _host(concat).copy()
    d = [dev(q[k]) for k in ("x", "V", "w_num")]
    _chk(lib.mi_numeric_embed_fwd(_p(d[0]), _p(d[1]), _p(d[2]), B, nd, E, _p(concat), ld, col0, _p(sumv), _p(fm), _p(lin), _st()),
         "mi_numeric_embed_fwd")
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in (cbuf, sbuf, fbuf, lbuf))
    ref = S.numeric_embed_reference(q["x"], q["V"], q["w_num"], sumv0, fm0, lin0)
    got = _host(concat)
    assert S.same_bits(got[:, col0:col0 + nd * E], ref["concat"])               # one rounding: the fp32 product
    assert S.same_bits(got[:, :col0], cat0[:, :col0]) and np.isnan(got[:, col0 + nd * E:]).all()
    a, b = S.max_err_scaled(_host(sumv), ref["sumv"]), S.max_err_scaled(_host(lin), ref["lin"])
    e = float(np.max(np.abs(_host(fm) - ref["fm"]) / ref["mag"]))
    _note("numeric_embed sumv", a / S.TOL); _note("numeric_embed fm", e / S.FM_BAR); _note("numeric_embed lin", b / S.TOL)
    assert a < S.TOL and b < S.TOL and e < S.FM_BAR, (a, b, e)
    # without the optional outputs: the concat columns alone, the same bits
    cbuf2, concat2 = guarded_nan(B, ld)
    _chk(lib.mi_numeric_embed_fwd(_p(d[0]), _p(d[1]), None, B, nd, E, _p(concat2), ld, col0, None, None, None, _st()))
    torch.cuda.synchronize()
    assert guards_intact(cbuf2) and S.same_bits(_host(concat2)[:, col0:col0 + nd * E], ref["concat"])
    assert np.isnan(_host(concat2)[:, :col0]).all()


@pytest.mark.parametrize("B", [1, 256, 257])
def test_numeric_raw_fwd_pads_with_zeros_and_adds_in_column_order(lib, B):
    nd, n_cols, col0, ld = 5, 16, 8, 28
    q = S.numeric_inputs(B, nd, 4)
    lin0 = np.random.default_rng(B).standard_normal(B).astype(F32)
    cols, acc = S.numeric_raw_reference(q["x"], q["w_num"], lin0, n_cols)
    dx, dw = dev(q["x"]), dev(q["w_num"])
    for with_concat, with_lin in ((1, 1), (1, 0), (0, 1)):
        cbuf, concat = guarded_nan(B, ld)
        lbuf, lin = _flat(lin0)
        _chk(lib.mi_numeric_raw_fwd(_p(dx), _p(dw) if with_lin else None, B, nd, _p(concat) if with_concat else None, ld, col0, n_cols,
                                    _p(lin) if with_lin else None, _st()), "mi_numeric_raw_fwd")
        torch.cuda.synchronize()
        assert guards_intact(cbuf) and guards_intact(lbuf)
        got = _host(concat)
        if with_concat:
            assert S.same_bits(got[:, col0:col0 + n_cols], cols) and np.isnan(got[:, :col0]).all() and np.isnan(got[:, col0 + n_cols:]).all()
        else:
            assert np.isnan(got).all()
        assert S.same_bits(_host(lin), acc if with_lin else lin0)
    assert lib.mi_numeric_raw_fwd(_p(dx), None, B, nd, None, ld, col0, n_cols, _p(lin), _st()) != 0      # lin needs w_num


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_gather_u32_moves_bit_patterns(lib, n):
    rng = np.random.default_rng(n)
    src = S.nan_patterns(300)
    idx = rng.integers(0, 300, n).astype(np.int32)
    idx[-1] = 0                                              # (a NaN payload)
    for view in (torch.int32, torch.float32):
        d_src = dev(src.view(np.int32)).view(view)
        d_idx = dev(idx)
        obuf, out = guarded_nan(n)
        out = out.view(view)
        _chk(lib.mi_gather_u32(_p(d_src), _p(d_idx), n, _p(out), _st()), "mi_gather_u32")
        torch.cuda.synchronize()
        assert guards_intact(obuf)
        assert np.array_equal(_host(out.view(torch.int32)).view(np.uint32), src[idx])


@pytest.mark.parametrize("n", [0, 1, 255, 257, 4097])
def test_axpy_rounds_the_product_and_the_sum_once_each(lib, n):
    rng = np.random.default_rng(n + 1)
    x, y = rng.standard_normal(n + 3).astype(F32), rng.standard_normal(n + 3).astype(F32)
    alpha = F32(0.3)
    dx = dev(x)
    ybuf, dy = _flat(y)
    _chk(lib.mi_axpy(_p(dy), _p(dx), n, float(alpha), _st()), "mi_axpy")
    torch.cuda.synchronize()
    got = _host(dy)
    assert guards_intact(ybuf) and S.same_bits(got[n:], y[n:])                  # past n: untouched
    exact = y[:n].astype(np.float64) + float(alpha) * x[:n].astype(np.float64)
    # alpha x rounded once (2^-24 |alpha x|), the sum once (2^-24 |result|): no operation more, none fused away
    bar = S.U24 * (np.abs(float(alpha) * x[:n].astype(np.float64)) + np.abs(exact)) * (1 + 2 * S.U24)
    assert np.all(np.abs(got[:n] - exact) <= bar)
    assert S.same_bits(got[:n], y[:n] + alpha * x[:n])
    if n:
        _note("axpy", float(np.max(np.abs(got[:n] - exact) / bar)))


def test_summary_lines():
    """one SPARSE line per family: the worst measured error as a fraction of its bar (run last; pytest -s)"""
    for family in sorted(_WORST):
        print("SPARSE worst %-32s %.3f of its bar" % (family, _WORST[family]))
    assert all(v <= 1.0 for v in _WORST.values()), _WORST
