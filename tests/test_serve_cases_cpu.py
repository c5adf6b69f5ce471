"""CPU: tests/serve_cases.py itself — the case list against what it claims to cover, the poison and the extents of the built
arrays, the loop reference against the fp64 stand-in of tests/cpu_kernels.py and against the oracle, and the fp32 evaluation
of the same formula: a case is only asked of the kernel at 1e-5 if fp32 itself stays within a quarter of that."""
import functools

import numpy as np
import pytest
import torch

from oracle import deepfm as O
from tests import serve_cases as SC
from tests.cpu_kernels import NumpyKernels
from tests.util import max_err_scaled

NAMES = [c.name for c in SC.CASES + SC.GROUP]
PARTS = ("lin", "fm", "dnn")
FP32_BOUND = 2.5e-6                  # a quarter of the kernel's contract (include/mi355x_rec.h: 1e-5, max_err_scaled)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(case, arrays, ids, x, fp64 reference) of a case, built once"""
    case = SC.BY_NAME[name]
    a = SC.build(case)
    ids, x = SC.requests(case)
    return case, a, ids, x, SC.reference(case, a, ids, x)


def _alone(part):
    return tuple(int(p == part) for p in PARTS)


def test_the_case_list_covers_what_it_claims():
    cs = SC.CASES
    assert len(set(NAMES)) == len(NAMES) == len(cs) + len(SC.GROUP) and all(c.guard for c in cs + SC.GROUP)
    assert all(SC.input_columns(c) <= SC.MAX_INPUT_COLUMNS for c in cs)
    cpf = {c.E // 4 for c in cs if c.F}
    assert {3, 5} <= cpf and 64 in cpf                                          # odd cpf (E = 12, 20); E = 256
    assert {0, 1, 2, 63, 64} <= {c.F for c in cs}
    assert {1, 2, 3, 7, 8, 9, 17} <= {c.F * c.E // 4 for c in cs}              # chunks of layer 1 around a block of 8
    kn = {c.nd * (1 if c.mode == "raw" else c.E) for c in cs if c.nd}
    assert {1, 3} <= kn and any(k % 2 == 0 for k in kn)                         # odd kn: raw columns, odd count
    assert {(c.nd, c.mode) for c in cs if c.nd and c.F} >= {(1, "raw"), (3, "raw"), (1, "embed"), (3, "embed")}
    assert any(c.F == 0 and c.mode == "embed" and c.parts == (1, 1, 1) and c.nd == 3 for c in cs)
    assert any(c.F == 0 and c.mode == "raw" and c.parts == (0, 0, 1) and c.nd == 1 for c in cs)
    outs = {w for c in cs for w in c.hidden}
    assert any(256 < w <= 384 for w in outs) and {257, 384} <= outs             # the 4-tile form with an idle wave
    assert {1, 31, 33, 129, 511, 512, 385} <= outs
    assert {1 + (w - 1) // 128 for w in outs} == {1, 2, 3, 4}
    assert any(len(c.hidden) == 8 for c in cs)                                  # both LDS buffers over 9 swaps
    fan_in = {w for c in cs for w in c.hidden}                                  # a hidden width is the next layer's fan-in
    assert {15, 16, 17, 31, 32, 33, 47, 48, 49} <= fan_in
    chain = [c for c in cs if c.hidden == SC.CHAIN]
    assert sorted(c.act for c in chain) == [0, 1, 2, 3] and all(c.act == 1 for c in cs if c.hidden != SC.CHAIN)
    for F in (63, 64):                                                          # mask bits at and above 32
        full = (1 << F) - 1
        masks = {c.wide for c in cs if c.F == F and c.hidden == (16,)}
        assert masks >= {full, SC.EDGE_BITS & full, full & ~SC.EDGE_BITS}
    assert any(c.wide >> 32 and c.wide != (1 << c.F) - 1 for c in cs)
    # and one mask whose words differ at every position a field uses: bit f is not bit f % 32
    assert any(c.F == 64 and all(((c.wide >> f) ^ (c.wide >> (f + 32))) & 1 for f in range(31)) for c in cs)
    assert any(c.F == 64 and c.hidden == (512, 512) for c in cs)                # the largest legal launch
    lds = max(SC.lds_bytes(c) for c in cs)
    assert lds == SC.lds_bytes(SC.BY_NAME["largest"]) == 139264 and lds + 4096 <= 160 * 1024
    assert {(c.ts - c.E, c.E) for c in cs if c.ts} >= {(4, 12), (20, 20)}       # table_stride = E + 4 and 2 E
    assert {2, 5} <= {c.ls for c in cs} and any(c.pad == 4 for c in cs)


@pytest.mark.parametrize("name", NAMES)
def test_poison_is_in_place_and_the_extents_are_finite(name):
    case, a, ids, x, _ = _problem(name)
    E, F = case.E, case.F
    assert a.table.dtype == a.lin_w.dtype == a.dense.dtype == np.float32
    assert a.layer_off.dtype == a.field_off.dtype == np.int64 and a.widths.dtype == np.int32
    assert np.isfinite(a.table[a.table_ok]).all() and np.isnan(a.table[~a.table_ok]).all()
    assert a.table.shape == (a.R, case.ts or E) and np.isfinite(a.table[:, :E]).all() and np.isnan(a.table[:, E:]).all()
    assert np.isfinite(a.lin_w[a.lin_ok]).all() and np.isnan(a.lin_w[~a.lin_ok]).all()
    for f in range(F):
        slots = (a.field_off[f] + np.arange(a.vocab[f])) * a.ls
        assert a.lin_ok[slots].all() == bool((case.wide >> f) & 1) and a.lin_ok[slots].any() == bool((case.wide >> f) & 1)
    assert a.lin_ok.sum() == sum(v for f, v in enumerate(a.vocab) if (case.wide >> f) & 1)
    d = a.dense
    assert np.isfinite(d[a.dense_ok]).all() and (d[a.dense_pad] == np.float32(SC.ROW_POISON)).all()
    assert np.isnan(d[~a.dense_ok & ~a.dense_pad]).all() and np.isnan(d[:3]).all() and np.isnan(d[-7:]).all()
    d_in, L = SC.input_columns(case), a.n_layers
    assert L == len(case.hidden) + 1 and a.widths.tolist() == [d_in + case.pad] + list(case.hidden) + [1]
    assert a.dense_pad.sum() == case.pad * a.widths[1]
    seen = np.zeros(d.size, bool)
    for i in range(L):                                              # every variable sits alone, NaN before and after it
        fi, fo = int(a.widths[i]), int(a.widths[i + 1])
        for at, n in ((int(a.layer_off[2 * i]), fi * fo), (int(a.layer_off[2 * i + 1]), fo)):
            assert np.isnan(d[at - 1]) and np.isnan(d[at + n]) and not seen[at:at + n].any()
            seen[at:at + n] = True
    k0 = d[a.layer_off[0]:a.layer_off[0] + a.widths[0] * a.widths[1]].reshape(a.widths[0], a.widths[1])
    assert np.isfinite(k0[:d_in]).all() and (k0[d_in:] == np.float32(SC.ROW_POISON)).all()
    if a.num_emb_off >= 0:
        assert a.num_emb_off % 4 == 0 and np.isnan(d[a.num_emb_off - 1]) and np.isnan(d[a.num_emb_off + case.nd * E])
    assert (a.lin_bias_off >= 0) == bool(case.parts[0]) and (a.lin_num_off >= 0) == bool(case.parts[0] and case.nd)
    assert (a.num_emb_off >= 0) == (case.mode == "embed")
    # the requests: id 0 and the last id of every field, every id inside its field
    assert ids.shape == (SC.B_MAX, F) and ids.dtype == np.int32
    if F:
        assert (ids[0] == 0).all() and (ids[1] == np.asarray(a.vocab) - 1).all()
        assert (ids >= 0).all() and (ids < np.asarray(a.vocab)[None, :]).all()
        assert int((a.field_off + np.asarray(a.vocab)).max()) == a.R
    assert (x is None) == (case.nd == 0) and (x is None or (x.shape == (SC.B_MAX, case.nd) and x.dtype == np.float32))


def _stand_in(case, a, ids, x, parts):
    """NumpyKernels.mi_predict_fused on the same arrays (the strides as views), its fp64 logits"""
    t = lambda v: None if v is None else torch.from_numpy(v)
    lin, fm, dnn = parts
    B = ids.shape[0]
    out = torch.full((B,), float("nan"), dtype=torch.float64)
    NumpyKernels().mi_predict_fused(
        t(a.table)[:, :case.E], a.ts, t(a.lin_w)[::a.ls], a.ls, t(a.field_off), t(ids), t(x), B, case.F, case.E, case.nd,
        t(a.dense), t(a.layer_off), t(a.widths), a.n_layers if dnn else 0, case.act, lin, fm, dnn, int(case.mode == "raw"),
        a.lin_bias_off, a.num_emb_off, a.lin_num_off, case.wide, out, None, None, None, None, 0)
    return out.numpy()


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_fp64_stand_in(name):
    case, a, ids, x, ref = _problem(name)
    err = max_err_scaled(_stand_in(case, a, ids, x, case.parts), ref["logits"])
    assert err < 1e-12, ("logits", err)
    for part, on in zip(PARTS, case.parts):
        if on:
            err = max_err_scaled(_stand_in(case, a, ids, x, _alone(part)), ref[part])
            assert err < 1e-12, (part, err)


def _oracle_params(case, a):
    f64 = np.float64
    d, E = a.dense.astype(f64), case.E
    off, voc = a.field_off, a.vocab
    emb = [a.table[off[f]:off[f] + voc[f], :E].astype(f64) for f in range(case.F)]
    lw = a.lin_w[::a.ls].astype(f64)
    lin_w = [lw[off[f]:off[f] + voc[f]] if (case.wide >> f) & 1 else np.zeros(voc[f]) for f in range(case.F)]
    d_in, mlp = SC.input_columns(case), []
    for i in range(a.n_layers):
        fi, fo = int(a.widths[i]), int(a.widths[i + 1])
        w0, b0 = int(a.layer_off[2 * i]), int(a.layer_off[2 * i + 1])
        mlp.append((d[w0:w0 + fi * fo].reshape(fi, fo)[:d_in if i == 0 else fi], d[b0:b0 + fo]))
    num_emb = d[a.num_emb_off:a.num_emb_off + case.nd * E].reshape(case.nd, E) if a.num_emb_off >= 0 else None
    lin_num = d[a.lin_num_off:a.lin_num_off + case.nd] if a.lin_num_off >= 0 else None
    bias = d[a.lin_bias_off:a.lin_bias_off + 1] if a.lin_bias_off >= 0 else np.zeros(1)
    return O.Params(emb, lin_w, bias, mlp, num_emb, lin_num)


# the oracle takes its embedding width from a table or from the numeric embeddings: F = 0 with raw columns has neither
ORACLE_NAMES = [n for n in NAMES if not (SC.BY_NAME[n].F == 0 and SC.BY_NAME[n].mode == "raw")]


def test_the_oracle_expresses_all_cases_but_one():
    assert sorted(set(NAMES) - set(ORACLE_NAMES)) == ["f0_raw1"]


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_reference_equals_the_oracle(name):
    case, a, ids, x, ref = _problem(name)
    lin, fm, dnn = case.parts
    c = O.forward(_oracle_params(case, a), ids, None if x is None else x.astype(np.float64), use_linear=bool(lin),
                  use_mf=bool(fm), use_dnn=bool(dnn), numeric=case.mode or "embed", activation=SC.ACT_NAMES[case.act],
                  wide_fields=[bool((case.wide >> f) & 1) for f in range(case.F)])
    assert c["logits"].dtype == np.float64
    assert max_err_scaled(c["logits"], ref["logits"]) < 1e-12
    for part, on in zip(PARTS, case.parts):
        if on:
            assert max_err_scaled(c[part], ref[part]) < 1e-12, part


def _fp32_errors(case, r32, ref):
    """per checked quantity, the worst max_err_scaled over the batch sizes the kernel is run at (every batch is a prefix
    of the 65 requests; with one request the measure is that request's relative error)"""
    keys = ["logits"] + [p for p, on in zip(PARTS, case.parts) if on]
    return {k: max(max_err_scaled(r32[k][:B], ref[k][:B]) for B in SC.BATCHES) for k in keys}


def test_fp32_formula_of_the_group_members_on_the_groups_requests():
    ids = SC.group_requests()
    for c in SC.GROUP:
        a = SC.build(c)
        ref, r32 = SC.reference(c, a, ids, None), SC.reference(c, a, ids, None, dtype=np.float32)
        errs = _fp32_errors(c, r32, ref)
        print("fp32 formula %-16s on the group's requests: %s" % (c.name, "  ".join("%s %.2e" % kv for kv in errs.items())))
        assert max(errs.values()) < FP32_BOUND, (c.name, errs)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_formula_stays_within_a_quarter_of_the_contract(name):
    case, a, ids, x, ref = _problem(name)
    r32 = SC.reference(case, a, ids, x, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in r32.values())
    errs = _fp32_errors(case, r32, ref)
    print("fp32 formula %-16s %s" % (name, "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert np.isfinite(ref["logits"]).all() and float(np.sqrt(np.mean(ref["logits"] ** 2))) > 0
    assert max(errs.values()) < FP32_BOUND, errs
    # the MLP's output is no constant: a relu layer of one unit leaves the bias for the requests it cuts off, and enough
    # of the others must still carry the layers before it
    assert len(np.unique(ref["dnn"])) > SC.B_MAX // 4, len(np.unique(ref["dnn"]))
