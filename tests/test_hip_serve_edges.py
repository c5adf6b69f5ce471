"""-m gpu: the one-launch serving forward (csrc/serve.hip: mi_predict_fused, mi_predict_group) through the C entry, on the
models of tests/serve_cases.py — each stands at one guard of the kernel's loops — against that module's fp64 loop reference.

Every array the entry reads carries poison outside its extents (NaN between table rows, linear weights and the variables of
the dense buffer; 1e30 in the rows of kernel_0 past the input columns), every output lies between guard bands.  Per case
and batch size: the logits within the header's 1e-5 (max_err_scaled); the DNN and the FM term each once more on their
own, so that the larger part does not hide the smaller one's error; the head's outputs bit for bit against
mi_binary_predictions; a request's bits independent of the batch around it.  Then each output requested alone, and an
ensemble of three members that differ most in LDS need.  What was measured, and which deliberate errors in the kernel this
file catches: profiles/serve_edges.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from tests import serve_cases as SC
from tests.util import GUARD, _chk, _p, _st, dev, guarded_nan, guards_intact, max_err_scaled

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in SC.CASES]
CONTRACT = 1e-5                      # include/mi355x_rec.h: "Within 1e-5 of an fp64 forward, scaled as max_err_scaled"
CLS_FILL = -7
DNN_ALONE, FM_ALONE, LIN_ALONE = (0, 0, 1), (0, 1, 0), (1, 0, 0)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(case, host arrays, device arrays, ids, x, fp64 reference of the 65 requests), made once per case"""
    case = SC.BY_NAME[name]
    a = SC.build(case)
    ids, x = SC.requests(case)
    d = dict(table=dev(a.table) if a.R else None, lin_w=dev(a.lin_w) if a.R else None,
             field_off=dev(a.field_off) if case.F else None, dense=dev(a.dense),
             layer_off=torch.from_numpy(a.layer_off), widths=torch.from_numpy(a.widths))          # (host, as the entry wants)
    return case, a, d, ids, x, SC.reference(case, a, ids, x)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Outs:
    """the four outputs of B requests between their guard bands (`only`: the others stay NULL)"""

    def __init__(self, B, only=None):
        self.B, self.whole = B, {}
        self.logits = self.logistic = self.probabilities = self.class_ids = None
        for key, shape in (("logits", (B,)), ("logistic", (B,)), ("probabilities", (B, 2))):
            if only in (None, key):
                self.whole[key], view = guarded_nan(*shape)
                setattr(self, key, view)
        if only in (None, "class_ids"):
            self.cls_whole = torch.full((B + 2 * GUARD,), CLS_FILL, dtype=torch.int64, device="cuda")
            self.class_ids = self.cls_whole[GUARD:GUARD + B]

    def pointers(self):
        return [_p(self.logits), _p(self.logistic), _p(self.probabilities), _p(self.class_ids)]

    def check_written_inside_only(self):
        for key, buf in self.whole.items():
            assert guards_intact(buf), key
            assert not bool(torch.isnan(getattr(self, key)).any()), key
        if self.class_ids is not None:
            w = self.cls_whole
            assert bool((w[:GUARD] == CLS_FILL).all()) and bool((w[-GUARD:] == CLS_FILL).all())
            assert bool(((self.class_ids == 0) | (self.class_ids == 1)).all())


def _serve(lib, case, a, d, ids_d, x_d, B, parts, outs):
    """one call of mi_predict_fused on the case's arrays with the parts (linear, fm, dnn) switched as given"""
    lin, fm, dnn = parts
    L = a.n_layers if dnn else 0
    _chk(lib.mi_predict_fused(_p(d["table"]), a.ts, _p(d["lin_w"]), a.ls, _p(d["field_off"]), _p(ids_d), _p(x_d), B, case.F,
                              case.E, case.nd, _p(d["dense"]), _p(d["layer_off"]) if L else None,
                              _p(d["widths"]) if L else None, L, case.act, lin, fm, dnn, int(case.mode == "raw"),
                              a.lin_bias_off, a.num_emb_off, a.lin_num_off, case.wide if lin else 0, *outs.pointers(),
                              None, 0, _st()), "mi_predict_fused")
    torch.cuda.synchronize()
    outs.check_written_inside_only()


def _inputs(case, ids, x, B):
    """the first B requests as device tensors of exactly B rows"""
    return (dev(ids[:B]) if case.F else None), (dev(x[:B]) if case.nd else None)


def _check_head(lib, o):
    """logistic, probabilities and class_ids are mi_binary_predictions on the returned logits, bit for bit"""
    B = o.B
    ref = Outs(B)
    _chk(lib.mi_binary_predictions(_p(o.logits), None, B, _p(ref.logistic), _p(ref.probabilities), _p(ref.class_ids), None, _st()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(o.logistic), _bits(ref.logistic))
    assert torch.equal(_bits(o.probabilities), _bits(ref.probabilities))
    assert torch.equal(o.class_ids, ref.class_ids)


@pytest.mark.parametrize("name", NAMES)
def test_logits_and_each_part_match_fp64(lib, name):
    case, a, d, ids, x, ref = _problem(name)
    kept = {}
    for B in SC.BATCHES:
        ids_d, x_d = _inputs(case, ids, x, B)
        runs = [("logits", case.parts), ("dnn", DNN_ALONE)] + ([("fm", FM_ALONE)] if case.parts[1] else [])
        if case.parts[0] and case.mode != "embed":                   # (numeric embeddings need the FM term or the DNN)
            runs.append(("lin", LIN_ALONE))
        for what, parts in runs:
            o = Outs(B)
            _serve(lib, case, a, d, ids_d, x_d, B, parts, o)
            got = o.logits.cpu().numpy()
            err = max_err_scaled(got, ref[what][:B])
            print("%-16s B=%-2d %-6s err=%.3g" % (name, B, what, err))
            assert err < CONTRACT, (name, B, what, err)
            _check_head(lib, o)
            if what == "logits":
                kept[B] = o.logits.clone()
    # a request's bits do not depend on the batch around it: two workgroups and a tail against one full workgroup
    assert torch.equal(_bits(kept[65][:32]), _bits(kept[32]))
    assert torch.equal(_bits(kept[33][:32]), _bits(kept[32])) and torch.equal(_bits(kept[31]), _bits(kept[32][:31]))
    assert torch.equal(_bits(kept[1]), _bits(kept[32][:1]))


def test_each_output_alone_gives_the_bits_of_all_four(lib):
    case, a, d, ids, x, _ = _problem("walk_e12")
    B = 33
    ids_d, x_d = _inputs(case, ids, x, B)
    full = Outs(B)
    _serve(lib, case, a, d, ids_d, x_d, B, case.parts, full)
    for key in ("logits", "logistic", "probabilities", "class_ids"):
        o = Outs(B, only=key)
        assert sum(p is not None for p in o.pointers()) == 1
        _serve(lib, case, a, d, ids_d, x_d, B, case.parts, o)
        got, want = getattr(o, key), getattr(full, key)
        assert torch.equal(got, want) if key == "class_ids" else torch.equal(_bits(got), _bits(want)), key


# ---- the ensemble: three members that share the fields and differ most in LDS need ----------------------------------------
def _member(case, a, d):
    m = _lib.ServeMember()
    _lib.set_ptrs(m, table=d["table"], lin_w=d["lin_w"], dense=d["dense"], layer_off=d["layer_off"], widths=d["widths"])
    m.table_stride, m.lin_stride, m.E, m.n_layers, m.activation = a.ts, a.ls, case.E, a.n_layers, case.act
    m.use_linear, m.use_fm, m.use_dnn = case.parts
    m.numeric_raw = int(case.mode == "raw")
    m.lin_bias_off, m.num_emb_off, m.lin_num_off, m.wide_fields = a.lin_bias_off, a.num_emb_off, a.lin_num_off, case.wide
    return m


@functools.lru_cache(maxsize=None)
def _group(lib):
    """(member problems, device table, plan) of serve_cases.GROUP"""
    probs = [_problem(c.name) for c in SC.GROUP]
    M, F = len(probs), SC.GROUP[0].F
    assert all(p[0].F == F and p[0].nd == 0 and np.array_equal(p[1].field_off, probs[0][1].field_off) for p in probs)
    members = (_lib.ServeMember * M)(*[_member(p[0], p[1], p[2]) for p in probs])
    table = torch.full((max(int(lib.mi_predict_group_plan_bytes(M)), 16),), 0xA5, dtype=torch.uint8, device="cuda")
    plan = _lib.ServeGroupPlan()
    _chk(lib.mi_predict_group_plan(C.byref(members), M, F, 0, _p(probs[0][2]["field_off"]), _p(table), C.byref(plan), _st()),
         "mi_predict_group_plan")
    torch.cuda.synchronize()
    return probs, table, plan


def _run_group(lib, plan, M, ids_d, B, tickets):
    ml_whole, ml = guarded_nan(M, B)
    o = Outs(B)
    _chk(lib.mi_predict_group(C.byref(plan), M, _p(ids_d), None, B, _p(ml), _p(tickets), *o.pointers(), _st()), "mi_predict_group")
    torch.cuda.synchronize()
    o.check_written_inside_only()
    assert guards_intact(ml_whole) and not bool(torch.isnan(ml).any())
    assert not bool(tickets.any())                                   # zero again when the call has completed
    return ml, o


def test_group_plan_takes_the_largest_members_lds(lib):
    probs, _, plan = _group(lib)
    need = [SC.lds_bytes(p[0]) for p in probs]
    assert need == [768, 4 * 32 * (5 + 47 + 49), 4 * 32 * (5 + 512 + 512)]
    assert (plan.n_members, plan.F, plan.n_numeric, plan.lds_bytes) == (3, 5, 0, max(need))


def test_group_members_are_the_solo_bits_and_the_mean_is_fp32_in_member_order(lib):
    probs, _, plan = _group(lib)
    M = len(probs)
    ids = SC.group_requests()                                        # one request batch for all members
    tickets = torch.zeros((SC.B_MAX + 31) // 32, dtype=torch.int32, device="cuda")
    for B in (1, 33, 65):
        ids_d = dev(ids[:B])
        ml, o = _run_group(lib, plan, M, ids_d, B, tickets[:(B + 31) // 32])
        z = []
        for m, (case, a, d, _, _, _) in enumerate(probs):
            solo = Outs(B)
            _serve(lib, case, a, d, ids_d, None, B, case.parts, solo)
            assert torch.equal(_bits(ml[m]), _bits(solo.logits)), (B, m)
            ref = SC.reference(case, a, ids[:B], None)["logits"]     # (the member's own requests are not these)
            err = max_err_scaled(solo.logits.cpu().numpy(), ref)
            print("%-16s B=%-2d member %d err=%.3g" % (case.name, B, m, err))
            assert err < CONTRACT, (case.name, B, err)
            z.append(solo.logits.cpu().numpy())
        want = (((z[0] + z[1]).astype(np.float32) + z[2]).astype(np.float32) / np.float32(3)).astype(np.float32)
        assert np.array_equal(o.logits.cpu().numpy().view(np.int32), want.view(np.int32)), B
        _check_head(lib, o)
