"""CPU: a solo fused entry and its group plan refuse alike.  mi_train_step_fused / mi_train_group_plan and mi_predict_fused /
mi_predict_group_plan (include/mi355x_rec.h) check a model with one host function each; a description the checks refuse is
handed to the real library twice — to the solo entry as positional arguments and to the group plan as member 1 of 3 — and
must give the same status and the same text behind "<plan entry>: member 1: " (B and F are one value for all members of a
plan, so a bad one is met at member 0 first: "member 0: ").  Every case is a refusal: the library
decides on the host and launches nothing, so no GPU is needed (the kernels: test_hip_fused_step.py, test_hip_population.py,
test_hip_serve.py, test_hip_ensemble.py)."""
import ctypes as C

import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import OptimizerSpec
from mi355x_rec.population import FusedPopulation
from mi355x_rec.predictor import _serve_member
from tests.cases import _numpy_engine
from tests.cpu_kernels import library_sized

VOCAB = [9, 13, 5]
F = len(VOCAB)


def _engines(lib, **kw):
    k = library_sized(lib)
    return [_numpy_engine(VOCAB, 4, [8], k, **kw), _numpy_engine(VOCAB, 4, [8], k, **kw), _numpy_engine(VOCAB, 4, [8], k, **kw)]


def _widths(m):
    """the host table member m's widths points to: n_layers + 1 int32"""
    return torch.tensor(list((C.c_int32 * (m.n_layers + 1)).from_address(m.widths)), dtype=torch.int32)


def _with(w, keep, **at):
    """a copy of the widths table w with entries replaced (index -> value), kept alive: its address"""
    w = w.clone()
    for i, v in at.items():
        w[int(i)] = v
    keep.append(w)
    return w.data_ptr()


# case -> (what is corrupted: (member 1, its valid widths table, keep-alive list) -> another B for the call or None,
#          the expected status, a piece of the expected text)
TRAIN_CASES = {
    "B = 129": (lambda m, w, keep: 129, -2, "B=129 (1 to 128 examples)"),
    "E = 20": (lambda m, w, keep: setattr(m, "E", 20), -2, "embedding size 20"),
    "n_layers = 5": (lambda m, w, keep: setattr(m, "n_layers", 5), -2, "4 hidden layers (at most 3)"),
    "keep_prob = 0": (lambda m, w, keep: setattr(m, "keep_prob", 0.0), -1, "keep_prob=0"),
    "optimizer kind 1": (lambda m, w, keep: setattr(m, "hp", OptimizerSpec("Adagrad", 0.05).hparams()), -2,
                         "optimizer kind 1 (Adam only)"),
    "workspace_bytes = 8": (lambda m, w, keep: setattr(m, "workspace_bytes", 8), -4, "workspace of 8 bytes"),
    "activation = 4": (lambda m, w, keep: setattr(m, "activation", 4), -1, "activation 4"),
    "R = 0": (lambda m, w, keep: setattr(m, "R", 0), -2, "R=0 table rows"),
    "table_stride = E + 1": (lambda m, w, keep: setattr(m, "table_stride", m.E + 1), -1, "table_stride=5"),
    "last width 2": (lambda m, w, keep: setattr(m, "widths", _with(w, keep, **{"-1": 2})), -1, "the last layer has 2 outputs"),
    "lin_bias_off = n_dense": (lambda m, w, keep: setattr(m, "lin_bias_off", m.n_dense), -1, "lin_bias_off"),
    "table + 4 bytes": (lambda m, w, keep: setattr(m, "table", m.table + 4), -1, "table / t_m / t_v (16-byte aligned)"),
}


@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_the_fused_step_and_the_population_plan_refuse_alike(lib, case):
    corrupt, status, text = TRAIN_CASES[case]
    es = _engines(lib)
    pop, keep, B = FusedPopulation(es), [], 16
    ms = (_lib.FusedMember * 3)(*[pop._describe(e, B, keep) for e in es])
    m = ms[1]
    shared = corrupt(m, _widths(m), keep)            # (B = 129: an argument of the call, the same for every member)
    B, first = (shared, 0) if shared else (B, 1)
    field_off = es[0].field_off.data_ptr()

    # solo: the description as mi_train_step_fused's positional arguments, step = 1, a batch and outputs in hand
    ids, y = torch.zeros(129, F, dtype=torch.int32), torch.zeros(129, dtype=torch.uint8)
    logits, loss = torch.full((129,), float("nan")), torch.full((1,), float("nan"))
    hp = _lib.OptHparams.from_buffer_copy(m.hp)
    rc_solo = lib.mi_train_step_fused(m.table, m.t_m, m.t_v, m.table_stride, m.lin_w, m.l_m, m.l_v, m.lin_stride, m.last_step,
                                      field_off, m.R, ids.data_ptr(), y.data_ptr(), B, F, m.E, m.dense, m.d_m, m.d_v, m.n_dense,
                                      m.layer_off, m.widths, m.n_layers, m.activation, m.use_linear, m.use_fm, m.use_dnn,
                                      m.lin_bias_off, m.keep_prob, (m.seed_base + 1000003) & (2 ** 64 - 1), m.scale, 1, C.byref(hp),
                                      logits.data_ptr(), loss.data_ptr(), 0, m.workspace, m.workspace_bytes, None)
    solo = lib.mi_last_error().decode()
    assert rc_solo == status and solo.startswith("train_step_fused: ") and text in solo, (rc_solo, solo)
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())

    # group: the same description as member 1 of 3 (the refusal names the first member it is met at)
    table = torch.full((int(lib.mi_train_group_plan_bytes(3)),), 0xA5, dtype=torch.uint8)
    plan = _lib.FusedGroupPlan()
    rc_group = lib.mi_train_group_plan(ms, 3, B, F, field_off, table.data_ptr(), table.numel(), C.byref(plan), None)
    group = lib.mi_last_error().decode()
    print("%s: solo %d %r, group %d %r" % (case, rc_solo, solo, rc_group, group))
    assert rc_group == rc_solo
    assert group == "train_group_plan: member %d: " % first + solo
    assert plan.magic == 0 and plan.device_table is None and bool((table == 0xA5).all())       # nothing was written


SERVE_CASES = {
    "F = 65": (lambda m, w, keep: 65, -2, "F=65 categorical fields (at most 64)"),
    "E = 6": (lambda m, w, keep: setattr(m, "E", 6), -2, "embedding size 6 unsupported"),
    "activation = 7": (lambda m, w, keep: setattr(m, "activation", 7), -1, "activation 7"),
    "numeric_raw with use_fm": (lambda m, w, keep: setattr(m, "numeric_raw", 1), -1,
                                "raw numeric columns belong to the models without an FM term"),
    "n_layers = 10": (lambda m, w, keep: setattr(m, "n_layers", 10), -2, "9 hidden layers (at most 8)"),
    "hidden width 513": (lambda m, w, keep: setattr(m, "widths", _with(w, keep, **{"1": 513})), -2,
                         "hidden width 513 (at most 512)"),
    "last width 2": (lambda m, w, keep: setattr(m, "widths", _with(w, keep, **{"-1": 2})), -1, "the last layer has 2 outputs"),
    "widths[0] below the input": (lambda m, w, keep: setattr(m, "widths", _with(w, keep, **{"0": int(w[0]) - 1})), -1,
                                  "widths[0]=15 below the 16 input columns"),
    "num_emb_off = 2": (lambda m, w, keep: setattr(m, "num_emb_off", 2), -1, "num_emb_off=2"),
    "table + 4 bytes": (lambda m, w, keep: setattr(m, "table", m.table + 4), -1, "table (16-byte aligned)"),
    "table_stride = E + 2": (lambda m, w, keep: setattr(m, "table_stride", m.E + 2), -1, "table_stride=6"),
}


@pytest.mark.parametrize("case", sorted(SERVE_CASES))
def test_the_fused_forward_and_the_ensemble_plan_refuse_alike(lib, case):
    corrupt, status, text = SERVE_CASES[case]
    es = _engines(lib, n_numeric=1)                  # (one numeric column, embedded: 3 x 4 + 4 = 16 input columns)
    keep, B, n_numeric = [], 4, 1
    ms = (_lib.ServeMember * 3)(*[_serve_member(e, keep) for e in es])
    m = ms[1]
    shared = corrupt(m, _widths(m), keep)            # (F = 65: an argument of the call, the same for every member)
    Fc, first = (shared, 0) if shared else (F, 1)
    field_off = es[0].field_off.data_ptr()

    # solo: the description as mi_predict_fused's positional arguments, B = 4, ids, x_num and every output in hand
    ids, x = torch.zeros(B, 65, dtype=torch.int32), torch.zeros(B, n_numeric)
    outs = [torch.full((B,), float("nan")), torch.full((B,), float("nan")), torch.full((B, 2), float("nan")),
            torch.full((B,), -7, dtype=torch.int64)]
    rc_solo = lib.mi_predict_fused(m.table, m.table_stride, m.lin_w, m.lin_stride, field_off, ids.data_ptr(), x.data_ptr(), B, Fc,
                                   m.E, n_numeric, m.dense, m.layer_off, m.widths, m.n_layers, m.activation, m.use_linear,
                                   m.use_fm, m.use_dnn, m.numeric_raw, m.lin_bias_off, m.num_emb_off, m.lin_num_off,
                                   m.wide_fields, *[o.data_ptr() for o in outs], None, 0, None)
    solo = lib.mi_last_error().decode()
    assert rc_solo == status and solo.startswith("predict_fused: ") and text in solo, (rc_solo, solo)
    assert all(bool(torch.isnan(o).all()) for o in outs[:3]) and bool((outs[3] == -7).all())

    # group: the same description as member 1 of 3 (the refusal names the first member it is met at)
    table = torch.full((int(lib.mi_predict_group_plan_bytes(3)),), 0xA5, dtype=torch.uint8)
    plan = _lib.ServeGroupPlan()
    rc_group = lib.mi_predict_group_plan(ms, 3, Fc, n_numeric, field_off, table.data_ptr(), C.byref(plan), None)
    group = lib.mi_last_error().decode()
    print("%s: solo %d %r, group %d %r" % (case, rc_solo, solo, rc_group, group))
    assert rc_group == rc_solo
    assert group == "predict_group_plan: member %d: " % first + solo
    assert plan.magic == 0 and plan.device_table is None and bool((table == 0xA5).all())       # nothing was written
