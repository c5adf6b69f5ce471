"""CPU: numeric embedding columns in the one-launch step — the host side (engine.fused_train_step with x_num,
FusedPopulation, model.run_batch, the ABI) over the numpy stand-in of the numeric entries (tests/fused_numeric_kernels.py),
the stand-in itself against the fp64 oracle, and the library's own host checks (nothing is launched: no GPU needed).  The
kernel is tested in test_hip_fused_numeric.py over the same case table (tests/fused_numeric_cases.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec import feature_column as fc
from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.population import FusedPopulation
from tests import fused_numeric_cases as NC
from tests.cases import _sweep_args
from tests.cpu_kernels import NumpyKernels
from tests.fused_numeric_kernels import FusedNumericKernels, fused_numeric_kernels  # noqa: F401  (a fixture)
from tests.fused_rules_kernels import FusedRulesKernels
from tests.util import _t
from trainers import deep_fm, ml_100k

VOCAB = [9, 13, 5]


def _engine(vocab=VOCAB, nd=2, E=4, hidden=(8,), k=None, **kw):
    opt = kw.pop("optimizer", OptimizerSpec("Adam", 0.001))
    kw.setdefault("fused_numeric", True)
    return DeepFM(vocab, n_numeric=nd, embedding_size=E, hidden_units=list(hidden), optimizer=opt, device="cpu",
                  _kernels=k if k is not None else FusedNumericKernels(), **kw)


def _batch(seed, vocab, B, nd):
    rng = np.random.default_rng(seed)
    return _t(NC.draw_ids(rng, vocab, B)), _t(NC.draw_x(rng, B, nd)), _t((rng.random(B) < 0.3).astype(np.uint8))


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("mi_train_step_fused_workspace_bytes_numeric", "mi_train_step_model_numeric", "mi_train_group_plan_models_numeric",
               "mi_train_group_step_numeric", "mi_eval_group_numeric")


def test_the_numeric_entries_are_exported_and_the_version_stays(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and (" T %s\n" % name) in out, name
    assert lib.mi_abi_version() == 21 == _lib.ABI_VERSION
    # the workspace: the dense gradient and d_concat [B, (F + nd) E]; without numeric columns the existing entry's
    assert lib.mi_train_step_fused_workspace_bytes_numeric(32, 26, 13, 4, 1001) == 4 * (1004 + 32 * 39 * 4)
    assert lib.mi_train_step_fused_workspace_bytes_numeric(16, 3, 0, 4, 77) == lib.mi_train_step_fused_workspace_bytes(16, 3, 4, 77)
    assert FusedNumericKernels().query("mi_train_step_fused_workspace_bytes_numeric", 32, 26, 13, 4, 1001) == 4 * (1004 + 32 * 39 * 4)


def test_the_numeric_struct_is_laid_out_as_the_c_compiler_lays_it_out(tmp_path):
    """host only: the header through the system's C compiler; the ctypes mirror must agree on the size and on every offset"""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mi355x_rec.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mi_fused_numeric_t), offsetof(mi_fused_numeric_t, n_numeric), '
                   'offsetof(mi_fused_numeric_t, num_emb_off), offsetof(mi_fused_numeric_t, lin_num_off)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", header, str(src), "-o", str(exe)], check=True)
    got = tuple(int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    N = _lib.FusedNumeric
    assert got == (ctypes.sizeof(N), N.n_numeric.offset, N.num_emb_off.offset, N.lin_num_off.offset)
    assert [n for n, _ in N._fields_] == ["n_numeric", "num_emb_off", "lin_num_off"]


# ---- the engine's limits ----------------------------------------------------------------------------------------------------
def test_a_model_with_numeric_embeddings_is_inside_the_scope():
    m = _engine()
    assert m.fused_step_ok(32) and m._fused_step_limit(32) is None
    assert not m.fused_step_auto(32)                               # (no table says the fused step wins there)
    n = m.fused_numeric()
    assert (n.n_numeric, n.num_emb_off, n.lin_num_off) == (2, m.num_emb_off, m.lin_num_off)
    assert _engine(nd=0).fused_numeric() is None and _engine(nd=0).fused_step_ok(32)
    assert _engine([3] * 26, 13, 4, [64, 64, 64]).fused_step_ok(32)          # 26 + 13 columns fit at E = 4, B = 32
    assert _engine([3] * 26, 6, 4, [8]).fused_step_ok(128)                   # B (F + nd) E = 16384
    # an engine built as before this feature keeps its answer: numeric embeddings are asked for at construction
    assert _engine(fused_numeric=False)._fused_step_limit(16) == "2 numeric columns (fused_numeric=True admits numeric embeddings)"
    with pytest.raises(ValueError, match="member 0: the model has 2 numeric columns"):
        FusedPopulation([_engine(fused_numeric=False)])
    # the stand-ins without the numeric entries keep the earlier answer
    for k in (NumpyKernels(), FusedRulesKernels()):
        assert _engine(k=k)._fused_step_limit(16) == "2 numeric columns (categorical columns only)"


@pytest.mark.parametrize("kw,B,text", [
    (dict(nd=17, vocab=[3]), 8, "17 numeric columns (at most 16)"),
    (dict(nd=7, vocab=[3] * 26), 128, "B * (F + n_numeric) * E = 16896 (at most 16384)"),
    (dict(nd=2, numeric="raw", use_mf=False), 8, "2 raw numeric columns"),
    (dict(nd=2, vocab=[]), 8, "no categorical column"),
    (dict(nd=2, vocab=[3] * 33), 8, "33 categorical fields"),
])
def test_the_new_limits_are_refused_with_their_text(kw, B, text):
    kw = dict(kw)
    m = _engine(kw.pop("vocab", VOCAB), kw.pop("nd"), **kw)
    assert not m.fused_step_ok(B)
    ids = torch.zeros(B, m.F, dtype=torch.int32)
    with pytest.raises(ValueError, match=re.escape("fused_train_step: the model has " + text)):
        m.fused_train_step(ids, torch.zeros(B, dtype=torch.uint8), torch.zeros(B, m.n_numeric))
    assert not m.k.calls and m.step == 0
    with pytest.raises(ValueError, match=re.escape(text)):
        FusedPopulation([m]).train_step(ids, torch.zeros(B, dtype=torch.uint8), x_num=torch.zeros(B, m.n_numeric))


def test_numeric_embeddings_need_the_embedding_path():
    with pytest.raises(NotImplementedError, match="numeric embeddings need the embedding path"):
        _engine(use_mf=False, use_dnn=False)                       # (use_fm || use_dnn with nd > 0: the engine never builds it)


def test_x_num_is_validated_as_predict_validates_it():
    m = _engine()
    ids, x, y = _batch(3, VOCAB, 8, 2)
    for bad in (None, x[:, :1].contiguous(), x.double(), x[:4]):
        with pytest.raises(ValueError, match=r"x_num must be float32 \[B, 2\]"):
            m.fused_train_step(ids, y, bad)
    with pytest.raises(ValueError, match="x_num must be contiguous"):
        m.fused_train_step(ids, y, torch.zeros(2, 8).t())
    with pytest.raises(ValueError, match="model has no numeric columns"):
        _engine(nd=0).fused_train_step(ids, y, x)
    assert not m.k.calls and m.step == 0
    m.fused_train_step(ids, y, x)
    assert m.k.calls == {"mi_train_step_model_numeric": 1} and m.step == 1


# ---- the stand-in against the oracle: the case table states the same thing on both sides --------------------------------------
@pytest.mark.parametrize("case", NC.CASES, ids=NC.CASE_IDS)
def test_the_stand_in_follows_the_oracle(case):
    NC.run_trajectory(case, "cpu", FusedNumericKernels())


@pytest.mark.parametrize("case", NC.GRAD_CASES, ids=NC.GRAD_IDS)
def test_the_stand_ins_numeric_gradients_against_fp64(case):
    NC.check_gradient_window(case, "cpu", FusedNumericKernels())


@pytest.mark.parametrize("name", sorted(NC.RULES))
def test_the_stand_in_under_the_other_rules(name):
    m, _ = NC.run_rule(name, "cpu", FusedNumericKernels())
    if m.lin_opt is not None:                                      # lin_num keeps the WIDE rule's slots, numeric_embeddings the deep rule's
        sl = slice(m.lin_num_off, m.lin_num_off + m.n_numeric)
        assert bool((m.dl_s0[sl] != 0.1).all()) and bool((m.d_s0[sl] == 0.1).all())
        se = slice(m.num_emb_off, m.num_emb_off + m.n_numeric * m.E)
        assert bool((m.d_s0[se] != 0.1).any()) and bool((m.dl_s0[se] == 0.1).all())


# ---- the population -----------------------------------------------------------------------------------------------------------
def _members(M, k, **kw):
    out = []
    for i in range(M):
        m = _engine(k=k, seed=i, **kw)
        g = torch.Generator()
        g.manual_seed(50 + i)
        m.init_variables(g, lin_scale=0.05)
        out.append(m)
    return out


@pytest.mark.parametrize("per_member", [False, True])
def test_a_population_steps_and_evaluates_with_x_num(per_member):
    M, B, N = 3, 8, 20
    k = FusedNumericKernels()
    pop_e, solo_e = _members(M, k), _members(M, k)
    pop = FusedPopulation(pop_e)
    assert pop.nd == 2
    rng = np.random.default_rng(5)
    for s in range(2):
        if per_member:
            ids = _t(np.stack([NC.draw_ids(rng, VOCAB, B) for _ in range(M)]))
            x = _t(np.stack([NC.draw_x(rng, B, 2) for _ in range(M)]))
        else:
            ids, x = _t(NC.draw_ids(rng, VOCAB, B)), _t(NC.draw_x(rng, B, 2))
        y = _t((rng.random(B) < 0.3).astype(np.uint8))
        loss, logits = pop.train_step(ids, y, x_num=x)
        for i, e in enumerate(solo_e):
            l1, z1 = e.fused_train_step(ids[i] if per_member else ids, y, x[i] if per_member else x)
            assert torch.equal(z1, logits[i]) and l1.item() == loss[i].item()
            assert torch.equal(e.dense, pop_e[i].dense) and torch.equal(e.t_rec, pop_e[i].t_rec)
    assert k.calls["mi_train_group_step_numeric"] == 2 and "mi_train_group_step" not in k.calls
    # (values of order 1: the layered stand-in sums the FM term in another order, and this is a check of the plumbing)
    ids, x = _t(NC.draw_ids(rng, VOCAB, N)), _t(rng.standard_normal((N, 2)).astype(np.float32))
    y = _t((rng.random(N) < 0.3).astype(np.uint8))
    before = [e.dense.clone() for e in pop_e]
    metrics, z = pop.evaluate(ids, y, batch_size=B, return_logits=True, x_num=x)
    assert len(metrics) == M and all(np.isfinite(m["loss"]) and 0.0 <= m["auc"] <= 1.0 for m in metrics)
    for i, e in enumerate(pop_e):
        assert torch.equal(e.dense, before[i])
        assert np.allclose(z[i].numpy(), e.predict_logits(ids, x).numpy(), rtol=1e-5, atol=2e-6)
    assert k.calls["mi_eval_group_numeric"] == 1
    # x_num is checked before anything runs
    for bad in (None, x[:, :1].contiguous(), x.double()):
        with pytest.raises(ValueError, match="x_num must be a contiguous float32"):
            pop.evaluate(ids, y, batch_size=B, x_num=bad)
    with pytest.raises(ValueError, match="x_num must be a contiguous float32"):
        pop.train_step(ids[:B].contiguous(), y[:B].contiguous(), x_num=None)
    with pytest.raises(ValueError, match="no numeric columns"):
        FusedPopulation(_members(2, k, nd=0)).train_step(ids[:B].contiguous(), y[:B].contiguous(), x_num=x[:B].contiguous())


def test_members_share_their_numeric_columns():
    k = FusedNumericKernels()
    with pytest.raises(ValueError, match="member 1 has 1 numeric columns, member 0 has 2"):
        FusedPopulation([_engine(k=k), _engine(k=k, nd=1)])


def test_the_entries_without_x_num_refuse_a_numeric_plan():
    k = FusedNumericKernels()
    pop = FusedPopulation(_members(2, k))
    ids, x, y = _batch(9, VOCAB, 8, 2)
    pop.train_step(ids, y, x_num=x)
    plan = pop._plans[8][1]
    logits, loss = torch.full((2, 8), float("nan")), torch.full((2,), float("nan"))
    with pytest.raises(_lib.MiError, match="numeric columns and this entry brings no x_num"):
        k.mi_train_group_step(plan, 2, ids, 0, y, 0, 8, 2, logits, loss, 0)
    with pytest.raises(_lib.MiError, match="numeric columns and this entry brings no x_num"):
        k.mi_eval_group(plan, 2, ids, y, 8, None, None, torch.zeros(2, 1), torch.zeros(2, 2, 201, dtype=torch.int64),
                        torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 1, 3, dtype=torch.float64), 0)
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())


# ---- the library's own host checks: refused before anything is launched, so they run here --------------------------------------
def _raw(lib, m, B, nd, x, ws_bytes=None, F=None):
    """mi_train_step_model_numeric through ctypes on host memory with n_numeric = nd; returns (status, text, logits, loss)"""
    ws = torch.empty(ws_bytes if ws_bytes is not None else 1 << 20, dtype=torch.uint8)
    model, held = m.fused_model(B, ws, 0.001, 0.0)
    num = m.fused_numeric()
    num.n_numeric = nd
    F = m.F if F is None else F
    ids, y = torch.zeros(B, F, dtype=torch.int32), torch.zeros(B, dtype=torch.uint8)
    logits, loss = torch.full((B,), float("nan")), torch.full((1,), float("nan"))
    rc = lib.mi_train_step_model_numeric(ctypes.byref(model), ctypes.byref(num), m.field_off.data_ptr(), ids.data_ptr(),
                                         None if x is None else x.data_ptr(), y.data_ptr(), B, F, 1, 1, logits.data_ptr(),
                                         loss.data_ptr(), 0, None)
    return rc, lib.mi_last_error().decode(), logits, loss


def test_the_library_refuses_on_the_host(lib):
    m = _engine([3] * 26, 6, 4, [8], k=NumpyKernels())
    x = torch.zeros(128, 16)
    cases = [
        (dict(B=8, nd=17), -2, "17 numeric columns (0 to 16)"),
        (dict(B=128, nd=7), -2, "B (F + n_numeric) E = 16896 (at most 16384)"),
        (dict(B=8, nd=6, x=None), -1, "x_num (the model has 6 numeric columns)"),
        (dict(B=8, nd=5), -1, "widths[0]=128, the 124 input columns expected"),
        (dict(B=8, nd=6, ws_bytes=64), -4, "workspace of 64 bytes"),
    ]
    for kw, status, text in cases:
        rc, msg, logits, loss = _raw(lib, m, kw["B"], kw["nd"], kw.get("x", x), kw.get("ws_bytes"))
        assert rc == status and msg.startswith("train_step_fused: ") and text in msg, (kw, rc, msg)
        assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())
    # numeric embeddings without the FM term and the DNN, and offsets outside dense: a description the engine never builds
    ws = torch.empty(1 << 16, dtype=torch.uint8)
    ids, y = torch.zeros(8, 26, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8)
    logits, loss = torch.full((8,), float("nan")), torch.full((1,), float("nan"))
    for at, nat, text in ((dict(use_fm=0, use_dnn=0, n_layers=0), {}, "without the FM term and the DNN"),
                          ({}, dict(num_emb_off=m.P - 4), "num_emb_off="), ({}, dict(lin_num_off=m.P), "lin_num_off=")):
        model, held = m.fused_model(8, ws, 0.001, 0.0)
        num = m.fused_numeric()
        for k, v in at.items():
            setattr(model, k, v)
        for k, v in nat.items():
            setattr(num, k, v)
        rc = lib.mi_train_step_model_numeric(ctypes.byref(model), ctypes.byref(num), m.field_off.data_ptr(), ids.data_ptr(),
                                             x.data_ptr(), y.data_ptr(), 8, 26, 1, 1, logits.data_ptr(), loss.data_ptr(), 0, None)
        assert rc == -1 and text in lib.mi_last_error().decode(), (text, rc, lib.mi_last_error().decode())
        # ... and as member 0 of a plan, with nothing written
        table = torch.full((int(lib.mi_train_group_plan_bytes(1)),), 0xA5, dtype=torch.uint8)
        plan = _lib.FusedGroupPlan()
        model.lr_table, model.lr_table_len = m.sched.table.data_ptr(), m.sched.table.numel()
        rc = lib.mi_train_group_plan_models_numeric(ctypes.byref(model), ctypes.byref(num), 1, 8, 26, m.field_off.data_ptr(),
                                                    table.data_ptr(), table.numel(), ctypes.byref(plan), None)
        msg = lib.mi_last_error().decode()
        assert rc == -1 and msg.startswith("train_group_plan: member 0: train_step_fused: ") and text in msg, msg
        assert plan.magic == 0 and plan.device_table is None and bool((table == 0xA5).all())
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())
    # a damaged or foreign plan is no plan for the numeric entries either
    plan = _lib.FusedGroupPlan()
    rc = lib.mi_train_group_step_numeric(ctypes.byref(plan), 1, ids.data_ptr(), 0, x.data_ptr(), 0, y.data_ptr(), 0, 8, 1,
                                         logits.data_ptr(), loss.data_ptr(), 0, None)
    assert rc == -1 and "not written by mi_train_group_plan" in lib.mi_last_error().decode()


# ---- model_fn -----------------------------------------------------------------------------------------------------------------
def test_model_fn_trains_numeric_columns_with_the_fused_step(fused_numeric_kernels):
    cols = ml_100k.get_feature_columns(4)["linear"]
    numeric = [fc.numeric_column("age"), fc.numeric_column("release_year")]
    feats, labels = next(ml_100k.get_input_fn("synthetic:200:1", batch_size=32, seed=0)())
    params = {"categorical_columns": cols, "numeric_columns": numeric, "device": "cpu", "fused_step": "on"}
    deep_fm.model_fn(feats, labels, "_build", params)
    eng = params["_store"]["engine"]
    assert eng.n_numeric == 2 and eng.fused_step_ok(32)
    v0 = eng.dense[eng.num_emb_off:eng.num_emb_off + 2 * eng.E].clone()
    for _ in range(3):
        spec = deep_fm.model_fn(feats, labels, "train", params)
    assert spec.train_op == 3 and eng.k.calls.get("mi_train_step_model_numeric") == 3 and np.isfinite(float(spec.loss))
    assert "mi_numeric_embed_fwd" not in eng.k.calls and "mi_train_step_fused" not in eng.k.calls
    assert not torch.equal(v0, eng.dense[eng.num_emb_off:eng.num_emb_off + 2 * eng.E])
    # "auto" stays with today's path for such a model
    params = {"categorical_columns": cols, "numeric_columns": numeric, "device": "cpu", "fused_step": "auto", "hip_graph": "off"}
    deep_fm.model_fn(feats, labels, "_build", params)
    deep_fm.model_fn(feats, labels, "train", params)
    assert "mi_train_step_model_numeric" not in params["_store"]["engine"].k.calls


def test_a_sweep_feeds_the_numeric_columns_of_its_feature_column_set(fused_numeric_kernels, tmp_path, monkeypatch):
    """trainers.sweep over a feature-column set with two numeric columns: every population step and every population
    evaluation goes through the numeric entries (the ML-100k CLI set itself has none)"""
    import json

    from trainers import sweep
    real = sweep.get_feature_columns

    def with_numeric(embedding_size=4):
        cols = dict(real(embedding_size=embedding_size))
        cols["numeric"] = [fc.numeric_column("age"), fc.numeric_column("release_year")]
        return cols
    monkeypatch.setattr(sweep, "get_feature_columns", with_numeric)
    job = tmp_path / "job"
    members = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "6", "--learning-rate", "0.001", "0.01", "--eval-every", "3",
                                                   "--final-eval", "fused"))
    assert len(members) == 2 and all(est.global_step == 6 for est in members)
    calls = members[0]._engine().k.calls
    assert members[0]._engine().n_numeric == 2
    assert calls.get("mi_train_group_step_numeric") == 6 and calls.get("mi_eval_group_numeric", 0) >= 2
    assert "mi_train_group_step" not in calls and "mi_eval_group" not in calls
    rows = json.load(open(job / "sweep.json"))["members"]
    assert len(rows) == 2 and all(np.isfinite(r["metrics"]["loss"]) for r in rows)
