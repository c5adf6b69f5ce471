"""CPU: the host side of the one-launch train step under every optimizer, two rules and the canned estimators' columns, on
the numpy stand-in tests/fused_rules_kernels.FusedRulesKernels — trajectories against the oracle (the cases and bars of
tests/fused_rules_cases.py, the ones test_hip_fused_rules.py runs on the device), the capability seam, the canned CLIs,
trainers.sweep --optimizer, and what the real library refuses on the host through its two new entries."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.population import FusedPopulation
from tests import fused_rules_cases as FC
from tests.cases import _sweep_args
from tests.cpu_kernels import NumpyKernels
from tests.fused_rules_kernels import FusedRulesKernels, fused_rules_kernels  # noqa: F401  (fused_rules_kernels: a fixture)

LAYERED_GEMMS = ("mi_dense_fwd", "mi_dense_fwd_gathered", "mi_dense_bwd_data", "mi_dense_bwd_weight", "mi_dense_bwd_weight_gathered",
                 "mi_sparse_apply", "mi_sparse_apply_fused", "mi_dense_apply", "mi_embed_fm_linear_fwd")


# ---- trajectories ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.TRAJECTORY_NAMES)
def test_trajectory_against_the_oracle(name):
    k = FusedRulesKernels()
    FC.run_trajectory(name, name, "cpu", k)
    assert k.calls["mi_train_step_model"] == 3 and not any(n in k.calls for n in LAYERED_GEMMS + ("mi_train_step_fused",))


def test_a_model_of_the_old_entrys_scope_keeps_calling_it():
    k = FusedRulesKernels()
    m = FC.make_engine(dict(flags=(True, True, True), hp=("Adam", 0.001)), "cpu", k)
    ids, y = FC.draw_batch(np.random.default_rng(1), FC.VOCAB, 16)
    m.fused_train_step(torch.from_numpy(ids), torch.from_numpy(y))
    assert k.calls.get("mi_train_step_fused") == 1 and "mi_train_step_model" not in k.calls
    assert m.fused_step_auto(16)
    for name in FC.TRAJECTORY_NAMES:                            # nothing measured admits the new models yet
        n = FC.make_engine(name, "cpu", FusedRulesKernels())
        assert n.fused_step_ok(16) and not n.fused_step_auto(16), name


# ---- the seam ------------------------------------------------------------------------------------------------------------------
def test_the_capability_flag_is_the_seam():
    from mi355x_rec import engine
    assert engine.HipKernels.supports_fused_rules is True and not hasattr(NumpyKernels, "supports_fused_rules")
    texts = {"linear_classifier_ftrl_sum": "optimizer Ftrl (Adam for every variable, one schedule)",
             "dnn_classifier_adagrad_sum_dropout": "optimizer Adagrad (Adam for every variable, one schedule)",
             "wide_deep_two_optimizers": "optimizer Adagrad with linear_optimizer Ftrl (Adam for every variable, one schedule)",
             "two_different_adam_optimizers": "optimizer Adam with linear_optimizer Adam (Adam for every variable, one schedule)",
             "deepfm_sgd": "optimizer SGD (Adam for every variable, one schedule)"}
    for name in FC.TRAJECTORY_NAMES:
        old, new = FC.make_engine(name, "cpu", NumpyKernels()), FC.make_engine(name, "cpu", FusedRulesKernels())
        assert not old.fused_step_ok(16) and new.fused_step_ok(16), name
        if name in texts:
            assert old._fused_step_limit(16) == texts[name]
            with pytest.raises(ValueError, match="fused_train_step: the model has optimizer"):
                old.fused_train_step(torch.zeros(16, 4, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8))
        with pytest.raises(ValueError, match="member 0: the model has optimizer"):
            FusedPopulation([old])
        FusedPopulation([new])
    subsets = dict(embedding_size=8, hidden_units=[8], use_mf=False, numeric="raw", field_dims=FC.DIMS, wide_fields=FC.WIDE, device="cpu")
    assert DeepFM(FC.VOCAB, _kernels=NumpyKernels(), **subsets)._fused_step_limit(16) == \
        "field_dims / wide_fields (the canned estimators' columns)"
    assert DeepFM(FC.VOCAB, _kernels=FusedRulesKernels(), **subsets).fused_step_ok(16)
    for k in (NumpyKernels(), FusedRulesKernels()):             # numeric columns, sharding and the sizes: refused everywhere
        n = DeepFM(FC.VOCAB, n_numeric=2, embedding_size=8, hidden_units=[8], optimizer=OptimizerSpec("Adagrad", 0.05)
                   if isinstance(k, FusedRulesKernels) else None, device="cpu", _kernels=k)
        assert n._fused_step_limit(16) == "2 numeric columns (categorical columns only)"
        big = DeepFM(FC.VOCAB, embedding_size=8, hidden_units=[128], device="cpu", _kernels=k)
        assert big._fused_step_limit(16) == "a hidden layer of 128 units (at most 64)"
        assert big._fused_step_limit(129) is not None


# ---- the canned CLIs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opt,extra", [("linear", (), []), ("deep", ("hidden_units", "dropout"), ["--hidden-units", "8"]),
                                            ("linear_deep", ("hidden_units", "dropout"), ["--hidden-units", "8"])])
def test_a_canned_cli_trains_with_one_launch_per_step(fused_rules_kernels, tmp_path, name, opt, extra):
    import importlib
    from trainers import _cli
    trainer = importlib.import_module("trainers." + name)
    job = str(tmp_path / name)
    argv = ["--synthetic", "200", "--job-dir", job, "--train-steps", "5", "--batch-size", "16", "--device", "cpu"] + extra
    est = trainer.train_and_evaluate(_cli.make_parser(name, opt).parse_args(argv + ["--fused-step", "on"]))
    k = est._engine().k
    assert est.global_step == 5 and k.calls["mi_train_step_model"] == 5 and "mi_train_step_fused" not in k.calls
    # (the evaluation at the end runs the layered FORWARD; no training entry of the layered step was called: no backward
    # GEMM, no apply)
    assert not any(n in k.calls for n in ("mi_dense_bwd_data", "mi_dense_bwd_weight", "mi_dense_bwd_weight_gathered",
                                          "mi_sparse_apply", "mi_sparse_apply_fused", "mi_dense_apply"))
    assert os.path.exists(os.path.join(job, "model.ckpt-5.pt"))
    # the checkpoint restores into a layered engine (no flag), which carries on
    est2 = trainer.train_and_evaluate(_cli.make_parser(name, opt).parse_args(argv + ["--restore", "--train-steps", "8"]))
    k2 = est2._engine().k
    assert est2.global_step == 8 and "mi_train_step_model" not in k2.calls
    assert k2.calls.get("mi_sparse_apply_fused", 0) + k2.calls.get("mi_sparse_apply", 0) >= 3
    assert "ONE kernel launch" in _cli.make_parser(name, opt).format_help() and "canned" in _cli.make_parser(name, opt).format_help()


# ---- trainers.sweep --optimizer -----------------------------------------------------------------------------------------------
def test_sweep_optimizer_grid():
    from trainers import sweep
    a = _sweep_args("job")
    assert a.optimizer is None
    assert sweep.grid(a) == [dict(embedding_size=4, hidden_units=[8, 8], dropout=0.1, learning_rate=0.001, seed=0)]
    a = _sweep_args("job", "--optimizer", "Adam", "Adagrad", "--seeds", "2")
    g = sweep.grid(a)
    assert [(h["optimizer"], h["seed"]) for h in g] == [("Adam", 0), ("Adam", 1), ("Adagrad", 0), ("Adagrad", 1)]
    assert all(set(h) == {"embedding_size", "hidden_units", "dropout", "learning_rate", "optimizer", "seed"} for h in g)
    with pytest.raises(SystemExit):
        _sweep_args("job", "--optimizer", "Momentum")
    assert "--optimizer" in sweep.make_parser().format_help() and "optimizer" in sweep.__doc__


def test_sweep_members_under_different_optimizers_are_stand_alone_runs(fused_rules_kernels, tmp_path):
    from mi355x_rec.estimator import Estimator
    from trainers import deep_fm, ml_100k, sweep
    job = tmp_path / "job"
    members = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "6", "--optimizer", "Adam", "Adagrad", "--seeds", "2"))
    assert len(members) == 4 and all(m.global_step == 6 for m in members)
    assert [m._engine().opt.name for m in members] == ["Adam", "Adam", "Adagrad", "Adagrad"]
    k = members[0]._engine().k
    assert sum(m._engine().k.calls.get("mi_train_group_step", 0) for m in members) == 6
    assert any(m._engine().k.calls.get("mi_train_group_plan_models", 0) for m in members)
    rows = json.load(open(job / "sweep.json"))["members"]
    assert sorted((r["params"]["optimizer"], r["params"]["seed"]) for r in rows) == [("Adagrad", 0), ("Adagrad", 1), ("Adam", 0),
                                                                                     ("Adam", 1)]
    # every member: bit for bit a solo fused_train_step run with its hyper-parameters on the same batches
    from trainers import _cli
    config = _cli.get_run_config()
    config.device = "cpu"
    args = _sweep_args(tmp_path / "job2", "--optimizer", "Adam", "Adagrad", "--seeds", "2")
    hps = sweep.grid(args)
    side = sweep.make_members(args, hps, config)
    sweep.train(side, ml_100k.get_input_fn("synthetic:600:1", batch_size=16, seed=7), 6, config)
    for i, hp in enumerate(hps):
        params = {"categorical_columns": ml_100k.get_feature_columns(hp["embedding_size"])["linear"], "fused_step": "on", **hp}
        alone = Estimator(deep_fm.model_fn, model_dir=str(tmp_path / ("alone_%d" % i)), config=config, params=params)
        alone.train(ml_100k.get_input_fn("synthetic:600:1", batch_size=16, seed=7), max_steps=6)
        a, b = side[i]._engine().state_dict(), alone._engine().state_dict()
        assert a["step"] == b["step"] == 6 and set(a) == set(b)
        for key, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, b[key]), (i, key)
        calls = alone._engine().k.calls
        assert calls.get("mi_train_step_model" if hp["optimizer"] != "Adam" else "mi_train_step_fused") == 6
    # evaluate and checkpoints work as for any member
    pop = FusedPopulation([m._engine() for m in members])
    ids, y = FC.draw_batch(np.random.default_rng(2), members[0]._engine().vocab_sizes, 40)
    ms = pop.evaluate(torch.from_numpy(ids), torch.from_numpy(y), batch_size=16)
    assert len(ms) == 4 and all(np.isfinite(m["loss"]) and 0.0 <= m["auc"] <= 1.0 for m in ms)
    again = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "8", "--restore", "--optimizer", "Adam", "Adagrad", "--seeds", "2"))
    assert all(m.global_step == 8 for m in again) and [m._engine().opt.name for m in again] == ["Adam", "Adam", "Adagrad", "Adagrad"]


# ---- what the library refuses on the host ------------------------------------------------------------------------------------
def _library_engine(lib, case):
    k = FusedRulesKernels()
    k.query = lambda name, *a: getattr(lib, name)(*a)
    m = FC.make_engine(case, "cpu", k)
    return m


REFUSALS = {
    "table slot 0 missing": (dict(t_m=None), -1, "table / t_m / t_v (16-byte aligned)"),
    "wide slot 1 missing": (dict(l_v=None), -1, "lin_w / l_m / l_v"),
    "dense slot 1 missing": (dict(d_v=None), -1, "dense / d_m / d_v / n_dense"),
    "wide dense slot 0 missing": (dict(dw_m=None), -1, "dw_m / dw_v (the wide rule's dense slots)"),
    "last_step NULL with an Adam part": (dict(last_step=None), -1, "field_off / ids / labels / last_step"),
    "two_rules without use_linear": (dict(use_linear=0), -1, "two_rules without the wide part (use_linear = 0)"),
    "wide_fields bit F": (dict(wide_fields=1 << 4), -1, "wide_fields names a field at or above F=4"),
    "wide_fields bit 40": (dict(wide_fields=(1 << 40) | 1), -1, "wide_fields names a field at or above F=4"),
    "Ftrl lr_power": (dict(hp_wide=OptimizerSpec("Ftrl", 0.1, lr_power=-0.4).hparams()), -1,
                      "Ftrl learning_rate_power -0.400000 unsupported (TF default -0.5 only)"),
    "optimizer kind 5": (dict(hp=_lib.OptHparams(5, 0.1, 0.9, 0.999, 1e-8, 0, 0, 0, -0.5, 0, 0)), -1, "optimizer kind 5 (0 to 4)"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_new_entries_refuse_alike_and_write_nothing(lib, case):
    """the real library, as test_plan_parity_cpu.py does it for the Adam-only pair: the same description to the solo entry and,
    as member 1 of 3, to the plan; Adam on the table, Ftrl on the wide part, so that every slot and the stamps are needed"""
    at, status, text = REFUSALS[case]
    spec = dict(flags=(True, True, True), hp=("Adam", 0.001), lin_hp=("Ftrl", 0.1))
    es = [_library_engine(lib, spec) for _ in range(3)]
    B, F, keep = 16, 4, []
    pop = FusedPopulation(es)
    ms = (_lib.FusedModel * 3)(*[pop._describe(e, B, keep) for e in es])
    for k, v in at.items():
        setattr(ms[1], k, v)
    m = ms[1]
    field_off = es[0].field_off.data_ptr()
    ids, y = torch.zeros(B, F, dtype=torch.int32), torch.zeros(B, dtype=torch.uint8)
    logits, loss = torch.full((B,), float("nan")), torch.full((1,), float("nan"))
    before = [t.clone() for t in (es[1].t_rec, es[1].lin_state, es[1].dense, es[1].d_s0, es[1].d_s1, es[1].dl_s0, es[1].dl_s1)]
    rc_solo = lib.mi_train_step_model(C.byref(m), field_off, ids.data_ptr(), y.data_ptr(), B, F, 1, 1, logits.data_ptr(),
                                      loss.data_ptr(), 0, None)
    solo = lib.mi_last_error().decode()
    assert rc_solo == status and solo == "train_step_fused: " + text, (rc_solo, solo)
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())
    table = torch.full((int(lib.mi_train_group_plan_bytes(3)),), 0xA5, dtype=torch.uint8)
    plan = _lib.FusedGroupPlan()
    rc_group = lib.mi_train_group_plan_models(ms, 3, B, F, field_off, table.data_ptr(), table.numel(), C.byref(plan), None)
    group = lib.mi_last_error().decode()
    print("%s: solo %d %r, group %d %r" % (case, rc_solo, solo, rc_group, group))
    assert rc_group == rc_solo and group == "train_group_plan: member 1: " + solo
    assert plan.magic == 0 and plan.device_table is None and bool((table == 0xA5).all())
    after = (es[1].t_rec, es[1].lin_state, es[1].dense, es[1].d_s0, es[1].d_s1, es[1].dl_s0, es[1].dl_s1)
    assert all(torch.equal(x, z) for x, z in zip(before, after))


def test_a_schedule_table_is_required_exactly_for_a_rule_under_adam(lib):
    B, F, keep = 16, 4, []
    cases = [(dict(flags=(True, True, True), hp=("Adam", 0.001), lin_hp=("Ftrl", 0.1)), "lr_table", "lr_table of 0 entries"),
             (dict(flags=(True, True, True), hp=("Adagrad", 0.05), lin_hp=("Adam", 0.02)), "lr_table_wide", "lr_table_wide of 0 entries")]
    for spec, field, text in cases:
        e = _library_engine(lib, spec)
        m = FusedPopulation([e])._describe(e, B, keep)
        assert bool(m.lr_table) == (spec["hp"][0] == "Adam") and bool(m.lr_table_wide) == (spec["lin_hp"][0] == "Adam")
        setattr(m, field, None)
        setattr(m, field + "_len", 0)
        table = torch.full((int(lib.mi_train_group_plan_bytes(1)),), 0xA5, dtype=torch.uint8)
        plan = _lib.FusedGroupPlan()
        rc = lib.mi_train_group_plan_models((_lib.FusedModel * 1)(m), 1, B, F, e.field_off.data_ptr(), table.data_ptr(), table.numel(),
                                            C.byref(plan), None)
        err = lib.mi_last_error().decode()
        assert rc == -1 and err.startswith("train_group_plan: member 0: train_step_fused: " + text), err
        assert plan.magic == 0 and bool((table == 0xA5).all())
    # the Adam-only entries keep their refusal
    e = _library_engine(lib, dict(flags=(True, True, True), hp=("Adam", 0.001)))
    m = FusedPopulation([e])._describe(e, B, keep)
    assert isinstance(m, _lib.FusedMember)
    m.hp = OptimizerSpec("SGD", 0.1).hparams()
    plan = _lib.FusedGroupPlan()
    rc = lib.mi_train_group_plan((_lib.FusedMember * 1)(m), 1, B, F, e.field_off.data_ptr(), table.data_ptr(), table.numel(),
                                 C.byref(plan), None)
    assert rc == -2 and lib.mi_last_error().decode() == "train_group_plan: member 0: train_step_fused: optimizer kind 4 (Adam only)"
