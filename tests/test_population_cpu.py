"""CPU: the host side of the population step — mi355x_rec.population.FusedPopulation and the trainers.sweep CLI.
mi_train_group_plan / mi_train_group_step are stood in by a numpy restatement of their contract in include/mi355x_rec.h
(tests.cpu_kernels.NumpyKernels: a member is what mi_train_step_fused does to its buffers with lr_t = lr_table[step] and
seed = seed_base + step * 1000003); the real kernel is tested in test_hip_population.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import AdamSchedule, OptimizerSpec
from mi355x_rec.population import FusedPopulation
from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import ML100K_VOCAB, ORACLE_MEMBERS, _numpy_engine, _sweep_args
from tests.cpu_kernels import NumpyKernels, cpu_kernels, library_sized  # noqa: F401  (cpu_kernels: a fixture)
from tests.util import _check_vars, _fresh_ids, _t, make_problem

def _oracle_population(k, members=ORACLE_MEMBERS, B=32):
    engines, params, states = [], [], []
    for seed, E, hidden, lr in members:
        p = make_problem(seed, ML100K_VOCAB, E, hidden, B)[0]
        m = _numpy_engine(ML100K_VOCAB, E, hidden, k, lr)
        m.load_oracle_params(p)
        engines.append(m)
        params.append(p)
        states.append(O.TrainState(p, OO.Hyper("Adam", lr)))
    return engines, params, states


def test_one_entry_call_per_step_and_members_match_the_oracle():
    B = 32
    k = NumpyKernels()
    engines, params, states = _oracle_population(k)
    y = make_problem(300, ML100K_VOCAB, 4, [16, 16], B)[3]
    pop = FusedPopulation(engines)
    rng = np.random.default_rng(300)
    k.calls.clear()
    for step in range(2):
        ids = _fresh_ids(rng, ML100K_VOCAB, B)
        loss, logits = pop.train_step(_t(ids), _t(y))
        assert tuple(loss.shape) == (6,) and tuple(logits.shape) == (6, B)
        for i, (p, st) in enumerate(zip(params, states)):
            lo, zo = O.train_step(p, st, ids, y)
            assert abs(loss[i].item() - float(lo)) < 2e-5 * abs(float(lo)), (step, i)
            assert np.allclose(logits[i].numpy(), zo, rtol=1e-5, atol=2e-6), (step, i)
    assert k.calls == {"mi_train_group_plan": 1, "mi_train_group_step": 2}
    for m, p in zip(engines, params):
        assert m.step == m._final_step == 2 and bool((m.last_step == 2).all())
        _check_vars(m, p, 2e-6)


def test_a_member_is_its_own_fused_step_bit_for_bit_with_shared_and_per_member_batches():
    B, vocab = 16, [9, 13, 5, 6]
    specs = [dict(E=8, hidden=[16, 8], dropout=0.25, seed=3), dict(E=4, hidden=[8], lr=0.01, activation="tanh"),
             dict(E=8, hidden=[16, 8], use_linear=False, reduction="sum"), dict(E=4, hidden=[], use_dnn=False, seed=9)]

    def make(k):
        out = []
        for j, s in enumerate(specs):
            s = dict(s)
            m = _numpy_engine(vocab, s.pop("E"), s.pop("hidden"), k, s.pop("lr", 0.001), **s)
            g = torch.Generator()
            g.manual_seed(j)
            m.init_variables(g, lin_scale=0.05)
            out.append(m)
        return out
    k = NumpyKernels()
    group, solo = make(k), make(NumpyKernels())
    pop = FusedPopulation(group)
    rng = np.random.default_rng(4)
    for step in range(4):
        per_member = step % 2 == 1
        ids = np.stack([_fresh_ids(rng, vocab, B) for _ in specs]) if per_member else _fresh_ids(rng, vocab, B)
        y = (rng.random((len(specs), B) if per_member else B) < 0.3).astype(np.uint8)
        loss, logits = pop.train_step(_t(ids), _t(y))
        for i, s in enumerate(solo):
            ls, zs = s.fused_train_step(_t(ids[i] if per_member else ids), _t(y[i] if per_member else y))
            assert torch.equal(ls, loss[i:i + 1]) and torch.equal(zs, logits[i]), (step, i)
            g = group[i]
            for a, b in ((g.t_rec, s.t_rec), (g.lin_state, s.lin_state), (g.dense, s.dense), (g.d_s0, s.d_s0), (g.d_s1, s.d_s1)):
                assert (a is None and b is None) or torch.equal(a, b), (step, i)
            assert g.step == s.step == step + 1 and g._final_step == g.step
    assert "mi_train_step_fused" not in k.calls and k.calls["mi_train_group_step"] == 4 and k.calls["mi_train_group_plan"] == 1


def test_the_plan_is_reused_and_rebuilt_only_when_it_must_be():
    vocab, B = [9, 13, 5], 8
    k = NumpyKernels()
    engines = [_numpy_engine(vocab, 4, [8], k, lr) for lr in (0.001, 0.01, 0.003)]
    engines[1].sched = AdamSchedule(engines[1].opt, engines[1].device, capacity=4)
    pop = FusedPopulation(engines)
    rng = np.random.default_rng(0)
    ids, y = _t(_fresh_ids(rng, vocab, B)), _t((rng.random(B) < 0.3).astype(np.uint8))
    plans = lambda: k.calls.get("mi_train_group_plan", 0)
    for _ in range(4):
        pop.train_step(ids, y)
    assert plans() == 1
    pop.train_step(ids, y)                               # step 5: member 1's table of 4 steps is extended and moves
    assert plans() == 2 and engines[1].sched.gen == 2
    for _ in range(5):
        pop.train_step(ids, y)                           # ... to step 10
    assert plans() == 2
    pop.train_step(ids, y)                               # step 11: extended again
    assert plans() == 3
    ids2, y2 = _t(_fresh_ids(rng, vocab, 12)), _t((rng.random(12) < 0.3).astype(np.uint8))
    pop.train_step(ids2, y2)                             # a new batch size
    assert plans() == 4
    pop.train_step(ids2, y2)
    sd = [m.state_dict() for m in engines]
    for m, s in zip(engines, sd):
        m.load_state_dict(s)                             # in place: no rebuild
    pop.train_step(ids2, y2)
    assert plans() == 4
    pop.rebuild()
    pop.train_step(ids2, y2)
    assert plans() == 5 and all(m.step == 15 for m in engines) and k.calls["mi_train_group_step"] == 15
    assert "mi_sparse_catchup" not in k.calls and "mi_train_step_fused" not in k.calls


def test_refusals_before_anything_is_launched():
    vocab, B = [9, 13, 5], 8
    k = NumpyKernels()
    mk = lambda **kw: _numpy_engine(kw.pop("vocab", vocab), kw.pop("E", 4), kw.pop("hidden", [8]), k, **kw)
    ids, y = torch.zeros(B, 3, dtype=torch.int32), torch.zeros(B, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no members"):
        FusedPopulation([])
    a = mk()
    with pytest.raises(ValueError, match="member 1 is the same engine as member 0"):
        FusedPopulation([a, a])
    with pytest.raises(ValueError, match="member 1: the model has a hidden layer of 65 units"):
        FusedPopulation([a, mk(hidden=[65])])
    with pytest.raises(ValueError, match="member 2: the model has optimizer Adagrad"):
        FusedPopulation([a, mk(), mk(optimizer=OptimizerSpec("Adagrad", 0.05))])
    with pytest.raises(ValueError, match="member 1 has other vocab_sizes than member 0 \\(4 fields against 3\\)"):
        FusedPopulation([a, mk(vocab=[9, 13, 5, 6])])
    with pytest.raises(ValueError, match="member 1 has other vocab_sizes"):
        FusedPopulation([a, mk(vocab=[9, 13, 6])])
    with pytest.raises(ValueError, match="at most %d in one launch" % FusedPopulation.MAX_MEMBERS):
        FusedPopulation([a] * (FusedPopulation.MAX_MEMBERS + 1))
    b = mk()
    b.device = torch.device("meta")
    with pytest.raises(ValueError, match="member 1 lives on meta, member 0 on cpu"):
        FusedPopulation([a, b])
    pop = FusedPopulation([a, mk(), mk()])
    with pytest.raises(ValueError, match="member 0: the model has a batch of 129 examples"):
        pop.train_step(torch.zeros(129, 3, dtype=torch.int32), torch.zeros(129, dtype=torch.uint8))
    for bad_ids, bad_y, msg in ((ids.long(), y, "ids must be"), (ids[:, :2].contiguous(), y, "ids must be"),
                                (torch.zeros(2, B, 3, dtype=torch.int32), y, "ids must be"), (ids, y.float(), "labels must be"),
                                (ids, y[:4], "labels must be"), (ids, torch.zeros(2, B, dtype=torch.uint8), "labels must be"),
                                (ids.numpy(), y, "ids must be")):
        with pytest.raises(ValueError, match=msg):
            pop.train_step(bad_ids, bad_y)
    assert not k.calls
    pop.train_step(ids, y)
    pop.engines[1].fused_train_step(ids, y)
    before = dict(k.calls)
    with pytest.raises(ValueError, match="member 1 is at step 2, member 0 at step 1"):
        pop.train_step(ids, y)
    assert k.calls == before and [m.step for m in pop.engines] == [1, 2, 1]
    pop.engines[0].fused_train_step(ids, y)
    pop.engines[2].train_step(ids, y)                    # (the layered step: rows are owed, the population settles them)
    pop.train_step(ids, y)
    assert [m.step for m in pop.engines] == [3, 3, 3] and all(m._final_step == 3 for m in pop.engines)


# ---- the grid-search CLI ----------------------------------------------------------------------------------------------
def test_sweep_parser_defaults():
    from trainers import sweep
    a = sweep.make_parser().parse_args([])
    assert (a.learning_rate, a.dropout, a.embedding_size, a.hidden_units, a.seeds, a.select) == ([0.001], [0.1], [4], None, 1, "auc")
    assert a.batch_size == 32 and a.train_steps == 20000 and a.job_dir == "checkpoints/sweep" and not a.restore
    assert sweep.grid(a) == [dict(embedding_size=4, hidden_units=[16, 16], dropout=0.1, learning_rate=0.001, seed=0)]
    a = sweep.make_parser().parse_args(["--learning-rate", "0.001", "0.01", "--hidden-units", "8", "--hidden-units", "16", "8",
                                        "--seeds", "3", "--embedding-size", "4", "8", "--select", "loss"])
    g = sweep.grid(a)
    assert len(g) == 2 * 2 * 2 * 3 and a.hidden_units == [[8], [16, 8]] and a.select == "loss"
    assert g[0] == dict(embedding_size=4, hidden_units=[8], dropout=0.1, learning_rate=0.001, seed=0)
    assert g[-1] == dict(embedding_size=8, hidden_units=[16, 8], dropout=0.1, learning_rate=0.01, seed=2)
    a.seeds = 600
    with pytest.raises(ValueError, match="the grid has 4800 members \\(at most %d" % FusedPopulation.MAX_MEMBERS):
        sweep.grid(a)
    assert "layer" in sweep.make_parser().format_help() and "0.001" in sweep.make_parser().format_help()


def test_sweep_cli_end_to_end(cpu_kernels, tmp_path, capsys):
    from trainers import _cli, deep_fm, sweep
    job = tmp_path / "job"
    grid_flags = ["--learning-rate", "0.001", "0.01", "--dropout", "0", "0.1"]
    members = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "25", *grid_flags))
    assert len(members) == 4 and all(m.global_step == 25 for m in members)
    k = members[0]._engine().k
    out = capsys.readouterr().out
    assert "best of 4 members by auc" in out
    doc = json.load(open(job / "sweep.json"))
    rows = doc["members"]
    assert doc["select"] == "auc" and sorted(r["member"] for r in rows) == [0, 1, 2, 3]
    aucs = [r["metrics"]["auc"] for r in rows]
    assert aucs == sorted(aucs, reverse=True) and all(np.isfinite(list(r["metrics"].values())).all() for r in rows)
    by = {r["member"]: r for r in rows}
    assert [(by[i]["params"]["dropout"], by[i]["params"]["learning_rate"]) for i in range(4)] == [(0.0, 0.001), (0.0, 0.01),
                                                                                                 (0.1, 0.001), (0.1, 0.01)]
    assert by[2]["flags"] == ["--embedding-size", "4", "--hidden-units", "8", "8", "--dropout", "0.1"]
    for i in range(4):
        assert os.path.exists(job / ("member_%d" % i) / "model.ckpt-25.pt") and os.path.isdir(by[i]["export"])
        eng = members[i]._engine()
        assert eng.k.calls.get("mi_train_step_fused", 0) == 0 and eng.opt.lr == by[i]["params"]["learning_rate"]
        assert not os.path.exists(job / ("member_%d" % i) / "summaries.jsonl")
    assert sum(m._engine().k.calls.get("mi_train_group_step", 0) for m in members) == 25   # one entry call per step, for all four
    # --restore: every member from its own newest checkpoint, at its own rate; --select loss sorts ascending
    again = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "30", "--restore", "--select", "loss", *grid_flags))
    assert all(m.global_step == 30 for m in again) and "restored" in capsys.readouterr().out
    assert [m._engine().opt.lr for m in again] == [0.001, 0.01, 0.001, 0.01]
    rows = json.load(open(job / "sweep.json"))["members"]
    losses = [r["metrics"]["loss"] for r in rows]
    assert losses == sorted(losses) and all(r["global_step"] == 30 for r in rows)
    # a member is an ordinary job directory: trainers.deep_fm --restore carries it on (at that CLI's learning rate)
    opt = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")
    est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(
        ["--synthetic", "300", "--job-dir", str(job / "member_2"), "--batch-size", "16", "--device", "cpu", "--restore",
         "--train-steps", "33"] + by[2]["flags"]))
    assert est.global_step == 33 and est._engine().opt.lr == 0.001
    with pytest.raises(ValueError, match="different steps .*member 1 at step 30, member 2 at step 33"):
        sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "40", "--restore", *grid_flags))


def test_sweep_refuses_a_member_outside_the_scope_before_any_step(cpu_kernels, tmp_path):
    from trainers import sweep
    args = sweep.make_parser().parse_args(["--synthetic", "300", "--job-dir", str(tmp_path / "job"), "--batch-size", "16",
                                           "--device", "cpu", "--hidden-units", "8", "--hidden-units", "128", "--train-steps", "5"])
    with pytest.raises(ValueError, match="member 1 .*: the model has a hidden layer of 128 units"):
        sweep.train_and_evaluate(args)
    assert not os.path.exists(tmp_path / "job" / "member_0" / "checkpoint.json")


def test_a_sweep_member_is_a_stand_alone_run(cpu_kernels, tmp_path):
    from mi355x_rec.estimator import Estimator
    from trainers import _cli, deep_fm, ml_100k, sweep
    args = _sweep_args(tmp_path / "job", "--learning-rate", "0.001", "0.01", "--dropout", "0.1")
    config = _cli.get_run_config()
    config.device = "cpu"
    hps = sweep.grid(args)
    members = sweep.make_members(args, hps, config)
    input_fn = ml_100k.get_input_fn("synthetic:2000:1", batch_size=32, seed=7)
    sweep.train(members, input_fn, 40, config)
    for i, hp in enumerate(hps):
        params = {"categorical_columns": ml_100k.get_feature_columns(hp["embedding_size"])["linear"], "fused_step": "on", **hp}
        alone = Estimator(deep_fm.model_fn, model_dir=str(tmp_path / ("alone_%d" % i)), config=config, params=params)
        alone.train(ml_100k.get_input_fn("synthetic:2000:1", batch_size=32, seed=7), max_steps=40)
        a, b = members[i]._engine().state_dict(), alone._engine().state_dict()
        assert a["step"] == b["step"] == 40 and set(a) == set(b)
        for key, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, b[key]), (i, key)
        assert alone._engine().k.calls["mi_train_step_fused"] == 40


def test_the_library_itself_refuses_on_the_host_before_it_touches_a_device(lib):
    """The real mi_train_group_plan / mi_train_group_step on this machine: every refusal is decided on the host from the
    members' descriptions (which also pins the binding's struct layout to the header's)."""
    k = library_sized(lib)
    es = [_numpy_engine([9, 13, 5], 4, [8], k), _numpy_engine([9, 13, 5], 8, [16, 8], k, dropout=0.25), _numpy_engine([9, 13, 5], 4, [8], k)]
    pop, keep = FusedPopulation(es), []
    table = torch.full((int(lib.mi_train_group_plan_bytes(3)),), 0xA5, dtype=torch.uint8)

    def plan_call(match, status, edit=None, n=3, B=16):
        ms = (_lib.FusedMember * 3)(*[pop._describe(e, B, keep) for e in es])
        if edit:
            edit(ms)
        plan = _lib.FusedGroupPlan()
        rc = lib.mi_train_group_plan(ms, n, B, 3, es[0].field_off.data_ptr(), table.data_ptr(), table.numel(), C.byref(plan), None)
        msg = lib.mi_last_error().decode()
        assert rc == status and match in msg, (rc, msg)
        assert plan.magic == 0 and plan.device_table is None and bool((table == 0xA5).all())      # nothing was written
        return plan
    assert C.sizeof(_lib.FusedMember) * 3 <= lib.mi_train_group_plan_bytes(3) <= 4096 * 3 and lib.mi_train_group_plan_bytes(-1) == 0
    plan_call("0 members (at least 1)", -1, n=0)
    plan_call("1025 members (at most 1024 in one launch)", -2, n=_lib.FUSED_GROUP_MAX_MEMBERS + 1)
    plan_call("member 0: train_step_fused: B=129 (1 to 128 examples)", -2, B=129)
    plan_call("member 1: train_step_fused: embedding size 20", -2, lambda ms: setattr(ms[1], "E", 20))
    plan_call("member 1: train_step_fused: 4 hidden layers (at most 3)", -2, lambda ms: setattr(ms[1], "n_layers", 5))
    plan_call("member 2: train_step_fused: keep_prob=0", -1, lambda ms: setattr(ms[2], "keep_prob", 0.0))
    plan_call("member 1: train_step_fused: optimizer kind 1 (Adam only)", -2,
              lambda ms: setattr(ms[1], "hp", OptimizerSpec("Adagrad", 0.05).hparams()))
    plan_call("member 1: train_step_fused: lr_table of 1 entries", -1, lambda ms: setattr(ms[1], "lr_table_len", 1))
    plan_call("member 1: train_step_fused: workspace of 8 bytes", -4, lambda ms: setattr(ms[1], "workspace_bytes", 8))
    plan_call("member 0 and member 2 share a state or workspace pointer", -1, lambda ms: setattr(ms[2], "d_v", ms[0].d_v))
    plan = plan_call("member 0 and member 1 share", -1, lambda ms: setattr(ms[1], "workspace", ms[0].workspace))
    ids, y = torch.zeros(16, 3, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8)
    logits, loss = torch.full((3, 16), float("nan")), torch.full((3,), float("nan"))
    rc = lib.mi_train_group_step(C.byref(plan), 3, ids.data_ptr(), 0, y.data_ptr(), 0, 16, 1, logits.data_ptr(), loss.data_ptr(), 0, None)
    assert rc == -1 and "train_group_step: plan" in lib.mi_last_error().decode()
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())
