"""CPU: the host side of the one-launch train step — DeepFM.fused_train_step / fused_step_ok, model.run_batch's
params["fused_step"], the trainers' --fused-step flag.  mi_train_step_fused is stood in by a numpy restatement of its
contract in include/mi355x_rec.h (tests.cpu_kernels.NumpyKernels); the real kernel is tested in test_hip_fused_step.py."""
import os

import numpy as np
import pytest
import torch

from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.predictor import Predictor
from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import ML100K_VOCAB
from tests.cpu_kernels import NumpyKernels, cpu_kernels  # noqa: F401  (a fixture)
from tests.util import _check_vars, _fresh_ids, _t, dropout_mask, make_problem
from trainers import _cli, deep, deep_fm, linear, linear_deep, ml_100k

_DEEP_FM_OPT = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")


def _engine(vocab, E, hidden, **kw):
    opt = kw.pop("optimizer", OptimizerSpec("Adam", 0.001))
    return DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=opt, device="cpu", _kernels=NumpyKernels(), **kw)


@pytest.mark.parametrize("vocab,E,hidden,B,dropout", [(ML100K_VOCAB, 4, [16, 16], 32, 0.0), ([9, 13, 5, 6], 8, [16, 8], 64, 0.25)])
def test_fused_train_step_matches_oracle(vocab, E, hidden, B, dropout):
    p, _, _, y = make_problem(11, vocab, E, hidden, B)
    m = _engine(vocab, E, hidden, dropout=dropout, seed=3)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(11)
    for step in range(5):
        ids = _fresh_ids(rng, vocab, B)
        kw = {}
        if dropout:
            kw = dict(dropout_masks=[dropout_mask(m._layer_seed(i), B, h, 1 - dropout) for i, h in enumerate(hidden)],
                      keep_prob=1 - dropout)
        lo, logit_o = O.train_step(p, st, ids, y, **kw)
        lg, logit_g = m.fused_train_step(_t(ids), _t(y))
        assert abs(lg.item() - float(lo)) < 2e-5 * abs(float(lo)), step
        assert np.allclose(logit_g.numpy(), logit_o, rtol=1e-5, atol=2e-6), step
        assert m.step == step + 1 and m._final_step == m.step and bool((m.last_step == m.step).all())
    _check_vars(m, p, 2e-6)
    assert m.k.calls["mi_train_step_fused"] == 5 and "mi_sparse_catchup" not in m.k.calls and "mi_dense_fwd" not in m.k.calls


def test_fused_steps_interleave_with_every_other_step():
    vocab, E, hidden, B = [9, 13, 5, 6], 8, [16, 8], 64
    p, _, _, y = make_problem(12, vocab, E, hidden, B)
    m = _engine(vocab, E, hidden, catchup="exact")
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(12)
    for kind in ("fused", "layered", "layered", "fused", "loss", "fused"):
        ids = _fresh_ids(rng, vocab, B)
        if kind == "loss":
            c = O.forward(p, ids)
            loss, logits = m.loss(_t(ids), _t(y))
            assert np.allclose(logits.numpy(), c["logits"], rtol=1e-5, atol=2e-6)
            continue
        lo, logit_o = O.train_step(p, st, ids, y)
        lg, logit_g = (m.fused_train_step if kind == "fused" else m.train_step)(_t(ids), _t(y))
        assert abs(lg.item() - float(lo)) < 2e-5 * abs(float(lo)), kind
        assert np.allclose(logit_g.numpy(), logit_o, rtol=1e-5, atol=2e-6), kind
        if kind == "fused":
            assert bool((m.last_step == m.step).all()) and m._final_step == m.step
            before = dict(m.k.calls)
            m.finalize_rows()
            assert m.k.calls == before                      # nothing is owed after a fused step
    assert m.step == 5
    _check_vars(m, p, 2e-6)
    sd = m.state_dict()                                     # a checkpoint after a fused step restores and carries on
    m2 = _engine(vocab, E, hidden, catchup="exact")
    m2.load_state_dict(sd)
    ids = _fresh_ids(rng, vocab, B)
    la, _ = m.fused_train_step(_t(ids), _t(y))
    lb, _ = m2.fused_train_step(_t(ids), _t(y))
    assert la.item() == lb.item() and torch.equal(m.t_rec, m2.t_rec) and torch.equal(m.dense, m2.dense)


@pytest.mark.parametrize("kw,B,msg", [
    (dict(optimizer=OptimizerSpec("Adagrad", 0.05)), 8, "Adam for every variable"),
    (dict(linear_optimizer=OptimizerSpec("Adam", 0.01)), 8, "Adam for every variable"),
    (dict(n_numeric=2), 8, "numeric columns"),
    (dict(use_mf=False, field_dims=[4, 2, 4]), 8, "field_dims / wide_fields"),
    (dict(use_mf=False, wide_fields=[True, False, True]), 8, "field_dims / wide_fields"),
    (dict(vocab=[3] * 33), 8, "33 categorical fields"),
    (dict(E=32), 8, "embedding size 32"),
    (dict(hidden=[8, 8, 8, 8]), 8, "4 hidden layers"),
    (dict(hidden=[65]), 8, "a hidden layer of 65 units"),
    (dict(vocab=[(1 << 18) - 8, 5, 4]), 8, "table rows"),
    (dict(), 129, "a batch of 129 examples"),
    (dict(vocab=[3] * 32, E=16), 33, "B \\* F \\* E = 16896"),
])
def test_models_outside_the_scope_are_refused_before_any_launch(kw, B, msg):
    kw = dict(kw)
    vocab, E, hidden = kw.pop("vocab", [9, 13, 5]), kw.pop("E", 4), kw.pop("hidden", [8])
    nn = kw.pop("n_numeric", 0)
    m = DeepFM(vocab, n_numeric=nn, embedding_size=E, hidden_units=hidden, device="cpu", _kernels=NumpyKernels(),
               optimizer=kw.pop("optimizer", OptimizerSpec("Adam", 0.001)), **kw)
    assert not m.fused_step_ok(B) and m._fused_step_limit(B)
    ids = torch.zeros(B, len(vocab), dtype=torch.int32)
    with pytest.raises(ValueError, match=msg):
        m.fused_train_step(ids, torch.zeros(B, dtype=torch.uint8))
    assert not m.k.calls and m.step == 0


def test_limits_are_inclusive():
    assert _engine([3] * 32, 16, [64, 64, 64]).fused_step_ok(32)
    assert _engine([3] * 32, 4, [64]).fused_step_ok(128)
    assert _engine([(1 << 18) - 9, 5, 4], 4, [8]).fused_step_ok(1)
    assert not _engine([3] * 32, 4, [64]).fused_step_ok(0)
    for flags in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        assert _engine([9, 13], 8, [8], use_linear=flags[0], use_mf=flags[1], use_dnn=flags[2]).fused_step_ok(16)


def test_run_batch_honours_off_on_auto_and_summaries(cpu_kernels, monkeypatch):
    cols = ml_100k.get_feature_columns(4)["linear"]
    feats, labels = next(ml_100k.get_input_fn("synthetic:200:1", batch_size=32, seed=0)())

    def run(fs, steps=3, summaries=(), **extra):
        params = {"categorical_columns": cols, "device": "cpu", **extra}
        if fs is not None:
            params["fused_step"] = fs
        deep_fm.model_fn(feats, labels, "_build", params)
        eng = params["_store"]["engine"]
        for i in range(steps):
            eng.summaries_next = i in summaries
            spec = deep_fm.model_fn(feats, labels, "train", params)
        assert spec.train_op == steps
        return eng, eng.k.calls.get("mi_train_step_fused", 0)

    assert run(None)[1] == 0 and run("off")[1] == 0
    eng, n = run("on")
    assert n == 3 and "mi_dense_fwd_gathered" not in eng.k.calls
    eng, n = run("on", steps=4, summaries=(1,))            # the step whose summaries are recorded runs the layered path
    assert n == 3 and eng.step == 4
    assert run("auto")[1] == 3
    monkeypatch.setattr(DeepFM, "FUSED_STEP_MAX_BATCH", 16)
    assert run("auto")[1] == 0
    monkeypatch.setattr(DeepFM, "FUSED_STEP_MAX_BATCH", 128)
    monkeypatch.setattr(DeepFM, "FUSED_STEP_MAX_STATE_BYTES", 1000)
    assert run("auto")[1] == 0
    monkeypatch.setattr(DeepFM, "FUSED_STEP_MAX_STATE_BYTES", 1 << 20)
    assert run("auto")[1] == 3
    assert run("auto", hidden_units=[64, 64])[1] == 0      # in scope, but an MLP larger than the measured winner's
    assert run("on", hidden_units=[64, 64])[1] == 3
    assert run("auto", hidden_units=[128])[1] == 0         # outside the scope: auto stays on today's path
    with pytest.raises(ValueError, match="fused_step=on: the model has a hidden layer of 128 units"):
        run("on", hidden_units=[128])
    with pytest.raises(ValueError, match="fused_step must be"):
        run("yes")


def test_fused_step_flag_on_all_four_clis(cpu_kernels, tmp_path):
    for model, opt in (("deep_fm", _DEEP_FM_OPT), ("linear", ()), ("deep", ("hidden_units", "dropout")),
                       ("linear_deep", ("hidden_units", "dropout"))):
        parser = _cli.make_parser(model, opt)
        assert parser.parse_args([]).fused_step == "off"
        assert parser.parse_args(["--fused-step"]).fused_step == "on"
        assert parser.parse_args(["--fused-step", "auto"]).fused_step == "auto"
        with pytest.raises(SystemExit):
            parser.parse_args(["--fused-step", "maybe"])
    # the canned estimators (Ftrl / Adagrad) are outside the scope: "on" is refused with the reason, "auto" leaves them alone
    for trainer, opt, extra in ((linear, (), []), (deep, ("hidden_units", "dropout"), ["--hidden-units", "8"]),
                                (linear_deep, ("hidden_units", "dropout"), ["--hidden-units", "8"])):
        name = trainer.__name__.split(".")[-1]
        argv = ["--synthetic", "200", "--job-dir", str(tmp_path / name), "--train-steps", "5", "--batch-size", "16",
                "--device", "cpu"] + extra
        with pytest.raises(ValueError, match="fused_step=on: the model has optimizer"):
            trainer.train_and_evaluate(_cli.make_parser(name, opt).parse_args(argv + ["--fused-step", "on"]))
        est = trainer.train_and_evaluate(_cli.make_parser(name, opt).parse_args(argv + ["--fused-step", "auto"]))
        assert est.global_step == 5 and "mi_train_step_fused" not in est._engine().k.calls


def test_deep_fm_cli_trains_with_the_fused_step(cpu_kernels, tmp_path, capsys):
    job = str(tmp_path / "job")
    argv = ["--synthetic", "300", "--job-dir", job, "--train-steps", "25", "--batch-size", "16", "--device", "cpu",
            "--hidden-units", "8", "8", "--dropout", "0.1", "--fused-step", "on"]
    est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", _DEEP_FM_OPT).parse_args(argv))
    eng = est._engine()
    assert est.global_step == 25 and eng.k.calls["mi_train_step_fused"] == 25
    assert "mi_sparse_apply_fused" not in eng.k.calls and "mi_sparse_apply" not in eng.k.calls
    out = capsys.readouterr().out
    assert "Saving dict for global step 25" in out and "auc = " in out
    assert os.path.exists(os.path.join(job, "model.ckpt-25.pt"))
    # restore: a run without the flag continues from the checkpoint, and one with it too
    est2 = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", _DEEP_FM_OPT).parse_args(
        argv[:-2] + ["--restore", "--train-steps", "30"]))
    assert est2.global_step == 30 and "restored" in capsys.readouterr().out
    est3 = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", _DEEP_FM_OPT).parse_args(argv + ["--restore", "--train-steps", "35"]))
    assert est3.global_step == 35 and est3._engine().k.calls["mi_train_step_fused"] == 5
    m = est3.evaluate(ml_100k.get_input_fn("synthetic:30:2", "eval", 16))
    assert {"accuracy", "auc", "average_loss", "loss", "global_step"} <= set(m) and np.isfinite(m["loss"])
    root = os.path.join(job, "export", "exporter")
    newest = os.path.join(root, sorted(os.listdir(root))[-1])
    pred = Predictor.from_export(newest, device="cpu")
    cols, _ = ml_100k._read_csv("synthetic:10:2")
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    out = pred({k: v for k, v in cols.items() if k in recv})
    assert np.asarray(out["logistic"]).reshape(-1).shape == (10,)
