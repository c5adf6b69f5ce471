"""CPU: the host side of the one-launch train step — DeepFM.fused_train_step / fused_step_ok, model.run_batch's
params["fused_step"], the trainers' --fused-step flag.  mi_train_step_fused is stood in by a numpy restatement of its
contract in include/mi355x_rec.h on top of the other numpy stand-ins (FusedStepKernels below); the real kernel is
tested in test_hip_fused_step.py."""
import os

import numpy as np
import pytest
import torch

from mi355x_rec import engine
from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.predictor import Predictor
from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cpu_kernels import _hyper
from tests.test_predictor_cpu import ServeKernels
from tests.util import MASK64, dropout_mask, make_problem
from trainers import _cli, deep, deep_fm, linear, linear_deep, ml_100k

ML100K_VOCAB = [2, 2, 7, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 2000, 2, 2, 50, 8, 2, 2, 2, 2, 1000, 2, 2, 1000]
_ACT = {0: lambda v: v, 1: lambda v: np.maximum(v, 0), 2: lambda v: 1 / (1 + np.exp(-v)), 3: np.tanh}
_DEEP_FM_OPT = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")


class FusedStepKernels(ServeKernels):
    """The numpy stand-ins + mi_train_step_fused restated from include/mi355x_rec.h (fp32 numpy, independent of the layered
    stand-ins: its own forward, backward, touched-row apply and all-rows sweep).  `calls` counts the entries fetched."""

    def __init__(self):
        self.calls = {}

    def __getattribute__(self, name):
        value = object.__getattribute__(self, name)
        if name.startswith("mi_"):
            calls = object.__getattribute__(self, "calls")
            calls[name] = calls.get(name, 0) + 1
        return value

    def mi_train_step_fused(self, table, t_m, t_v, ts, lin_w, l_m, l_v, ls, last_step, field_off, R, ids, labels, B, F, E,
                            dense, d_m, d_v, n_dense, layer_off, widths, n_layers, act, use_linear, use_fm, use_dnn,
                            lin_bias_off, keep, seed, scale, step, hp, logits, loss, sweep_blocks, ws, wsb):
        f32 = np.float32
        assert hp.kind == 0 and 1 <= B <= 128 and 1 <= F <= 32 and R <= 1 << 18 and n_layers <= 4
        assert bool((last_step.numpy() == step - 1).all()) or step == 1, "every row must be current"
        keep, scale, lr_t = f32(keep), f32(scale), f32(hp.lr_t)
        b1, b2, eps = f32(hp.beta1), f32(hp.beta2), f32(hp.epsilon)
        d = dense.numpy()
        rows = ids.numpy().astype(np.int64) + field_off.numpy()[None, :]
        emb = bool(use_fm or use_dnn)
        T = table.numpy() if emb else None
        V = T[rows] if emb else None                                  # [B, F, E]
        z = np.zeros(B, f32)
        if use_linear:
            z = z + (lin_w.numpy()[rows].sum(1, dtype=f32) + d[lin_bias_off])
        s = None
        if use_fm:
            s = V.sum(1, dtype=f32)
            z = z + f32(0.5) * (s * s - (V * V).sum(1, dtype=f32)).sum(1, dtype=f32)
        acts, Ws = [], []
        lo, wd = layer_off.numpy(), widths.numpy()
        if use_dnn:
            h = V.reshape(B, F * E)
            for i in range(n_layers):
                W = d[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]].reshape(wd[i], wd[i + 1])
                acts.append(h)
                Ws.append(W.copy())
                h = (h @ W + d[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]]).astype(f32)
                if i + 1 < n_layers:
                    h = _ACT[act](h).astype(f32)
                    if keep < 1:
                        h = (h / keep) * dropout_mask((seed + 7919 * i) & MASK64, B, int(wd[i + 1]), keep)
            z = z + h[:, 0]
        y = labels.numpy().astype(f32)
        logits.numpy()[:] = z
        e = np.exp(-np.abs(z))
        loss.numpy()[0] = ((np.maximum(z, 0) - z * y + np.log1p(e)) * scale).sum(dtype=f32)
        dl = ((np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(f32) - y) * scale).astype(f32)
        # backward
        gd = np.zeros(n_dense, f32)
        d_concat = None
        if use_dnn:
            dy = dl[:, None]
            for i in reversed(range(n_layers)):
                gd[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]] = (acts[i].T @ dy).reshape(-1)
                gd[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]] = dy.sum(0, dtype=f32)
                g = (dy @ Ws[i].T).astype(f32)
                if i:
                    x = acts[i]                                        # the layer's stored output: act(pre) / keep, or 0
                    if act == 1:
                        g = np.where(x > 0, g / keep, 0).astype(f32)
                    else:
                        o = x * keep
                        der = {0: np.ones_like(o), 2: o * (1 - o), 3: 1 - o * o}[act]
                        g = np.where((keep < 1) & (x == 0), 0, (g / keep) * der).astype(f32)
                    dy = g
                else:
                    d_concat = g.reshape(B, F, E)
        if use_linear:
            gd[lin_bias_off] = dl.sum(dtype=f32)
        # touched rows: entries summed in ascending entry order, TF's sparse Adam; every other row: one step of the sweep
        flat = rows.reshape(-1)
        touched = np.zeros(R, bool)
        touched[flat] = True
        G = None
        if emb:
            G = np.zeros((B, F, E), f32)
            if d_concat is not None:
                G = G + d_concat
            if use_fm:
                G = G + dl[:, None, None] * (s[:, None, :] - V)
            G = G.reshape(B * F, E)
        gl = np.repeat(dl, F)
        for w, m, v, grad in ((table, t_m, t_v, G), (lin_w, l_m, l_v, gl)):
            if w is None or grad is None or (w is lin_w and not use_linear):
                continue
            Wn, Mn, Vn = w.numpy(), m.numpy(), v.numpy()
            for r in np.flatnonzero(touched):
                g = np.zeros_like(Wn[r])
                for en in np.flatnonzero(flat == r):
                    g = g + grad[en]
                Mn[r] = Mn[r] * b1 + g * (f32(1) - b1)
                Vn[r] = Vn[r] * b2 + (g * g) * (f32(1) - b2)
                Wn[r] = Wn[r] - (lr_t * Mn[r]) / (np.sqrt(Vn[r]) + eps)
            u = ~touched
            Mn[u] = Mn[u] * b1
            Vn[u] = Vn[u] * b2
            Wn[u] = Wn[u] - (lr_t * Mn[u]) / (np.sqrt(Vn[u]) + eps)
        last_step.numpy()[:] = step
        OO.dense_apply(_hyper(hp), d, d_m.numpy(), d_v.numpy(), gd, lr_t)


@pytest.fixture
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(engine, "HipKernels", FusedStepKernels)


def _engine(vocab, E, hidden, **kw):
    opt = kw.pop("optimizer", OptimizerSpec("Adam", 0.001))
    return DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=opt, device="cpu", _kernels=FusedStepKernels(), **kw)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _check_vars(m, p, atol):
    g = m.export_numpy()
    for f in range(len(p.emb)):
        assert np.max(np.abs(g["emb"][f] - p.emb[f])) < atol, ("emb", f)
        assert np.max(np.abs(g["lin_w"][f] - p.lin_w[f])) < atol, ("lin_w", f)
    for i, (k, b) in enumerate(g["mlp"]):
        assert np.max(np.abs(k - p.mlp[i][0])) < atol and np.max(np.abs(b - p.mlp[i][1])) < atol, ("mlp", i)
    assert abs(g["lin_bias"][0] - p.lin_bias[0]) < atol


def _fresh_ids(rng, vocab, B):
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    if B > 1:
        ids[B // 2] = ids[0]
    return ids


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
    m = DeepFM(vocab, n_numeric=nn, embedding_size=E, hidden_units=hidden, device="cpu", _kernels=FusedStepKernels(),
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
