"""-m gpu: the one-launch train step (mi_train_step_fused, csrc/train_fused.hip) through engine.DeepFM.fused_train_step,
against the oracle's restatement of trainers/deep_fm.py:36-125 and against the layered step it stands in for.

Bars are the project's own (tests/test_hip_model.py): loss 2e-5 relative, logits 5e-6 on identical
weights and 5e-5 after the first update, every variable 2e-6 absolute (3e-6 for sigmoid / tanh / identity, the bar of
test_canned_parity.test_activation_other_than_relu).  Rows the batch does not touch are held to the BITS of the layered
step's exact one-step catch-up."""
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import FLAGS, ML100K_VOCAB, TRAJECTORIES, _hip_engine
from tests.util import (_compare_vars, _fresh_ids, dev, dropout_mask, guarded_nan, guards_intact, make_problem,
                        max_err_scaled)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("vocab,E,hidden,B,seed", TRAJECTORIES)
def test_trajectory_matches_oracle(vocab, E, hidden, B, seed):
    p, _, _, y = make_problem(seed, vocab, E, hidden, B)
    m = _hip_engine(vocab, E, hidden)
    assert m.fused_step_ok(B)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(seed)
    margin = np.inf
    for step in range(5):
        ids_s = _fresh_ids(rng, vocab, B)
        margin = min(margin, min(float(np.abs(q).min()) for q in O.forward(p, ids_s)["pre"]))
        loss_o, logit_o = O.train_step(p, st, ids_s, y)
        loss_g, logit_g = m.fused_train_step(dev(ids_s), dev(y))
        le = abs(loss_g.item() - float(loss_o)) / abs(float(loss_o))
        ge = max_err_scaled(logit_g.cpu().numpy(), logit_o)
        print("step %d: loss err %.2e, logits err %.2e, margin %.2e" % (step, le, ge, margin))
        assert le < 2e-5, step
        assert ge < (5e-6 if step == 0 else 5e-5), step
        assert bool((m.last_step == m.step).all()) and m._final_step == m.step == step + 1
    assert margin >= 1e-6, margin
    _compare_vars(m, p, 2e-6)


@pytest.mark.parametrize("catchup_b", ["exact", "bounded"])
def test_untouched_rows_get_the_layered_steps_exact_sweep_bit_for_bit(catchup_b):
    vocab, E, hidden, B = ML100K_VOCAB, 4, [16, 16], 32
    p, _, _, y = make_problem(41, vocab, E, hidden, B)
    a = _hip_engine(vocab, E, hidden, catchup="exact", gemm="fp32")        # (exact fp32 products, as the fused step's)
    a.load_oracle_params(p)
    rng = np.random.default_rng(41)
    for _ in range(4):                                       # m and v of many rows are non-zero afterwards
        a.train_step(dev(_fresh_ids(rng, vocab, B)), dev(y))
    b = _hip_engine(vocab, E, hidden, catchup=catchup_b)
    b.load_state_dict(a.state_dict())                        # (state_dict brings every row up to date: both start current)
    assert torch.equal(a.t_rec, b.t_rec) and torch.equal(a.lin_state, b.lin_state) and torch.equal(a.dense, b.dense)
    ids = _fresh_ids(rng, vocab, B)
    la, za = a.train_step(dev(ids), dev(y))
    a.finalize_rows()
    lb, zb = b.fused_train_step(dev(ids), dev(y))
    touched = torch.zeros(a.R, dtype=torch.bool, device="cuda")
    touched[(torch.from_numpy(ids).long() + torch.from_numpy(a.field_off_host[:-1])[None, :]).reshape(-1).cuda()] = True
    assert 0 < int(touched.sum()) < a.R
    u = ~touched
    assert torch.equal(a.t_rec[u], b.t_rec[u])               # table w, m, v of the rows that sat the batch out
    assert torch.equal(a.lin_state[u], b.lin_state[u])       # the wide record w, m, v and the stamp
    assert torch.equal(a.last_step, b.last_step) and bool((b.last_step == 5).all())
    assert float((a.t_rec[touched] - b.t_rec[touched]).abs().max()) < 2e-6
    assert float((a.lin_state[touched][:, :3] - b.lin_state[touched][:, :3]).abs().max()) < 2e-6
    for x, z in ((a.dense, b.dense), (a.d_s0, b.d_s0), (a.d_s1, b.d_s1)):
        assert float((x - z).abs().max()) < 2e-6
    assert abs(la.item() - lb.item()) < 2e-5 * abs(la.item()) and max_err_scaled(zb.cpu().numpy(), za.cpu().numpy()) < 5e-6
    # the sweep did move something: a row touched in the first four steps and not in the fifth has m != 0
    moved = (b.t_rec[u][:, E:2 * E] != 0).any(1)
    assert int(moved.sum()) > 0


@pytest.mark.parametrize("flags", FLAGS)
def test_component_flags(flags):
    ul, um, ud = flags
    vocab, E, hidden, B = [9, 13, 5, 6], 8, [16, 8], 64
    p, ids, x, y = make_problem(2, vocab, E, hidden, B, use_dnn=ud)
    m = _hip_engine(vocab, E, hidden, use_linear=ul, use_mf=um, use_dnn=ud)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    for _ in range(3):
        loss_o, _ = O.train_step(p, st, ids, y, None, ul, um, ud)
        loss_g, _ = m.fused_train_step(dev(ids), dev(y))
        assert abs(loss_g.item() - float(loss_o)) / abs(float(loss_o)) < 2e-5
    _compare_vars(m, p, 2e-6)
    assert bool((m.last_step == 3).all())


@pytest.mark.parametrize("activation,dropout", [("sigmoid", 0.0), ("tanh", 0.2), (None, 0.0), ("sigmoid", 0.2), ("relu", 0.0)])
def test_activations(activation, dropout):
    vocab, E, hidden, B = [9, 13, 5, 6], 8, [16, 8], 48
    p, _, _, _ = make_problem(21, vocab, E, hidden, B)
    m = _hip_engine(vocab, E, hidden, activation=activation, dropout=dropout, seed=3)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(22)
    keep = 1.0 - dropout
    for step in range(3):
        ids = _fresh_ids(rng, vocab, B)
        y = (rng.random(B) < 0.3).astype(np.uint8)
        masks = [dropout_mask(m._layer_seed(i), B, h, keep) for i, h in enumerate(hidden)] if dropout else None
        lo, logit_o = O.train_step(p, st, ids, y, dropout_masks=masks, keep_prob=keep, activation=activation)
        lg, logit_g = m.fused_train_step(dev(ids), dev(y))
        assert abs(lg.item() - float(lo)) <= 2e-5 * abs(float(lo)), step
        assert max_err_scaled(logit_g.cpu().numpy(), logit_o) < (5e-6 if step == 0 else 5e-5), step
    _compare_vars(m, p, 2e-6 if activation == "relu" else 3e-6)


def test_sum_reduction():
    vocab, E, hidden, B = [9, 13, 5], 4, [8], 40
    p, ids, x, y = make_problem(6, vocab, E, hidden, B)
    m = _hip_engine(vocab, E, hidden, reduction="sum")
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    for _ in range(3):
        lo, _ = O.train_step(p, st, ids, y, reduction="sum")
        lg, _ = m.fused_train_step(dev(ids), dev(y))
        assert abs(lg.item() - float(lo)) / abs(float(lo)) < 2e-5
    _compare_vars(m, p, 2e-6)


def test_dropout_training_step_matches_oracle_with_same_mask():
    vocab, E, hidden, B = [9, 13, 5, 6], 8, [32, 16], 128
    p, ids, x, y = make_problem(5, vocab, E, hidden, B)
    m = _hip_engine(vocab, E, hidden, dropout=0.25, seed=7)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    for _ in range(2):
        masks = [dropout_mask(m._layer_seed(i), B, h, 0.75) for i, h in enumerate(hidden)]
        loss_o, _ = O.train_step(p, st, ids, y, dropout_masks=masks, keep_prob=0.75)
        loss_g, _ = m.fused_train_step(dev(ids), dev(y))
        assert abs(loss_g.item() - float(loss_o)) / abs(float(loss_o)) < 2e-5
    _compare_vars(m, p, 2e-6)


def test_fused_and_layered_steps_draw_the_same_dropout_masks_and_interleave():
    """fused, layered, graph, fused, loss, fused against the oracle with the masks of _layer_seed."""
    vocab, E, hidden, B = ML100K_VOCAB, 4, [16, 16], 32
    p, _, _, y = make_problem(300, vocab, E, hidden, B)
    m = _hip_engine(vocab, E, hidden, dropout=0.1, seed=5)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(300)
    for kind in ("fused", "layered", "fused", "graph", "graph", "graph", "fused", "loss", "fused"):
        ids = _fresh_ids(rng, vocab, B)
        if kind == "loss":
            _, z = m.loss(dev(ids), dev(y))
            assert max_err_scaled(z.cpu().numpy(), O.forward(p, ids)["logits"]) < 5e-5
            continue
        masks = [dropout_mask(m._layer_seed(i), B, h, 0.9) for i, h in enumerate(hidden)]
        lo, _ = O.train_step(p, st, ids, y, dropout_masks=masks, keep_prob=0.9)
        step = {"fused": m.fused_train_step, "layered": m.train_step, "graph": m.graph_train_step}[kind]
        lg, _ = step(dev(ids), dev(y))
        assert abs(lg.item() - float(lo)) / abs(float(lo)) < 2e-5, kind
        if kind == "fused":
            assert bool((m.last_step == m.step).all()) and m._final_step == m.step
    assert m.step == 8
    _compare_vars(m, p, 2e-6)


def test_one_field_fm_only_gives_exactly_zero():
    vocab, E, B = [50], 8, 32
    p, ids, x, y = make_problem(9, vocab, E, [], B, use_dnn=False)
    m = _hip_engine(vocab, E, [], use_linear=False, use_mf=True, use_dnn=False)
    m.load_oracle_params(p)
    t0 = m.table.clone()
    for step in range(2):
        loss, logits = m.fused_train_step(dev(ids), dev(y))
        assert bool((logits == 0).all())                      # s * s - v * v with one field: exactly 0
        assert abs(loss.item() - np.log(2.0)) < 1e-6
    assert torch.equal(m.table, t0)                           # zero gradients on m = v = 0: nothing moves, not by a bit
    assert bool((m.t_s0 == 0).all()) and bool((m.t_s1 == 0).all()) and bool((m.last_step == 2).all())


def _raw_step(m, ids, y, logits, loss, sweep_blocks=0, **over):
    """mi_train_step_fused through the binding, as engine.fused_train_step calls it, with overrides."""
    B = over.get("B", ids.shape[0])
    layer_off, widths = m.layer_tables()
    F, E = over.get("F", m.F), over.get("E", m.E)
    nbytes = int(m.k.query("mi_train_step_fused_workspace_bytes", B, F, E, m.P))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    step = m.step + 1
    hp = over.get("hp", m.opt.hparams(m.sched.lr_t(step) if m.sched else 0.0))
    m.k.mi_train_step_fused(m.table, m.t_s0, m.t_s1, m.ts, m.lin_w, m.l_s0, m.l_s1, m.ls, m.last_step, m.field_off,
                            over.get("R", m.R), ids, y, B, F, E, m.dense, m.d_s0, m.d_s1, m.P, layer_off, widths,
                            over.get("n_layers", len(m.layers)), m.act, int(m.use_linear), int(m.use_mf), int(m.use_dnn),
                            m.lin_bias_off, 1.0 - m.dropout, m._layer_seed(0), 1.0 / B, step, hp, logits, loss, sweep_blocks,
                            ws, ws.numel())


@pytest.mark.parametrize("vocab,E,hidden,B", [(ML100K_VOCAB, 4, [16, 16], 32), (ML100K_VOCAB, 16, [64, 64, 32], 32)])
def test_same_bits_twice_and_for_every_sweep_grid(vocab, E, hidden, B):
    p, _, _, y = make_problem(51, vocab, E, hidden, B)
    a = _hip_engine(vocab, E, hidden, dropout=0.1, seed=2)
    a.load_oracle_params(p)
    rng = np.random.default_rng(51)
    for _ in range(3):
        a.fused_train_step(dev(_fresh_ids(rng, vocab, B)), dev(y))
    sd = a.state_dict()
    ids = dev(_fresh_ids(rng, vocab, B))
    results = []
    for blocks in (0, 0, 1, 7, 64):
        m = _hip_engine(vocab, E, hidden, dropout=0.1, seed=2)
        m.load_state_dict(sd)
        gl, logits = guarded_nan(B)
        gs, loss = guarded_nan(1)
        _raw_step(m, ids, dev(y), logits, loss, sweep_blocks=blocks)
        torch.cuda.synchronize()
        assert guards_intact(gl) and guards_intact(gs)
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss).all())
        results.append((m.t_rec.clone(), m.lin_state.clone(), m.dense.clone(), m.d_s0.clone(), m.d_s1.clone(),
                        logits.clone(), loss.clone()))
        assert bool((m.last_step == 4).all())
    for r in results[1:]:
        for x, z in zip(results[0], r):
            assert torch.equal(x, z)
    # and the engine's own call is that step
    m = _hip_engine(vocab, E, hidden, dropout=0.1, seed=2)
    m.load_state_dict(sd)
    loss, logits = m.fused_train_step(ids, dev(y))
    assert torch.equal(m.t_rec, results[0][0]) and torch.equal(m.dense, results[0][2])
    assert torch.equal(logits, results[0][5]) and torch.equal(loss, results[0][6])


def _snapshot(m):
    return [t.clone() for t in (m.t_rec, m.lin_state, m.dense, m.d_s0, m.d_s1) if t is not None]


@pytest.mark.parametrize("vocab,E,hidden,B,inside", [
    ([3] * 8, 4, [8], 128, True), ([3] * 8, 4, [8], 129, False),                     # B
    ([3] * 32, 4, [8], 16, True), ([3] * 33, 4, [8], 16, False),                     # F
    ([3] * 8, 16, [8], 16, True), ([3] * 8, 20, [8], 16, False),                     # E
    ([3] * 32, 16, [8], 32, True), ([3] * 32, 16, [8], 33, False),                   # B F E = 16384 / 16896
    ([3] * 8, 4, [8, 8, 8], 16, True), ([3] * 8, 4, [8, 8, 8, 8], 16, False),        # hidden layers
    ([3] * 8, 4, [64], 16, True), ([3] * 8, 4, [65], 16, False),                     # width
    ([3] * 32, 16, [64, 64, 64], 32, True), ([3] * 32, 4, [64, 64, 64], 128, True),  # the corners (d_concat in the workspace)
    ([(1 << 18) - 21, 7, 7, 7], 4, [8], 16, True), ([(1 << 18) - 20, 7, 7, 7], 4, [8], 16, False),   # R = 2^18 / 2^18 + 1
])
def test_limits_through_the_entry(vocab, E, hidden, B, inside):
    m = _hip_engine(vocab, E, hidden)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    m.init_variables(g, lin_scale=0.05)
    assert m.fused_step_ok(B) == inside
    rng = np.random.default_rng(3)
    ids = dev(_fresh_ids(rng, vocab, B))
    y = dev((rng.random(B) < 0.3).astype(np.uint8))
    gl, logits = guarded_nan(B)
    gs, loss = guarded_nan(1)
    before = _snapshot(m)
    if inside:
        _raw_step(m, ids, y, logits, loss)
        torch.cuda.synchronize()
        assert guards_intact(gl) and guards_intact(gs) and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss).all())
        assert bool((m.last_step == 1).all())
        # the same step by the layered path, from the same start
        n = _hip_engine(vocab, E, hidden, gemm="fp32")
        n.t_rec.copy_(before[0]); n.lin_state.copy_(before[1]); n.dense.copy_(before[2])
        ln, zn = n.train_step(ids, y)
        n.finalize_rows()
        assert max_err_scaled(logits.cpu().numpy(), zn.cpu().numpy()) < 5e-6 and abs(loss.item() - ln.item()) < 2e-5 * abs(ln.item())
        assert float((m.table - n.table).abs().max()) < 2e-6 and float((m.dense - n.dense).abs().max()) < 2e-6
        assert float((m.lin_w - n.lin_w).abs().max()) < 2e-6
    else:
        with pytest.raises(_lib.MiError, match=r"\(-2\)"):
            _raw_step(m, ids, y, logits, loss)
        torch.cuda.synchronize()
        assert all(torch.equal(x, z) for x, z in zip(before, _snapshot(m)))          # nothing was launched
        assert bool(torch.isnan(logits).all()) and bool((m.last_step == 0).all())
        with pytest.raises(ValueError, match="fused_train_step: the model has"):
            m.fused_train_step(ids, y)


def test_other_refusals_through_the_entry():
    from mi355x_rec.engine import OptimizerSpec
    vocab, E, hidden, B = [9, 13, 5], 4, [8], 16
    m = _hip_engine(vocab, E, hidden)
    rng = np.random.default_rng(3)
    ids, y = dev(_fresh_ids(rng, vocab, B)), dev((rng.random(B) < 0.3).astype(np.uint8))
    logits, loss = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    before = _snapshot(m)
    with pytest.raises(_lib.MiError, match="Adam only"):
        _raw_step(m, ids, y, logits, loss, hp=OptimizerSpec("Adagrad", 0.05).hparams())
    with pytest.raises(_lib.MiError, match="sweep_blocks"):
        _raw_step(m, ids, y, logits, loss, sweep_blocks=1025)
    with pytest.raises(_lib.MiError, match="widths"):
        _raw_step(m, ids[:, :2].contiguous(), y, logits, loss, F=2)
    torch.cuda.synchronize()
    assert all(torch.equal(x, z) for x, z in zip(before, _snapshot(m)))


def test_deep_fm_cli_trains_with_the_fused_step(tmp_path, capsys, monkeypatch):
    """python -m trainers.deep_fm --fused-step on, end to end.  The loss is logged every 10 steps instead of every 100: a
    logged loss is ONE batch of 32 (about +-0.05 around its mean), so "training lowered the loss" is asked of the mean
    of the last five logged losses (160 examples) against the first one (step 10: a model that has barely moved)."""
    from mi355x_rec.engine import DeepFM
    from mi355x_rec.predictor import Predictor
    from trainers import _cli, conf_utils, deep_fm, ml_100k

    def config():
        cfg = conf_utils.get_run_config()
        cfg.log_step_count_steps = 10
        return cfg
    monkeypatch.setattr(_cli, "get_run_config", config)
    opt = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")
    job = str(tmp_path / "job")
    calls = []
    orig = DeepFM.fused_train_step
    DeepFM.fused_train_step = lambda self, ids, y: (calls.append(1), orig(self, ids, y))[1]
    try:
        argv = ["--synthetic", "2000", "--job-dir", job, "--train-steps", "200", "--fused-step", "on"]
        est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(argv))
    finally:
        DeepFM.fused_train_step = orig
    assert est.global_step == 200
    assert 190 <= len(calls) <= 200                          # (the steps whose layer summaries are recorded run layered)
    out = capsys.readouterr().out
    import re
    losses = [float(v) for v in re.findall(r"loss = ([0-9.eE+-]+), step = ", out)]
    print("logged losses:", losses)
    assert len(losses) == 20 and np.isfinite(losses).all()
    assert float(np.mean(losses[-5:])) < losses[0]
    m = est.evaluate(ml_100k.get_input_fn("synthetic:200:2", "eval", 32))
    assert {"accuracy", "auc", "auc_precision_recall", "average_loss", "loss", "precision", "recall", "label/mean",
            "prediction/mean", "accuracy_baseline", "global_step"} <= set(m)
    assert np.isfinite(m["loss"]) and 0.0 <= m["auc"] <= 1.0
    assert os.path.exists(os.path.join(job, "model.ckpt-200.pt"))
    est2 = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(
        ["--synthetic", "2000", "--job-dir", job, "--train-steps", "230", "--fused-step", "off", "--restore"]))
    assert est2.global_step == 230 and "restored" in capsys.readouterr().out
    root = os.path.join(job, "export", "exporter")
    pred = Predictor.from_export(os.path.join(root, sorted(os.listdir(root))[-1]))
    cols, _ = ml_100k._read_csv("synthetic:50:2")
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    res = pred({k: v for k, v in cols.items() if k in recv})
    pr = np.asarray(res["logistic"].cpu() if hasattr(res["logistic"], "cpu") else res["logistic"]).reshape(-1)
    assert pr.shape == (50,) and np.isfinite(pr).all() and (pr > 0).all() and (pr < 1).all()
