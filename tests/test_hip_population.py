"""-m gpu: M small DeepFM models, one training step each, in ONE launch (mi_train_group_step, csrc/train_fused.hip) through
mi355x_rec.population.FusedPopulation and the trainers.sweep CLI.

A member is held to the BITS of its own engine.DeepFM.fused_train_step (torch.equal), and the population to the oracle at
the project's own bars (tests/test_hip_fused_step.py): loss 2e-5 relative, logits 5e-6 on identical
weights and 5e-5 after the first update, every variable 2e-6 absolute (3e-6 for sigmoid / tanh / identity)."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import (MIXED, ML100K_VOCAB, ORACLE_MEMBERS, STATE, _clones, _fresh, _population, _same_state, _spec,
                         _spec_engine)
from tests.util import (_compare_vars, _fresh_ids, dev, dropout_mask, guarded_nan, guards_intact, make_problem,
                        max_err_scaled)

pytestmark = pytest.mark.gpu

def _guarded_step(pop, ids, y, B):
    gs, loss = guarded_nan(len(pop))
    gl, logits = guarded_nan(len(pop), B)
    pop.train_step(ids, y, out=(loss, logits))
    torch.cuda.synchronize()
    assert guards_intact(gs) and guards_intact(gl)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(logits).all())
    return loss, logits


@pytest.mark.parametrize("M", [1, 3, 64])
def test_bits_of_the_solo_step(M):
    B = 32
    specs = [MIXED[i % len(MIXED)] for i in range(M)]
    group, sds = _fresh(specs)
    solo = _clones(specs, sds)
    pop = _population(group)
    rng = np.random.default_rng(M)
    for step in range(4):
        ids = dev(_fresh_ids(rng, ML100K_VOCAB, B))
        y = dev((rng.random(B) < 0.3).astype(np.uint8))
        loss, logits = _guarded_step(pop, ids, y, B)
        for i, s in enumerate(solo):
            ls, zs = s.fused_train_step(ids, y)
            assert torch.equal(ls, loss[i:i + 1]) and torch.equal(zs, logits[i]), (step, i, specs[i])
            assert _same_state(group[i], s) is None, (step, i, specs[i], _same_state(group[i], s))
            assert group[i].step == s.step == step + 1 and group[i]._final_step == step + 1
            assert bool((group[i].last_step == step + 1).all())


def test_bits_do_not_depend_on_neighbours_position_or_sweep_grid():
    B, M = 32, 8
    specs = [MIXED[i] for i in (0, 1, 2, 5, 11, 15, 18, 20)]
    first, sds = _fresh(specs)
    rng = np.random.default_rng(8)
    batches = [(dev(np.stack([_fresh_ids(rng, ML100K_VOCAB, B) for _ in range(M)])),
                dev((rng.random((M, B)) < 0.3).astype(np.uint8))) for _ in range(3)]
    want = []
    for i, s in enumerate(first):                                     # each member alone, on its own batches
        outs = [tuple(t.clone() for t in s.fused_train_step(ids[i].contiguous(), y[i].contiguous())) for ids, y in batches]
        want.append(outs)
    order = list(range(M))
    for blocks, members in ((0, order), (1, order), (7, order[::-1]), (64, order), (0, order[::-1]), (7, [3, 1, 6])):
        group = _clones([specs[i] for i in members], [sds[i] for i in members])
        pop = _population(group, blocks)
        for step, (ids, y) in enumerate(batches):
            idx = torch.tensor(members, device="cuda")
            loss, logits = _guarded_step(pop, ids[idx].contiguous(), y[idx].contiguous(), B)
            for j, i in enumerate(members):
                assert torch.equal(loss[j:j + 1], want[i][step][0]) and torch.equal(logits[j], want[i][step][1]), (blocks, i)
        for j, i in enumerate(members):
            assert _same_state(group[j], first[i]) is None, (blocks, members, i)


# two more without the margin, as the existing dropout and activation tests: (seed, E, hidden, lr, engine keywords)
ORACLE_EXTRA = [(306, 4, [16, 16], 0.001, dict(dropout=0.25, seed=7)), (307, 8, [32], 0.001, dict(activation="tanh"))]


def test_members_match_the_oracle():
    B = 32
    y = make_problem(300, ML100K_VOCAB, 4, [16, 16], B)[3]
    members = [m + ({},) for m in ORACLE_MEMBERS] + ORACLE_EXTRA
    engines, params, states = [], [], []
    for seed, E, hidden, lr, kw in members:
        p = make_problem(seed, ML100K_VOCAB, E, hidden, B)[0]
        m = _spec_engine(_spec(E, hidden, lr, **kw))
        m.load_oracle_params(p)
        engines.append(m)
        params.append(p)
        states.append(O.TrainState(p, OO.Hyper("Adam", lr)))
    pop = _population(engines)
    rng = np.random.default_rng(300)
    margins = [np.inf] * len(ORACLE_MEMBERS)
    for step in range(5):
        ids = _fresh_ids(rng, ML100K_VOCAB, B)
        want = []
        for i, (seed, E, hidden, lr, kw) in enumerate(members):
            m, p = engines[i], params[i]
            okw = {}
            if kw.get("dropout"):
                keep = 1.0 - kw["dropout"]
                okw = dict(dropout_masks=[dropout_mask(m._layer_seed(j), B, h, keep) for j, h in enumerate(hidden)], keep_prob=keep)
            if "activation" in kw:
                okw["activation"] = kw["activation"]
            if i < len(ORACLE_MEMBERS):
                margins[i] = min(margins[i], min(float(np.abs(q).min()) for q in O.forward(p, ids)["pre"]))
            want.append(O.train_step(p, states[i], ids, y, **okw))
        loss, logits = pop.train_step(dev(ids), dev(y))
        loss, logits = loss.cpu().numpy(), logits.cpu().numpy()
        for i, (lo, zo) in enumerate(want):
            le = abs(float(loss[i]) - float(lo)) / abs(float(lo))
            ge = max_err_scaled(logits[i], zo)
            print("step %d member %d: loss err %.2e, logits err %.2e" % (step, i, le, ge))
            assert le < 2e-5, (step, i)
            assert ge < (5e-6 if step == 0 else 5e-5), (step, i)
    print("margins:", margins)
    assert min(margins) >= 1e-6, margins
    for i, (m, p) in enumerate(zip(engines, params)):
        assert m.step == 5 and bool((m.last_step == 5).all())
        _compare_vars(m, p, 3e-6 if members[i][4].get("activation") == "tanh" else 2e-6)


def test_a_schedule_table_that_moves():
    from mi355x_rec.engine import AdamSchedule
    B = 32
    specs = [MIXED[0], MIXED[16], MIXED[2]]
    group, sds = _fresh(specs)
    solo = _clones(specs, sds)
    group[1].sched = AdamSchedule(group[1].opt, group[1].device, capacity=4)
    pop = _population(group)
    rng = np.random.default_rng(12)
    gens = []
    for step in range(12):
        ids = dev(_fresh_ids(rng, ML100K_VOCAB, B))
        y = dev((rng.random(B) < 0.3).astype(np.uint8))
        loss, logits = _guarded_step(pop, ids, y, B)
        gens.append(group[1].sched.gen)
        for i, s in enumerate(solo):
            ls, zs = s.fused_train_step(ids, y)
            assert torch.equal(ls, loss[i:i + 1]) and torch.equal(zs, logits[i]), (step, i)
            assert _same_state(group[i], s) is None, (step, i)
    assert gens == [1] * 4 + [2] * 6 + [3] * 2                        # (the table was extended, and moved, at steps 5 and 11)


def test_living_with_the_rest_of_the_engine():
    B = 32
    specs = [_spec(gemm="fp32"), MIXED[15], MIXED[3]]                  # (member 0's layered step: exact fp32 products, as the fused step's)
    group, sds = _fresh(specs)
    solo = _clones(specs, sds)
    pop = _population(group)
    rng = np.random.default_rng(5)
    batch = lambda: (dev(_fresh_ids(rng, ML100K_VOCAB, B)), dev((rng.random(B) < 0.3).astype(np.uint8)))

    def together(ids, y):
        loss, logits = pop.train_step(ids, y)
        return [tuple(t.clone() for t in s.fused_train_step(ids, y)) for s in solo], loss, logits
    ids, y = batch()
    together(ids, y)
    group[0].timers = {}
    group[0].finalize_rows()                                          # nothing is owed after a population step
    assert group[0].timers == {}
    group[0].timers = None
    ids, y = batch()
    group[0].train_step(ids, y)                                       # member 0 on its own, by the layered step
    with pytest.raises(ValueError, match="member 1 is at step 1, member 0 at step 2"):
        pop.train_step(ids, y)
    assert [m.step for m in group] == [2, 1, 1]
    for m in group[1:]:
        m.fused_train_step(ids, y)
    for s in solo:
        s.fused_train_step(ids, y)
    assert _same_state(group[1], solo[1]) is None and _same_state(group[2], solo[2]) is None
    assert group[0].step == 2                                         # (its layered step left rows owing their sweep)
    ids, y = batch()
    want, loss, logits = together(ids, y)                             # (the population settles member 0's owed rows first)
    assert all(m.step == 3 and m._final_step == 3 and bool((m.last_step == 3).all()) for m in group)
    # member 0 took one layered step where its clone took a fused one: the project's bars between the two
    assert float((group[0].table - solo[0].table).abs().max()) < 2e-6 and float((group[0].dense - solo[0].dense).abs().max()) < 2e-6
    assert float((group[0].lin_w - solo[0].lin_w).abs().max()) < 2e-6
    for i in (1, 2):
        assert torch.equal(loss[i:i + 1], want[i][0]) and torch.equal(logits[i], want[i][1]) and _same_state(group[i], solo[i]) is None
    # state_dict -> load_state_dict into fresh engines -> population step: the bits of the uninterrupted population
    restored = _clones(specs, [m.state_dict() for m in group])
    pop2 = _population(restored)
    ids, y = batch()
    la, za = pop.train_step(ids, y)
    lb, zb = pop2.train_step(ids, y)
    assert torch.equal(la, lb) and torch.equal(za, zb)
    for a, b in zip(group, restored):
        assert _same_state(a, b) is None and a.step == b.step == 4
    # a member alone afterwards: evaluation and its own fused step
    _, z = group[1].loss(ids, y)
    assert bool(torch.isfinite(z).all())
    group[1].fused_train_step(ids, y)
    restored[1].fused_train_step(ids, y)
    assert _same_state(group[1], restored[1]) is None


def _snapshot(engines):
    return [getattr(m, n).clone() for m in engines for n in STATE if getattr(m, n) is not None]


def _plan_call(k, pop, engines, B, n=None, edit=None):
    """mi_train_group_plan through the binding as FusedPopulation calls it; edit(members) changes the descriptions first"""
    keep = []
    members = (_lib.FusedMember * len(engines))(*[pop._describe(e, B, keep) for e in engines])
    if edit:
        edit(members)
    n = len(engines) if n is None else n
    table = torch.full((max(int(k.query("mi_train_group_plan_bytes", max(n, 1))), 16),), 0xA5, dtype=torch.uint8, device="cuda")
    plan = _lib.FusedGroupPlan()
    try:
        k.mi_train_group_plan(members, n, B, engines[0].F, engines[0].field_off, table, table.numel(), plan)
    finally:
        torch.cuda.synchronize()
        plan.keep = keep
    return plan, table


OUTSIDE = [  # test_limits_through_the_entry's "outside" rows: (vocab, E, hidden, B, E and hidden of a member INSIDE, index refused)
    ([3] * 8, 4, [8], 129, None, 0), ([3] * 33, 4, [8], 16, None, 0), ([3] * 8, 20, [8], 16, (4, [8]), 1),
    ([3] * 32, 16, [8], 33, None, 0), ([3] * 8, 4, [8, 8, 8, 8], 16, (4, [8]), 1), ([3] * 8, 4, [65], 16, (4, [8]), 1),
    ([(1 << 18) - 20, 7, 7, 7], 4, [8], 16, None, 0),
]


@pytest.mark.parametrize("vocab,E,hidden,B,inside,who", OUTSIDE)
def test_members_over_a_limit_are_refused_through_the_entry(vocab, E, hidden, B, inside, who):
    good = _spec_engine(_spec(*(inside or (4, [8]))), [3] * 8 if inside is None else vocab)
    bad = _spec_engine(_spec(E, hidden), vocab)
    engines = [good, bad] if inside else [bad, _spec_engine(_spec(E, hidden), vocab)]
    pop = _population([good])
    before = _snapshot(engines)
    with pytest.raises(_lib.MiError, match=r"\(-2\): train_group_plan: member %d: train_step_fused: " % who):
        plan, table = _plan_call(good.k, pop, engines, B)
    torch.cuda.synchronize()
    assert all(torch.equal(x, z) for x, z in zip(before, _snapshot(engines)))
    if inside:
        from mi355x_rec.population import FusedPopulation
        with pytest.raises(ValueError, match="member 1: the model has"):
            FusedPopulation(engines)


def test_other_refusals_through_the_entry():
    from mi355x_rec.engine import OptimizerSpec
    vocab, B = [9, 13, 5], 16
    engines = [_spec_engine(_spec(4, [8]), vocab) for _ in range(3)]
    k = engines[0].k
    pop = _population(engines)
    rng = np.random.default_rng(3)
    ids, y = dev(_fresh_ids(rng, vocab, B)), dev((rng.random(B) < 0.3).astype(np.uint8))
    before = _snapshot(engines)
    gs, loss = guarded_nan(3)
    gl, logits = guarded_nan(3, B)

    def refused(match, **kw):
        plan = _lib.FusedGroupPlan()
        with pytest.raises(_lib.MiError, match=match):
            plan, table = _plan_call(k, pop, engines, B, **kw)
        return plan

    def adagrad(ms):
        ms[1].hp = OptimizerSpec("Adagrad", 0.05).hparams()

    def shared(ms):
        ms[2].table = ms[0].table
    refused(r"\(-2\): train_group_plan: member 1: train_step_fused: optimizer kind \d+ \(Adam only\)", edit=adagrad)
    refused(r"\(-1\): train_group_plan: member 0 and member 2 share", edit=shared)
    refused(r"\(-1\): train_group_plan: 0 members", n=0)
    plan = refused(r"\(-2\): train_group_plan: %d members \(at most %d" % (_lib.FUSED_GROUP_MAX_MEMBERS + 1, _lib.FUSED_GROUP_MAX_MEMBERS),
                   n=_lib.FUSED_GROUP_MAX_MEMBERS + 1)
    with pytest.raises(_lib.MiError, match=r"\(-1\): train_group_step: plan"):       # a plan no call has written
        k.mi_train_group_step(plan, 3, ids, 0, y, 0, B, 1, logits, loss, 0)
    plan, table = _plan_call(k, pop, engines, B)
    for match, args in ((r"3 members|2 members", (2, ids, 0, y, 0, B, 1, logits, loss, 0)),
                        (r"B=8", (3, ids, 0, y, 0, 8, 1, logits, loss, 0)),
                        (r"step=0", (3, ids, 0, y, 0, B, 0, logits, loss, 0)),
                        (r"lr_table", (3, ids, 0, y, 0, B, 1 << 20, logits, loss, 0)),
                        (r"ids_member_stride", (3, ids, 7, y, 0, B, 1, logits, loss, 0)),
                        (r"labels_member_stride", (3, ids, 0, y, 3, B, 1, logits, loss, 0)),
                        (r"\(-2\): train_group_step: sweep_blocks", (3, ids, 0, y, 0, B, 1, logits, loss, 1025)),
                        (r"ids / labels / logits / loss", (3, ids, 0, y, 0, B, 1, None, loss, 0))):
        with pytest.raises(_lib.MiError, match=match):
            k.mi_train_group_step(plan, *args)
    torch.cuda.synchronize()
    assert all(torch.equal(x, z) for x, z in zip(before, _snapshot(engines)))
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all()) and guards_intact(gs) and guards_intact(gl)
    assert all(bool((m.last_step == 0).all()) for m in engines)
    k.mi_train_group_step(plan, 3, ids, 0, y, 0, B, 1, logits, loss, 0)              # and the plan does work
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and all(bool((m.last_step == 1).all()) for m in engines)


# ---- the grid-search CLI ----------------------------------------------------------------------------------------------
_DEEP_FM_OPT = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")


def test_sweep_cli_trains_a_grid(tmp_path, capsys, monkeypatch):
    """python -m trainers.sweep end to end.  As in test_hip_fused_step's CLI test the loss is logged every 10 steps, and
    "training lowered the loss" is asked of the mean of a member's last five logged losses against its first."""
    import json
    import os
    from mi355x_rec.predictor import Predictor
    from trainers import _cli, conf_utils, deep_fm, ml_100k, sweep

    def config():
        cfg = conf_utils.get_run_config()
        cfg.log_step_count_steps = 10
        return cfg
    monkeypatch.setattr(_cli, "get_run_config", config)
    job = str(tmp_path / "job")
    grid = ["--learning-rate", "0.001", "0.01", "--dropout", "0", "0.1"]
    members = sweep.train_and_evaluate(sweep.make_parser().parse_args(["--synthetic", "2000", "--job-dir", job, "--train-steps", "200"] + grid))
    assert len(members) == 4 and all(m.global_step == 200 for m in members)
    rows = json.load(open(os.path.join(job, "sweep.json")))["members"]
    assert len(rows) == 4 and sorted(r["member"] for r in rows) == [0, 1, 2, 3]
    aucs = [r["metrics"]["auc"] for r in rows]
    assert aucs == sorted(aucs, reverse=True)
    for r in rows:
        assert np.isfinite(list(r["metrics"].values())).all() and 0.0 <= r["metrics"]["auc"] <= 1.0
        assert os.path.exists(os.path.join(job, "member_%d" % r["member"], "model.ckpt-200.pt"))
    log = [json.loads(line) for line in open(os.path.join(job, "sweep_log.jsonl"))]
    assert [rec["global_step"] for rec in log] == list(range(10, 201, 10))
    for i in range(4):
        losses = [rec["loss"][i] for rec in log]
        print("member %d logged losses:" % i, losses)
        assert np.isfinite(losses).all() and float(np.mean(losses[-5:])) < losses[0], i
    assert "member loss lowest = " in capsys.readouterr().out
    # --restore: all four members to 230, each at its own rate
    again = sweep.train_and_evaluate(sweep.make_parser().parse_args(
        ["--synthetic", "2000", "--job-dir", job, "--train-steps", "230", "--restore"] + grid))
    assert all(m.global_step == 230 for m in again) and [m._engine().opt.lr for m in again] == [0.001, 0.01, 0.001, 0.01]
    assert "restored" in capsys.readouterr().out
    # a member is an ordinary job directory: trainers.deep_fm --restore carries member 2 (learning rate 0.001) on
    by = {r["member"]: r for r in json.load(open(os.path.join(job, "sweep.json")))["members"]}
    assert by[2]["params"]["learning_rate"] == 0.001 and by[2]["params"]["dropout"] == 0.1
    est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", _DEEP_FM_OPT).parse_args(
        ["--synthetic", "2000", "--job-dir", os.path.join(job, "member_2"), "--dropout", "0.1", "--train-steps", "260", "--restore"]))
    assert est.global_step == 260
    with pytest.raises(ValueError, match="different steps"):
        sweep.train_and_evaluate(sweep.make_parser().parse_args(
            ["--synthetic", "2000", "--job-dir", job, "--train-steps", "300", "--restore"] + grid))
    pred = Predictor.from_export(by[1]["export"])
    cols, _ = ml_100k._read_csv("synthetic:50:2")
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    res = pred({k: v for k, v in cols.items() if k in recv})
    pr = np.asarray(res["logistic"].cpu() if hasattr(res["logistic"], "cpu") else res["logistic"]).reshape(-1)
    assert pr.shape == (50,) and np.isfinite(pr).all() and (pr > 0).all() and (pr < 1).all()


def test_a_sweep_member_is_a_stand_alone_run(tmp_path):
    from mi355x_rec.estimator import Estimator
    from trainers import _cli, deep_fm, ml_100k, sweep
    args = sweep.make_parser().parse_args(["--job-dir", str(tmp_path / "job"), "--learning-rate", "0.001", "0.01"])
    config = _cli.get_run_config()
    hps = sweep.grid(args)
    assert len(hps) == 2
    members = sweep.make_members(args, hps, config)
    sweep.train(members, ml_100k.get_input_fn("synthetic:2000:1", batch_size=32, seed=7), 40, config)
    for i, hp in enumerate(hps):
        params = {"categorical_columns": ml_100k.get_feature_columns(hp["embedding_size"])["linear"], "fused_step": "on", **hp}
        alone = Estimator(deep_fm.model_fn, model_dir=str(tmp_path / ("alone_%d" % i)), config=config, params=params)
        alone.train(ml_100k.get_input_fn("synthetic:2000:1", batch_size=32, seed=7), max_steps=40)
        a, b = members[i]._engine().state_dict(), alone._engine().state_dict()
        assert a["step"] == b["step"] == 40 and set(a) == set(b)
        for key, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, b[key]), (i, key)
