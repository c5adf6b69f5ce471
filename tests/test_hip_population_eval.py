"""-m gpu: a whole evaluation set, for every member of a population, in ONE launch (mi_eval_group, eval_fused_group_k in
csrc/train_fused.hip) through the entry itself, mi355x_rec.population.FusedPopulation.evaluate and trainers.sweep
--eval-every / --final-eval fused.

A member's tile is held to the BITS of its own dropout-free fused step on that tile alone (torch.equal), the counters to
mi_eval_accumulate on those logits (integers exactly, the fp64 sums to the reordering of fp64 additions), and the
population to the fp64 oracle at the fused step's own bar: logits 5e-6 on identical weights, scaled as max_err_scaled.
The metrics are compared with oracle/metrics.py on the oracle's logits; an example can only be counted differently when its
sigmoid lies within that bar / 4 (sigmoid' <= 1/4) plus one fp32 ulp of a threshold, which the test counts with the oracle
alone (n_near) and caps at N / 100."""
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from oracle import deepfm as O
from oracle.metrics import BinaryMetrics, auc_thresholds
from tests.cases import (MIXED, ML100K_VOCAB, ORACLE_MEMBERS, STATE, _clones, _fresh, _population, _same_state, _spec,
                         _spec_engine)
from tests.util import GUARD, _fresh_ids, dev, guarded_nan, guards_intact, make_problem, max_err_scaled

pytestmark = pytest.mark.gpu

N_EVAL = 1000
E4 = [i for i, s in enumerate(MIXED) if s["E"] == 4]          # the members a batch of 128 examples fits (B F E <= 16384)
PATTERN = -0x5A5A5A5A5A5A5A5B


def _eval_set(seed, N=N_EVAL):
    rng = np.random.default_rng(seed)
    return dev(_fresh_ids(rng, ML100K_VOCAB, N)), dev((rng.random(N) < 0.3).astype(np.uint8))


def _trained(specs, steps=2, B=32, seed=0):
    """engines of `specs` after `steps` population steps (slots, stamps and the step counter are no longer at their start)"""
    group, _ = _fresh(specs)
    pop = _population(group)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        pop.train_step(dev(_fresh_ids(rng, ML100K_VOCAB, B)), dev((rng.random(B) < 0.3).astype(np.uint8)))
    return group, pop


def _guarded_i64(n):
    buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int64, device="cuda")
    buf[GUARD:GUARD + n] = 0
    return buf, buf[GUARD:GUARD + n]


def _i64_guards_intact(buf):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())


def _raw_eval(pop, ids, y, B, blocks=0, with_logits=True):
    """mi_eval_group through the binding, as FusedPopulation.evaluate calls it, into guarded outputs: (logits [M, N] or None,
    batch_loss [M, T], hist [M, 2, 201], counts [M, 8], partials [M, T, 3])"""
    M, N = len(pop), int(ids.shape[0])
    T = -(-N // B)
    plan = pop._plan_for(B)
    tail = torch.tensor([float(np.float32(1.0 / (N % B))) if (N % B and e.reduction == "mean") else 1.0 for e in pop.engines],
                        dtype=torch.float32, device="cuda")
    gz, logits = guarded_nan(M, N) if with_logits else (None, None)
    gl, loss = guarded_nan(M, T)
    gh, hist = _guarded_i64(M * 402)
    gc, counts = _guarded_i64(M * 8)
    gp = torch.full((M * T * 3 + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    partials = gp[GUARD:GUARD + M * T * 3]
    pop.k.mi_eval_group(plan[1], M, ids, y, N, tail, logits, loss, hist, counts, partials, blocks)
    torch.cuda.synchronize()
    assert guards_intact(gl) and (gz is None or guards_intact(gz)) and _i64_guards_intact(gh) and _i64_guards_intact(gc)
    assert bool(torch.isnan(gp[:GUARD]).all()) and bool(torch.isnan(gp[-GUARD:]).all())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(partials).all()) and (logits is None or bool(torch.isfinite(logits).all()))
    assert bool((counts.view(M, 8)[:, 7] == 0).all())
    return logits, loss, hist.view(M, 2, 201), counts.view(M, 8), partials.view(M, T, 3)


def _same(a, b):
    return all((x is None and z is None) or torch.equal(x, z) for x, z in zip(a, b))


def _snap(m):
    return {n: getattr(m, n).clone() for n in STATE if getattr(m, n) is not None}


def _rewind(m, snap, step):
    for n, t in snap.items():
        getattr(m, n).copy_(t)
    m.step = m._final_step = step


def _no_dropout(spec):
    return dict(spec, kw=dict(spec["kw"], dropout=0.0))


@pytest.mark.parametrize("B,which", [(32, list(range(len(MIXED)))), (128, E4)])
def test_every_tile_has_the_bits_of_the_members_own_dropout_free_step(B, which):
    specs = [MIXED[i] for i in which]
    assert any(s["kw"].get("dropout", 0) > 0 for s in specs) and any(s["kw"].get("reduction") == "sum" for s in specs)
    group, pop = _trained(specs)
    ids, y = _eval_set(B)
    N, T = N_EVAL, -(-N_EVAL // B)
    assert N % B != 0                                                  # (the short last tile is one of the tiles)
    logits, loss, hist, counts, partials = _raw_eval(pop, ids, y, B)
    clones = _clones([_no_dropout(s) for s in specs], [m.state_dict() for m in group])
    for i, c in enumerate(clones):
        assert c.dropout == 0 and c.step == 2
        snap = _snap(c)
        for t in range(T):
            lo, hi = t * B, min(N, (t + 1) * B)
            ls, zs = c.fused_train_step(ids[lo:hi].contiguous(), y[lo:hi].contiguous())
            assert torch.equal(zs, logits[i, lo:hi]), (i, t, specs[i])
            assert torch.equal(ls, loss[i, t:t + 1]), (i, t, specs[i], ls.item(), loss[i, t].item())
            _rewind(c, snap, 2)
    # the counters: exactly mi_eval_accumulate's on those logits; the fp64 sums differ from its by the order of additions only
    for i in range(len(specs)):
        h = torch.zeros(2, 201, dtype=torch.int64, device="cuda")
        c = torch.zeros(8, dtype=torch.int64, device="cuda")
        s = torch.zeros(4, dtype=torch.float64, device="cuda")
        pop.k.mi_eval_accumulate(logits[i].contiguous(), y, N, h, c, s)
        assert torch.equal(h, hist[i]) and torch.equal(c, counts[i]), (i, specs[i])
        assert int(counts[i, 0]) == N and int(hist[i].sum()) == N
        z = logits[i].double().cpu().numpy()
        yy = y.cpu().numpy().astype(np.float64)
        terms = (np.maximum(z, 0) - z * yy + np.log1p(np.exp(-np.abs(z))), 1 / (1 + np.exp(-z)), yy)
        got = np.cumsum(partials[i].cpu().numpy(), 0)[-1]
        for j in range(3):
            bound = N * 2.0 ** -52 * float(np.abs(terms[j]).sum())
            print("member %d sum %d: %.17g against %.17g (bound %.3g)" % (i, j, got[j], s[j].item(), bound))
            assert abs(got[j] - s[j].item()) <= bound, (i, j)


def test_bits_do_not_depend_on_the_grid_the_call_or_the_neighbours():
    B, M = 32, 64
    specs = [MIXED[i % len(MIXED)] for i in range(M)]
    group, pop = _trained(specs)
    ids, y = _eval_set(7)
    want = _raw_eval(pop, ids, y, B)
    for blocks in (1, 7, 0, 1024):                                       # (0 again: a second call; 1024: more workgroups than tiles)
        assert _same(want, _raw_eval(pop, ids, y, B, blocks)), blocks
    got = _raw_eval(pop, ids, y, B, with_logits=False)                   # the hot path writes no logits
    assert got[0] is None and _same(want[1:], got[1:])
    sds = [m.state_dict() for m in group]
    for members in ([0], [0, 1, 2], [5, 40, 13]):
        small = _population(_clones([specs[i] for i in members], [sds[i] for i in members]))
        idx = torch.tensor(members, device="cuda")
        for blocks in (0, 3):
            got = _raw_eval(small, ids, y, B, blocks)
            assert _same([t[idx] for t in want], got), (members, blocks)


def test_evaluation_writes_nothing_and_training_carries_on_with_the_same_bits():
    B = 32
    specs = [MIXED[i] for i in (0, 1, 5, 13, 14, 19, 20, 21)]
    a, pop_a = _trained(specs)
    b = _clones(specs, [m.state_dict() for m in a])
    pop_b = _population(b)
    ids, y = _eval_set(3)
    before = [_snap(m) for m in a]
    plans = len(pop_a._plans)
    out = pop_a.evaluate(ids, y)                                         # (batch_size None: the training step's)
    torch.cuda.synchronize()
    assert len(out) == len(specs) and len(pop_a._plans) == plans
    for m, s in zip(a, before):
        assert all(torch.equal(getattr(m, n), t) for n, t in s.items())
        assert m.step == 2 and m._final_step == 2
    rng = np.random.default_rng(9)
    for _ in range(2):
        bi, by = dev(_fresh_ids(rng, ML100K_VOCAB, B)), dev((rng.random(B) < 0.3).astype(np.uint8))
        la, za = pop_a.train_step(bi, by)
        lb, zb = pop_b.train_step(bi, by)
        assert torch.equal(la, lb) and torch.equal(za, zb)
        for x, z in zip(a, b):
            assert _same_state(x, z) is None
        pop_a.evaluate(ids, y)
    assert len(pop_a._plans) == plans


def test_evaluate_is_the_host_finish_of_the_raw_results():
    from mi355x_rec.metrics import metrics_from_counters
    B = 32
    specs = [MIXED[i] for i in (0, 13, 19)]
    group, pop = _trained(specs)
    ids, y = _eval_set(11)
    logits, loss, hist, counts, partials = _raw_eval(pop, ids, y, B)
    for blocks in (0, 5):
        pop.EVAL_BLOCKS = blocks
        out, z = pop.evaluate(ids, y, batch_size=B, return_logits=True)
        assert torch.equal(z, logits)
        raw = pop.eval_out
        assert np.array_equal(raw["hist"], hist.cpu().numpy()) and np.array_equal(raw["counts"], counts.cpu().numpy())
        assert np.array_equal(raw["partials"], partials.cpu().numpy()) and np.array_equal(raw["batch_loss"], loss.cpu().numpy())
        for i in range(len(specs)):
            sums = np.zeros(3)
            for t in range(partials.shape[1]):
                sums = sums + raw["partials"][i, t]
            want = metrics_from_counters(raw["hist"][i], raw["counts"][i], sums)
            want["loss"] = float(raw["batch_loss"][i].astype(np.float64).sum() / partials.shape[1])
            assert set(out[i]) == set(want)
            for k, v in want.items():
                assert out[i][k] == pytest.approx(v, rel=1e-14, abs=0), (i, k)
    # what Estimator.evaluate's loop gives for a member: the layered eng.loss per batch, then mi_eval_accumulate
    m = group[0]
    h = torch.zeros(2, 201, dtype=torch.int64, device="cuda")
    c = torch.zeros(8, dtype=torch.int64, device="cuda")
    s = torch.zeros(4, dtype=torch.float64, device="cuda")
    bl = []
    for lo in range(0, N_EVAL, B):
        l, z = m.loss(ids[lo:lo + B].contiguous(), y[lo:lo + B].contiguous())
        m.k.mi_eval_accumulate(z, y[lo:lo + B].contiguous(), z.shape[0], h, c, s)
        bl.append(l.clone())
    layered = metrics_from_counters(h.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy())
    print("layered:", layered, "fused:", out[0])
    assert abs(float(torch.stack(bl).double().mean()) - out[0]["loss"]) < 2e-5 * out[0]["loss"]
    assert abs(layered["average_loss"] - out[0]["average_loss"]) < 2e-5 * out[0]["average_loss"]
    assert abs(layered["auc"] - out[0]["auc"]) < 2e-3 and abs(layered["accuracy"] - out[0]["accuracy"]) <= 2 / N_EVAL


# ---- the oracle ---------------------------------------------------------------------------------------------------------
BAR = 5e-6          # the fused step's logits bar on identical weights (test_hip_fused_step.py), scaled as max_err_scaled
ULP32 = 2.0 ** -23  # one fp32 ulp at 1, the largest a sigmoid's can be
# make_problem's embeddings (truncated normal, 1 / sqrt(E)) over 26 fields give logits up to +-30: such a sigmoid sits within
# 1e-7 of tf.metrics.auc's outermost thresholds (-1e-7 and 1 + 1e-7), counts as "near" one by the definition above and can
# never cross it.  Scaled down, the logits stay inside +-6 and n_near counts the examples that can really change sides.
EMB_SCALE = 0.35


def _oracle_side(seed_ids):
    """Everything the oracle alone decides, on the CPU: per member the fp64 logits, the metrics of oracle/metrics.py on them,
    and the examples a result within the bar may count differently."""
    rng = np.random.default_rng(seed_ids)
    ids = _fresh_ids(rng, ML100K_VOCAB, N_EVAL)
    y = (rng.random(N_EVAL) < 0.3).astype(np.uint8)
    th = np.concatenate([auc_thresholds().astype(np.float64), [0.5]])
    out = []
    for seed, E, hidden, lr in ORACLE_MEMBERS:
        p = make_problem(seed, ML100K_VOCAB, E, hidden, 32)[0]
        for a in p.emb:
            a *= np.float32(EMB_SCALE)
        z = O.forward(p.astype(np.float64), ids)["logits"]
        dz = BAR * np.maximum(np.abs(z), np.sqrt(np.mean(z * z)))      # what max_err_scaled < BAR allows each logit
        tol = dz / 4 + ULP32
        sig = 1 / (1 + np.exp(-z))
        dist = np.abs(sig[:, None] - th[None, :])
        near = dist.min(1) <= tol
        near_th = dist[:, :200].min(1) <= tol                           # near one of the 200 (0.5 is none of them)
        j_near = dist[:, :200].argmin(1)                                # the threshold such an example may change sides of
        bm = BinaryMetrics()
        bm.update(z, y)
        out.append(dict(p=p, z=z, dz=dz, tol=tol, near=near, near_th=near_th, near5=dist[:, 200] <= tol, j_near=j_near, bm=bm, lr=lr, E=E, hidden=hidden))
    return ids, y, out


def _hist_of(bm):
    """hist [2, 201] of a BinaryMetrics: hist[y, k] = examples of label y above exactly k thresholds"""
    h = np.zeros((2, 201), np.int64)
    for row, pos, tot in ((1, bm.tp, bm.tp[0] + bm.fn[0]), (0, bm.fp, bm.fp[0] + bm.tn[0])):
        h[row, 0] = tot - pos[0]
        h[row, 1:200] = pos[:-1] - pos[1:]
        h[row, 200] = pos[-1]
    return h


def _auc_interval(tp, fp, P, Nn, ctp, cfp, curve):
    """interval arithmetic over metrics._auc's formula with tp[j] in tp[j] -+ ctp[j] and fp[j] in fp[j] -+ cfp[j]"""
    eps = 1.0e-6
    tl, th_, fl, fh = np.maximum(tp - ctp, 0.0), np.minimum(tp + ctp, P), np.maximum(fp - cfp, 0.0), np.minimum(fp + cfp, Nn)
    rl, rh = tl / (P + eps), th_ / (P + eps)
    if curve == "ROC":
        xl, xh, yl, yh = fl / (Nn + eps), fh / (Nn + eps), rl, rh
    else:
        xl, xh, yl, yh = rl, rh, (tl + eps) / (tl + fh + eps), (th_ + eps) / (th_ + fl + eps)
    dl, dh = xl[:-1] - xh[1:], xh[:-1] - xl[1:]
    sl, sh = yl[:-1] + yl[1:], yh[:-1] + yh[1:]
    lo = np.minimum(dl * sl, dl * sh) / 2
    hi = np.maximum(dh * sl, dh * sh) / 2
    return float(lo.sum()), float(hi.sum())


def test_the_cap_on_examples_near_a_threshold_holds_for_the_chosen_seed():
    """(the oracle alone; here so that the cap below cannot hide a failure)"""
    _, _, side = _oracle_side(301)
    n_near = [int(s["near"].sum()) for s in side]
    print("n_near per member:", n_near)
    assert max(n_near) <= N_EVAL // 100, n_near


def test_logits_and_metrics_match_the_oracle():
    B = 32
    ids, y, side = _oracle_side(301)
    engines = []
    for s in side:
        m = _spec_engine(_spec(s["E"], s["hidden"], s["lr"]))
        m.load_oracle_params(s["p"])
        engines.append(m)
    pop = _population(engines)
    out, logits = pop.evaluate(dev(ids), dev(y), batch_size=B, return_logits=True)
    raw = pop.eval_out
    logits = logits.cpu().numpy()
    T = -(-N_EVAL // B)
    for i, s in enumerate(side):
        err = max_err_scaled(logits[i], s["z"])
        n_near = int(s["near"].sum())
        print("member %d: logits err %.2e, n_near %d" % (i, err, n_near))
        assert n_near <= N_EVAL // 100, (i, n_near)
        assert err < BAR, (i, err)
        bm, want = s["bm"], s["bm"].result()
        ho = _hist_of(bm)
        diff = int(np.abs(raw["hist"][i] - ho).sum())
        print("member %d: sum |hist - hist_oracle| = %d (allowed %d)" % (i, diff, 2 * n_near))
        assert diff <= 2 * n_near, (i, diff, n_near)
        got = out[i]
        assert got["label/mean"] == want["label/mean"] and got["accuracy_baseline"] == want["accuracy_baseline"]
        n5 = int(s["near5"].sum())
        assert abs(got["accuracy"] - want["accuracy"]) <= n5 / N_EVAL + 1e-15, i
        for key, a, b_ in (("precision", bm.tp5, bm.fp5), ("recall", bm.tp5, bm.fn5)):
            lo = max(a - n5, 0) / max(max(a - n5, 0) + b_ + n5, 1)
            hi = (a + n5) / max(a + n5 + max(b_ - n5, 0), 1)
            assert lo - 1e-15 <= got[key] <= hi + 1e-15, (i, key, lo, got[key], hi)
        yb = y.astype(bool)
        ctp, cfp = np.zeros(200), np.zeros(200)
        np.add.at(ctp, s["j_near"][s["near_th"] & yb], 1)
        np.add.at(cfp, s["j_near"][s["near_th"] & ~yb], 1)
        P, Nn = float(yb.sum()), float((~yb).sum())
        for key, curve in (("auc", "ROC"), ("auc_precision_recall", "PR")):
            lo, hi = _auc_interval(bm.tp.astype(np.float64), bm.fp.astype(np.float64), P, Nn, ctp, cfp, curve)
            print("member %d %s: %.9f in [%.9f, %.9f], oracle %.9f" % (i, key, got[key], lo, hi, want[key]))
            assert lo - 1e-12 <= want[key] <= hi + 1e-12                # (the interval is around the oracle's value)
            assert lo - 1e-12 <= got[key] <= hi + 1e-12, (i, key)
        # |d loss / d z| <= 1 and sigmoid' <= 1/4: every example may move these by its share of the bar
        assert abs(got["average_loss"] - want["average_loss"]) <= float(s["dz"].mean()) + 1e-12, i
        assert abs(got["prediction/mean"] - want["prediction/mean"]) <= float(s["tol"].mean()) + 1e-12, i
        # loss: the mean over the batches of the batch's mean, at the project's bar for a loss (2e-5 relative)
        zz, yy = s["z"], y.astype(np.float64)
        per = np.maximum(zz, 0) - zz * yy + np.log1p(np.exp(-np.abs(zz)))
        lo_ = float(np.mean([per[t * B:(t + 1) * B].mean() for t in range(T)]))
        assert abs(got["loss"] - lo_) < 2e-5 * lo_, (i, got["loss"], lo_)


# ---- refusals through the binding -----------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    B = 32
    specs = [MIXED[i] for i in (0, 2, 13)]
    group, pop = _trained(specs)
    ids, y = _eval_set(5, 100)
    k, plan = pop.k, pop._plan_for(B)[1]
    T = 4
    tail = torch.ones(3, device="cuda")
    gl, loss = guarded_nan(3, T)
    gh, hist = _guarded_i64(3 * 402)
    gc, counts = _guarded_i64(3 * 8)
    par = torch.full((3, T, 3), float("nan"), dtype=torch.float64, device="cuda")
    before = [_snap(m) for m in group]
    ok = (plan, 3, ids, y, 100, tail, None, loss, hist, counts, par, 0)

    def edit(**kw):
        names = ("plan", "M", "ids", "y", "N", "tail", "logits", "loss", "hist", "counts", "par", "blocks")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    for match, args in ((r"\(-1\): eval_group: 2 members, the plan has 3", edit(M=2)), (r"\(-1\): eval_group: N=0", edit(N=0)),
                        (r"\(-1\): eval_group: plan", edit(plan=_lib.FusedGroupPlan())), (r"ids / labels", edit(ids=None)),
                        (r"batch_loss / hist / counts / partials", edit(hist=None)), (r"tail_scale", edit(tail=None)),
                        (r"\(-2\): eval_group: blocks=1025", edit(blocks=1025))):
        with pytest.raises(_lib.MiError, match=match):
            k.mi_eval_group(*args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(par).all()) and not bool(hist.any()) and not bool(counts.any())
    assert all(torch.equal(getattr(m, n), t) for m, s in zip(group, before) for n, t in s.items())
    k.mi_eval_group(*ok)                                                 # and the same arguments do work
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and int(counts.view(3, 8)[:, 0].sum()) == 300
    assert guards_intact(gl) and _i64_guards_intact(gh) and _i64_guards_intact(gc)


# ---- the grid-search CLI ----------------------------------------------------------------------------------------------
def test_sweep_cli_writes_the_members_curves(tmp_path, capsys):
    from trainers import _cli, ml_100k, sweep
    job = str(tmp_path / "job")
    flags = ["--synthetic", "2000", "--job-dir", job, "--learning-rate", "0.001", "0.01", "--dropout", "0", "0.1"]
    args = sweep.make_parser().parse_args(flags + ["--train-steps", "60", "--eval-every", "25", "--final-eval", "fused"])
    members = sweep.train_and_evaluate(args)
    assert all(m.global_step == 60 for m in members)
    out = capsys.readouterr().out
    assert out.count("INFO: evaluation at step") == 3 and "Saving dict for global step" not in out     # (no Estimator.evaluate)
    lines = [json.loads(line) for line in open(os.path.join(job, "sweep_eval.jsonl"))]
    assert [rec["global_step"] for rec in lines] == [25, 50, 60]
    rows = json.load(open(os.path.join(job, "sweep.json")))["members"]
    aucs = [r["metrics"]["auc"] for r in rows]
    assert aucs == sorted(aucs, reverse=True)
    for r in rows:
        i = r["member"]
        curve = [(rec["members"][i]["auc"], -rec["global_step"]) for rec in lines]
        assert np.isfinite([c[0] for c in curve]).all() and (r["best_value"], -r["best_step"]) == max(curve)
        assert r["metrics"] == dict(lines[-1]["members"][i], global_step=60.0)
        assert os.path.exists(os.path.join(job, "member_%d" % i, "model.ckpt-60.pt"))
    # the last line is FusedPopulation.evaluate on the members as their checkpoints restore them
    config = _cli.get_run_config()
    restored = sweep.make_members(args, sweep.grid(args), config)
    pop = sweep.train(restored, ml_100k.get_input_fn("synthetic:2000:1", batch_size=32), 60, config)
    assert all(m.global_step == 60 for m in restored)
    ev = sweep.PopulationEval("synthetic:200:2", 32, "auc", str(tmp_path / "elsewhere"))
    ev.load(restored[0].params["_store"]["plan"], restored[0]._engine().device)
    again = pop.evaluate(ev.data[0], ev.data[1], batch_size=32)
    assert ev.data[1].numel() == 200
    assert [{k: float(v) for k, v in m.items()} for m in again] == lines[-1]["members"]
