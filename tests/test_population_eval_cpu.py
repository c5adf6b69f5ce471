"""CPU: the host side of the population evaluation — FusedPopulation.evaluate and trainers.sweep's --eval-every /
--final-eval.  mi_eval_group is stood in by a numpy restatement of its contract in include/mi355x_rec.h
(tests.cpu_kernels.NumpyKernels: a tile's logits and batch loss are what mi_train_step_fused reports for that batch with
keep_prob = 1, taken on COPIES of the member's buffers; the counters are mi_eval_accumulate's in numpy); the real kernel is
tested in test_hip_population_eval.py.  The refusals and the binding are checked against the
real library, which decides them on the host."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.metrics import metrics_from_counters
from mi355x_rec.population import FusedPopulation
from tests.cases import _numpy_engine, _sweep_args
from tests.cpu_kernels import NumpyKernels, counters, cpu_kernels  # noqa: F401  (a fixture)
from tests.util import _fresh_ids, _header_decls, _t

F32 = np.float32


SPECS = [dict(E=8, hidden=[16, 8], dropout=0.25, seed=3), dict(E=4, hidden=[8], lr=0.01, activation="tanh"),
         dict(E=8, hidden=[16, 8], use_linear=False, reduction="sum"), dict(E=4, hidden=[], use_dnn=False, seed=9)]
VOCAB = [9, 13, 5, 6]


def _members(k, specs=SPECS, vocab=VOCAB):
    out = []
    for j, s in enumerate(specs):
        s = dict(s)
        m = _numpy_engine(vocab, s.pop("E"), s.pop("hidden"), k, s.pop("lr", 0.001), **s)
        g = torch.Generator()
        g.manual_seed(j)
        m.init_variables(g, lin_scale=0.3)
        out.append(m)
    return out


def _eval_set(N, vocab=VOCAB, seed=1):
    rng = np.random.default_rng(seed)
    return _t(_fresh_ids(rng, vocab, N)), _t((rng.random(N) < 0.4).astype(np.uint8))


def test_evaluate_is_metrics_from_counters_on_the_logits_and_the_mean_of_batch_losses():
    N, B = 100, 16                                                       # 6 tiles of 16 and a tail of 4
    k = NumpyKernels()
    members = _members(k)
    pop = FusedPopulation(members)
    ids, y = _eval_set(N)
    before = [m.state_dict() for m in members]
    k.calls.clear()
    out, logits = pop.evaluate(ids, y, batch_size=B, return_logits=True)
    assert k.calls == {"mi_train_group_plan": 1, "mi_eval_group": 1}
    assert len(out) == 4 and tuple(logits.shape) == (4, N)
    for i, m in enumerate(members):
        h, c, s = counters(logits[i].numpy(), y.numpy())
        want = metrics_from_counters(h, c, s)
        assert set(out[i]) == set(want) | {"loss"}
        for key, v in want.items():
            assert out[i][key] == pytest.approx(v, rel=1e-12, abs=1e-15), (i, key)
        # the loss: the mean over the 7 batch losses, each as the member's own fused step reports it without dropout — the tail
        # with the fp32 of 1/4 for a mean, 1 for a sum
        z = logits[i].numpy()
        yy = y.numpy().astype(F32)
        per = (np.maximum(z, 0) - z * yy + np.log1p(np.exp(-np.abs(z)))).astype(F32)
        bl = []
        for t in range(7):
            lo, hi = t * B, min(N, (t + 1) * B)
            scale = F32(1.0) if m.reduction == "sum" else F32(1.0 / (hi - lo))
            bl.append(float((per[lo:hi] * scale).sum(dtype=F32)))
        assert out[i]["loss"] == pytest.approx(np.mean(bl), rel=1e-6), i
        assert m.step == 0 and m._final_step == 0
        after = m.state_dict()
        for key, v in before[i].items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, after[key]), (i, key)
    # dropout is off in evaluation: member 0 (dropout 0.25) gives the logits of its dropout-free twin
    twin = _members(NumpyKernels(), [dict(SPECS[0], dropout=0.0)])[0]
    twin.load_state_dict(before[0])
    _, z = FusedPopulation([twin]).evaluate(ids, y, batch_size=B, return_logits=True)
    assert torch.equal(z[0], logits[0])
    # a population of one, batch_size dividing N, no logits
    one = FusedPopulation([members[1]]).evaluate(ids[:96].contiguous(), y[:96].contiguous(), batch_size=B)
    assert len(one) == 1 and np.isfinite(list(one[0].values())).all()


def test_the_tail_batch_is_reduced_with_its_own_scale():
    N, B = 20, 16
    k = NumpyKernels()
    members = _members(k, SPECS[1:3])                                    # a mean and a sum
    pop = FusedPopulation(members)
    ids, y = _eval_set(N, seed=2)
    out, logits = pop.evaluate(ids, y, batch_size=B, return_logits=True)
    yy = y.numpy().astype(np.float64)
    for i, m in enumerate(members):
        z = logits[i].numpy().astype(np.float64)
        per = np.maximum(z, 0) - z * yy + np.log1p(np.exp(-np.abs(z)))
        if m.reduction == "mean":
            want = 0.5 * (per[:16].mean() + per[16:].mean())             # (not the mean over the 20 examples)
        else:
            want = 0.5 * (per[:16].sum() + per[16:].sum())
        assert out[i]["loss"] == pytest.approx(want, rel=2e-6)
        assert out[i]["average_loss"] == pytest.approx(per.mean(), rel=2e-6)


def test_argument_checks_raise_with_the_populations_wording():
    k = NumpyKernels()
    pop = FusedPopulation(_members(k))
    ids, y = _eval_set(40)
    for bad_ids, bad_y, kw, msg in ((ids.long(), y, {}, r"ids must be a contiguous int32 \[N, 4\]"),
                                    (ids[:, :3].contiguous(), y, {}, "ids must be"), (ids.numpy(), y, {}, "ids must be"),
                                    (ids.t().contiguous().t(), y, {}, "ids must be"),
                                    (ids[:0], y[:0], {}, "no examples to evaluate"),
                                    (ids, y.float(), {}, r"labels must be a contiguous uint8 \[N\] tensor \(N = 40\)"),
                                    (ids, y[:8], {}, "labels must be"), (ids, y, dict(batch_size=0), "batch_size=0"),
                                    (ids, y, dict(batch_size=129), "member 0: the model has a batch of 129 examples")):
        with pytest.raises(ValueError, match="FusedPopulation: .*" + msg):
            pop.evaluate(bad_ids, bad_y, **kw)
    assert not k.calls


def test_the_plan_is_built_once_across_alternating_steps_and_evaluations():
    B = 8
    k = NumpyKernels()
    members = _members(k)
    pop = FusedPopulation(members)
    ids, y = _eval_set(50)
    rng = np.random.default_rng(0)
    plans = lambda: k.calls.get("mi_train_group_plan", 0)
    for step in range(3):
        pop.train_step(_t(_fresh_ids(rng, VOCAB, B)), _t((rng.random(B) < 0.3).astype(np.uint8)))
        out = pop.evaluate(ids, y)                                       # batch_size None: the step's
        assert len(out) == 4 and all(m.step == step + 1 and m._final_step == step + 1 for m in members)
    assert plans() == 1 and k.calls["mi_eval_group"] == 3 and k.calls["mi_train_group_step"] == 3
    pop.evaluate(ids, y, batch_size=16)                                  # another tile size: a plan of its own, kept
    pop.train_step(_t(_fresh_ids(rng, VOCAB, B)), _t((rng.random(B) < 0.3).astype(np.uint8)))
    pop.evaluate(ids, y, batch_size=16)
    pop.evaluate(ids, y)
    assert plans() == 2 and k.calls["mi_eval_group"] == 6
    # a member that took a layered step owes its rows their sweep: evaluate settles them first, as loss() does
    for m in members[1:]:
        m.fused_train_step(ids[:B].contiguous(), y[:B].contiguous())
    members[0].train_step(ids[:B].contiguous(), y[:B].contiguous())
    assert members[0]._final_step != members[0].step
    pop.evaluate(ids, y)
    assert all(m._final_step == m.step == 5 for m in members) and plans() == 2


# ---- the grid-search CLI ----------------------------------------------------------------------------------------------
GRID = ["--learning-rate", "0.001", "0.01", "--dropout", "0", "0.1"]


def _count_evaluate(monkeypatch):
    from mi355x_rec.estimator import Estimator
    calls = []
    real = Estimator.evaluate

    def counted(self, *a, **kw):
        calls.append(self.model_dir)
        return real(self, *a, **kw)
    monkeypatch.setattr(Estimator, "evaluate", counted)
    return calls


def test_sweep_eval_every_writes_the_curves(cpu_kernels, tmp_path, capsys, monkeypatch):
    from trainers import sweep
    calls = _count_evaluate(monkeypatch)
    job = tmp_path / "job"
    members = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "25", "--eval-every", "10", *GRID))
    lines = [json.loads(line) for line in open(job / "sweep_eval.jsonl")]
    assert [rec["global_step"] for rec in lines] == [10, 20, 25]         # every due step, and the last
    assert sum(m._engine().k.calls.get("mi_eval_group", 0) for m in members) == 3 and len(calls) == 4    # (--final-eval layered)
    out = capsys.readouterr().out
    assert out.count("INFO: evaluation at step") == 3 and "auc best = " in out and "30 examples" in out
    keys = {"accuracy", "accuracy_baseline", "auc", "auc_precision_recall", "average_loss", "label/mean", "prediction/mean",
            "precision", "recall", "loss"}
    assert all(len(rec["members"]) == 4 and all(set(m) == keys for m in rec["members"]) for rec in lines)
    rows = json.load(open(job / "sweep.json"))["members"]
    for r in rows:
        curve = [(rec["members"][r["member"]]["auc"], -rec["global_step"]) for rec in lines]
        assert (r["best_value"], -r["best_step"]) == max(curve)
    # the last line is the population's evaluation of the members as they are
    pop = FusedPopulation([m._engine() for m in members])
    ev = sweep.PopulationEval("synthetic:30:2", 16, "auc", str(job))
    ev.load(members[0].params["_store"]["plan"], torch.device("cpu"))
    again = pop.evaluate(ev.data[0], ev.data[1], batch_size=16)
    assert [{k_: float(v) for k_, v in m.items()} for m in again] == lines[-1]["members"]
    # the layered evaluation of a member sees the same batches: its metrics agree (fp32 against the stand-in's fp32)
    by = {r["member"]: r for r in rows}
    for i in range(4):
        for key in ("accuracy", "auc", "average_loss", "loss"):
            assert by[i]["metrics"][key] == pytest.approx(lines[-1]["members"][i][key], rel=1e-4, abs=1e-6), (i, key)
    # --select loss: best = lowest; a step that is due AND the last is written once
    job2 = tmp_path / "job2"
    sweep.train_and_evaluate(_sweep_args(job2, "--train-steps", "20", "--eval-every", "10", "--select", "loss", *GRID))
    lines = [json.loads(line) for line in open(job2 / "sweep_eval.jsonl")]
    assert [rec["global_step"] for rec in lines] == [10, 20]
    for r in json.load(open(job2 / "sweep.json"))["members"]:
        curve = [(rec["members"][r["member"]]["loss"], rec["global_step"]) for rec in lines]
        assert (r["best_value"], r["best_step"]) == min(curve)
    assert "loss best = " in capsys.readouterr().out


def test_sweep_default_flags_do_what_they_did(cpu_kernels, tmp_path, monkeypatch):
    from trainers import sweep
    a = sweep.make_parser().parse_args([])
    assert a.eval_every == 0 and a.final_eval == "layered"
    calls = _count_evaluate(monkeypatch)
    job = tmp_path / "job"
    members = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "12", *GRID))
    assert sorted(os.listdir(job)) == ["member_0", "member_1", "member_2", "member_3", "sweep.json"]      # (no sweep_eval.jsonl)
    rows = json.load(open(job / "sweep.json"))["members"]
    assert all(set(r) == {"member", "dir", "export", "global_step", "params", "flags", "metrics"} for r in rows)
    assert len(calls) == 4 and all("mi_eval_group" not in m._engine().k.calls for m in members)


def test_sweep_final_eval_fused_calls_no_estimator_evaluate(cpu_kernels, tmp_path, monkeypatch):
    from trainers import sweep
    calls = _count_evaluate(monkeypatch)
    job = tmp_path / "job"
    members = sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "12", "--final-eval", "fused", *GRID))
    assert calls == [] and sum(m._engine().k.calls.get("mi_eval_group", 0) for m in members) == 1
    lines = [json.loads(line) for line in open(job / "sweep_eval.jsonl")]
    assert [rec["global_step"] for rec in lines] == [12]
    doc = json.load(open(job / "sweep.json"))
    rows = doc["members"]
    aucs = [r["metrics"]["auc"] for r in rows]
    assert aucs == sorted(aucs, reverse=True)
    for r in rows:
        assert set(r) == {"member", "dir", "export", "global_step", "params", "flags", "metrics"}      # (no --eval-every: no best_*)
        assert r["metrics"] == dict(lines[0]["members"][r["member"]], global_step=12.0)
        assert os.path.exists(job / ("member_%d" % r["member"]) / "model.ckpt-12.pt") and os.path.isdir(r["export"])
    with pytest.raises(ValueError, match="--eval-every -1"):
        sweep.train_and_evaluate(_sweep_args(tmp_path / "bad", "--train-steps", "2", "--eval-every", "-1"))


# ---- the real library, without a device ---------------------------------------------------------------------------------
def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    """The real mi_eval_group without a device: every refusal is decided on the host, with its status and message, and
    nothing is launched or written."""
    N, M = 40, 3
    ids, y = torch.zeros(N, 3, dtype=torch.int32), torch.zeros(N, dtype=torch.uint8)
    T = 3                                                                # tiles of 16
    tail = torch.ones(M)
    loss, par = torch.full((M, T), float("nan")), torch.full((M, T, 3), float("nan"), dtype=torch.float64)
    hist, counts = torch.zeros(M, 2, 201, dtype=torch.int64), torch.zeros(M, 8, dtype=torch.int64)
    table = torch.zeros(4096, dtype=torch.uint8)

    def plan(magic=0x6d695f67726f7570, n=M, B=16, device_table=True):
        p = _lib.FusedGroupPlan()
        p.device_table, p.magic, p.n_members, p.B, p.F = (table.data_ptr() if device_table else None), magic, n, B, 3
        p.sweep_blocks, p.max_step, p.lds_bytes = 1, 100, 4096
        return p

    def refused(status, match, p=None, n=M, N_=N, blocks=0, **nulls):
        a = dict(ids=ids, labels=y, tail=tail, loss=loss, hist=hist, counts=counts, par=par)
        a.update(nulls)
        ptr = lambda t: None if t is None else t.data_ptr()
        p = plan() if p is None else p
        rc = lib.mi_eval_group(C.byref(p) if p is not False else None, n, ptr(a["ids"]), ptr(a["labels"]), N_, ptr(a["tail"]),
                               None, ptr(a["loss"]), ptr(a["hist"]), ptr(a["counts"]), ptr(a["par"]), blocks, None)
        msg = lib.mi_last_error().decode()
        assert rc == status and match in msg, (rc, msg)
    refused(-1, "eval_group: 2 members, the plan has 3", n=2)
    refused(-1, "eval_group: N=0 examples", N_=0)
    refused(-1, "eval_group: N=-5 examples", N_=-5)
    refused(-1, "eval_group: plan (not written by mi_train_group_plan)", p=plan(magic=0x1234))
    refused(-1, "eval_group: plan (not written by mi_train_group_plan)", p=_lib.FusedGroupPlan())
    refused(-1, "eval_group: plan (not written by mi_train_group_plan)", p=plan(device_table=False))
    refused(-1, "eval_group: plan (not written by mi_train_group_plan)", p=False)
    refused(-1, "eval_group: ids / labels", ids=None)
    refused(-1, "eval_group: ids / labels", labels=None)
    for name in ("loss", "hist", "counts", "par"):
        refused(-1, "eval_group: batch_loss / hist / counts / partials", **{name: None})
    refused(-1, "eval_group: tail_scale (the last tile has 8 of 16 examples)", tail=None)
    refused(-2, "eval_group: blocks=1025 (0 = the built-in choice, at most 1024)", blocks=1025)
    refused(-2, "eval_group: blocks=-1", blocks=-1)
    refused(-1, "eval_group: blocks=1024 for 1024 members (at most 65536 workgroups in all)", p=plan(n=1024), n=1024, blocks=1024)
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(par).all()) and not bool(hist.any()) and not bool(counts.any())
    assert lib.mi_abi_version() == 21


def test_header_binding_and_library_agree_on_the_new_entry(lib):
    decls = _header_decls()
    assert "mi_eval_group" in decls and "mi_eval_group" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mi_eval_group"][1]) == decls["mi_eval_group"] == 13
    assert hasattr(lib, "mi_eval_group") and set(decls) == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 21
    # the plan struct the entry reads is the one mi_train_group_plan writes: unchanged
    assert [f[0] for f in _lib.FusedGroupPlan._fields_] == ["device_table", "magic", "n_members", "B", "F", "sweep_blocks",
                                                           "max_step", "lds_bytes"]
