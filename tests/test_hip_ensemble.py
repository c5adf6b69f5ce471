"""GPU: serving an ensemble in one launch — mi_predict_group (csrc/serve.hip) through the bound entry, FusedGroup,
EnsemblePredictor and the two CLIs.

Every member's logit bit for bit against its own predict_fused, the ensemble's logit bit for bit against the fp32 mean in
member order formed by numpy, the head's outputs bit for bit against mi_binary_predictions, repeatability with the same
buffers (the tickets return to zero, nothing is written outside the outputs), the entry's refusals before anything is
launched, and the path from a sweep to its ensemble's predictions end to end."""
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import DeepFM, HipKernels, OptimizerSpec
from mi355x_rec.predictor import EnsemblePredictor, FusedGroup, _serve_member
from tests.util import PKG, ROOT, _run_module, guarded_nan, guards_intact, max_err_scaled
from trainers import ml_100k

pytestmark = pytest.mark.gpu

VOCAB = [9, 13, 5, 50, 7, 3]
BATCHES = (1, 31, 32, 33, 70)
# the mixed population: the CLI shape; no FM term; two output tiles per wave in a layer; no DNN; four tiles per wave
MIXED = [dict(embedding_size=4, hidden_units=[16, 16], activation="relu"),
         dict(embedding_size=8, hidden_units=[8], activation="tanh", use_mf=False),
         dict(embedding_size=16, hidden_units=[130, 40], activation="sigmoid"),
         dict(embedding_size=4, hidden_units=[], use_dnn=False),
         dict(embedding_size=4, hidden_units=[300])]
# canned-estimator style: raw numeric columns, a subset of the fields in the wide part
NUMERIC = [dict(embedding_size=4, hidden_units=[16, 8], n_numeric=2, numeric="raw", use_mf=False, reduction="sum",
                wide_fields=[True, False, True, True, False, True]),
           dict(embedding_size=8, hidden_units=[24], n_numeric=2, numeric="raw", use_mf=False, reduction="sum",
                wide_fields=[False, True, True, False, True, True], activation="tanh")]


def _engines(specs):
    out = []
    for i, s in enumerate(specs):
        m = DeepFM(VOCAB, optimizer=OptimizerSpec("SGD"), device="cuda", **s)
        g = torch.Generator(device="cuda")
        g.manual_seed(40 + i)
        m.init_variables(g, lin_scale=0.3)
        out.append(m)
    return out


@pytest.fixture(scope="module")
def mixed():
    return _engines(MIXED)


@pytest.fixture(scope="module")
def numeric():
    return _engines(NUMERIC)


def _batch(B, nd=0, seed=0):
    rng = np.random.default_rng(1000 * seed + B)
    ids = torch.from_numpy(np.stack([rng.integers(0, v, B) for v in VOCAB], 1).astype(np.int32)).cuda()
    x = torch.from_numpy(rng.standard_normal((B, nd)).astype(np.float32)).cuda() if nd else None
    return ids, x


def _guarded(M, B):
    """the entry's buffers for M members and B requests, every float output between NaN guards (class_ids: its own guards)"""
    whole, bufs = {}, {}
    for key, shape in (("member_logits", (M, B)), ("logits", (B, 1)), ("logistic", (B, 1)), ("probabilities", (B, 2))):
        whole[key], bufs[key] = guarded_nan(*shape)
    cls = torch.full((B + 128,), -7, dtype=torch.int64, device="cuda")
    whole["class_ids"], bufs["class_ids"] = cls, cls[64:64 + B].view(B, 1)
    tickets = torch.zeros((B + 31) // 32, dtype=torch.int32, device="cuda")
    return whole, {"member_logits": bufs["member_logits"], "tickets": tickets,
                   "out": {k: bufs[k] for k in ("logits", "logistic", "probabilities", "class_ids")}}


def _intact(whole, B):
    cls = whole["class_ids"]
    return all(guards_intact(whole[k]) for k in ("member_logits", "logits", "logistic", "probabilities")) and \
        bool((cls[:64] == -7).all()) and bool((cls[64 + B:] == -7).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_against_members(engines, group, ids, x, whole, bufs):
    """one synchronised call: member bits, ensemble bits, head bits, tickets, guards"""
    M, B = len(engines), ids.shape[0]
    out = group.run(ids, x, bufs)
    torch.cuda.synchronize()
    assert not bool(bufs["tickets"].any()) and _intact(whole, B)
    for key in ("member_logits", "logits", "logistic", "probabilities"):
        t = bufs["member_logits"] if key == "member_logits" else out[key]
        assert not bool(torch.isnan(t).any()), key
    solo = [e.predict_fused(ids, x) for e in engines]
    for i, s in enumerate(solo):
        assert torch.equal(_bits(bufs["member_logits"][i]), _bits(s["logits"].reshape(-1))), (M, B, i)
    z = [s["logits"].reshape(-1).cpu().numpy() for s in solo]
    acc = z[0]
    for zi in z[1:]:
        acc = (acc + zi).astype(np.float32)
    want = (acc / np.float32(M)).astype(np.float32)
    got = out["logits"].reshape(-1).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (M, B)
    lg = torch.empty(B, 1, device="cuda")
    pr = torch.empty(B, 2, device="cuda")
    cl = torch.empty(B, 1, dtype=torch.int64, device="cuda")
    group.k.mi_binary_predictions(out["logits"].reshape(-1).contiguous(), None, B, lg, pr, cl, None)
    assert torch.equal(_bits(out["logistic"]), _bits(lg)) and torch.equal(_bits(out["probabilities"]), _bits(pr))
    assert torch.equal(out["class_ids"], cl)
    return solo, out


@pytest.mark.parametrize("M", [1, 2, 5])
def test_member_and_ensemble_bits(mixed, M):
    engines = mixed[:M]
    group = FusedGroup(engines)
    for B in BATCHES:
        ids, _ = _batch(B)
        whole, bufs = _guarded(M, B)
        solo, out = _check_against_members(engines, group, ids, None, whole, bufs)
        if M == 1:                                                    # the member's own dict: a division by 1.0f is exact
            for key in ("logits", "logistic", "probabilities"):
                assert torch.equal(_bits(out[key]), _bits(solo[0][key])), (B, key)
            assert torch.equal(out["class_ids"], solo[0]["class_ids"])


def test_the_last_members_alone_and_in_another_order(mixed):
    """a group is defined by its member order alone: the wide tiles-per-wave paths first, and a population of the two widest"""
    for engines in ([mixed[4], mixed[2], mixed[3]], [mixed[2], mixed[4]]):
        group = FusedGroup(engines)
        for B in (33, 70):
            ids, _ = _batch(B, seed=2)
            whole, bufs = _guarded(len(engines), B)
            _check_against_members(engines, group, ids, None, whole, bufs)


@pytest.mark.parametrize("B", [1, 33])
def test_numeric_population_bits(numeric, B):
    group = FusedGroup(numeric)
    ids, x = _batch(B, nd=2, seed=1)
    whole, bufs = _guarded(2, B)
    _check_against_members(numeric, group, ids, x, whole, bufs)


def test_twenty_five_calls_with_the_same_buffers_give_the_same_bits(mixed):
    group = FusedGroup(mixed)
    B = 70
    ids, _ = _batch(B, seed=3)
    whole, bufs = _guarded(5, B)
    first = None
    for call in range(25):
        out = group.run(ids, None, bufs)
        torch.cuda.synchronize()
        assert not bool(bufs["tickets"].any()), call
        assert _intact(whole, B), call
        now = [_bits(bufs["member_logits"]).clone()] + [_bits(out[k]).clone() for k in ("logits", "logistic", "probabilities")] + [
            out["class_ids"].clone()]
        assert not any(bool(torch.isnan(t).any()) for t in (bufs["member_logits"], out["logits"], out["logistic"], out["probabilities"]))
        if first is None:
            first = now
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, now)), call
        # the next call starts from poisoned outputs: every element has to be written again
        for t in (bufs["member_logits"], out["logits"], out["logistic"], out["probabilities"]):
            t.fill_(float("nan"))
        out["class_ids"].fill_(-7)


def test_refusals_through_the_entry_launch_nothing(mixed, numeric):
    k = HipKernels()
    B = 33

    def members_of(engines, keep):
        return (_lib.ServeMember * len(engines))(*[_serve_member(e, keep) for e in engines])

    def table_for(M):
        return torch.full((max(int(k.query("mi_predict_group_plan_bytes", M)), 16),), 0xA5, dtype=torch.uint8, device="cuda")

    keep = []
    lead = mixed[0]
    # ---- the plan: a refused one writes neither the device table nor *plan
    wide = members_of(mixed[:2], keep)
    widths = torch.tensor([lead.F * 8, 513, 1], dtype=torch.int32)
    offs = torch.tensor([0, 0, 0, 0], dtype=torch.int64)
    keep += [widths, offs]
    wide[1].widths, wide[1].layer_off, wide[1].n_layers = widths.data_ptr(), offs.data_ptr(), 2
    for members, M, msg in ((wide, 2, r"\(-2\).*member 1: predict_fused: hidden width 513"),
                            (members_of(mixed[:1], keep), 0, r"\(-1\).*0 members"),
                            (members_of(mixed[:1], keep), 257, r"\(-2\).*257 members \(at most 256")):
        table, plan = table_for(max(M, 1)), _lib.ServeGroupPlan()
        with pytest.raises(_lib.MiError, match=msg):
            k.mi_predict_group_plan(members, M, lead.F, 0, lead.field_off, table, plan)
        torch.cuda.synchronize()
        assert bool((table == 0xA5).all()) and plan.magic == 0 and plan.device_table is None and plan.n_members == 0

    # ---- the call
    def fresh(M):
        whole, bufs = _guarded(M, B)
        o = bufs["out"]
        return whole, bufs, [bufs["member_logits"], bufs["tickets"], o["logits"], o["logistic"], o["probabilities"], o["class_ids"]]

    def untouched(whole, bufs):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(whole[key]).all()) for key in ("member_logits", "logits", "logistic", "probabilities")) and \
            bool((whole["class_ids"] == -7).all()) and not bool(bufs["tickets"].any())

    g3 = FusedGroup(mixed[:3])
    ids, _ = _batch(B)
    cases = []
    whole, bufs, a = fresh(2)
    cases.append(("2 members, the plan has 3", (g3.plan, 2, ids, None, B, *a), whole, bufs))
    whole, bufs, a = fresh(3)
    cases.append(("tickets", (g3.plan, 3, ids, None, B, a[0], None, *a[2:]), whole, bufs))
    whole, bufs, a = fresh(3)
    cases.append(("member_logits", (g3.plan, 3, ids, None, B, None, *a[1:]), whole, bufs))
    whole, bufs, a = fresh(3)
    cases.append(("ids", (g3.plan, 3, None, None, B, *a), whole, bufs))
    whole, bufs, a = fresh(3)
    cases.append(("at least one request", (g3.plan, 3, ids, None, 0, *a), whole, bufs))
    whole, bufs, a = fresh(3)
    cases.append(("no output requested", (g3.plan, 3, ids, None, B, a[0], a[1], None, None, None, None), whole, bufs))
    whole, bufs, a = fresh(3)
    cases.append(("not written by mi_predict_group_plan", (_lib.ServeGroupPlan(), 3, ids, None, B, *a), whole, bufs))
    gn = FusedGroup(numeric)
    whole, bufs, a = fresh(2)
    cases.append(("x_num", (gn.plan, 2, ids, None, B, *a), whole, bufs))
    for msg, args, whole, bufs in cases:
        with pytest.raises(_lib.MiError, match=msg):
            k.mi_predict_group(*args)
        assert untouched(whole, bufs), msg
    # (the same buffers do run: the refusals above were the arguments')
    whole, bufs, a = fresh(3)
    k.mi_predict_group(g3.plan, 3, ids, None, B, *a)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(bufs["out"]["logits"]).any()) and not bool(bufs["tickets"].any())


def test_host_side_refusals(mixed):
    with pytest.raises(ValueError, match="no members"):
        FusedGroup([])
    big = DeepFM(VOCAB, embedding_size=4, hidden_units=[513], optimizer=OptimizerSpec("SGD"), device="cuda")
    with pytest.raises(ValueError, match="member 1: the model has a hidden layer of 513 units"):
        FusedGroup([mixed[0], big])
    other = DeepFM(VOCAB[:5] + [4], embedding_size=4, hidden_units=[8], optimizer=OptimizerSpec("SGD"), device="cuda")
    with pytest.raises(ValueError, match="member 1 has columns"):
        FusedGroup([mixed[0], other])


# ---- end to end: exports and a sweep ----------------------------------------------------------------------------------
def _requests(spec):
    cols, _ = ml_100k._read_csv(spec)
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    return {k: v for k, v in cols.items() if k in recv}


def test_ensemble_predictor_fused_equals_layered(tmp_path):
    dirs = []
    for name, E in (("a", "4"), ("b", "8")):
        job = str(tmp_path / name)
        _run_module("trainers.deep_fm", ["--synthetic", "400", "--job-dir", job, "--train-steps", "20", "--embedding-size", E])
        dirs.append(os.path.join(job, "export", "exporter"))
    feats = _requests("synthetic:70:3")
    fused = EnsemblePredictor.from_exports(dirs, mode="fused")(feats, return_members=True)
    layered = EnsemblePredictor.from_exports(dirs, mode="layered", member_mode="layered")(feats, return_members=True)
    assert fused["logits"].shape == (70, 1) and fused["member_logits"].shape == (2, 70)
    err = max_err_scaled(fused["logits"], layered["logits"])
    print("ensemble fused vs layered err=%.3g" % err)
    assert np.max(np.abs(fused["logits"] - layered["logits"])) < 1e-5, err
    assert np.array_equal(fused["class_ids"], layered["class_ids"])
    want = ((fused["member_logits"][0] + fused["member_logits"][1]) / np.float32(2)).astype(np.float32)
    assert np.array_equal(fused["logits"][:, 0], want)
    auto = EnsemblePredictor.from_exports(dirs)                        # the CLI shape at B = 70: auto is the group launch
    assert auto.use_fused(70) and np.array_equal(auto(feats)["logits"], fused["logits"])


def test_sweep_to_ensemble_predictions(tmp_path):
    job = str(tmp_path / "sweep")
    r = _run_module("trainers.sweep", ["--synthetic", "600", "--train-steps", "30", "--seeds", "3", "--ensemble", "2", "--job-dir", job])
    assert "INFO: ensemble of the 2 best members" in r.stdout
    doc = json.load(open(os.path.join(job, "sweep.json")))
    ens = doc["ensemble"]
    assert ens["members"] == [row["member"] for row in doc["members"][:2]] and len(ens["members"]) == 2
    assert ens["metrics"] and all(np.isfinite(v) for v in ens["metrics"].values()) and doc["select"] in ens["metrics"]
    out = str(tmp_path / "pred.csv")
    _run_module("trainers.predict", ["--job-dir", job, "--top", "2", "--input", "synthetic:70:3", "--output", out])
    rows = list(csv.DictReader(open(out)))
    assert len(rows) == 70
    got = np.asarray([float(row["logit"]) for row in rows], np.float32)
    want = EnsemblePredictor.from_sweep(job, top=2)(_requests("synthetic:70:3"))
    assert np.array_equal(got, want["logits"][:, 0])
    assert np.array_equal(np.asarray([int(row["class_id"]) for row in rows]), want["class_ids"][:, 0])
    r = subprocess.run([sys.executable, "-m", "trainers.predict", "--job-dir", os.path.join(job, "member_0"), "--top", "1",
                        "--input", "synthetic:5:1"], cwd=PKG, env=dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT])),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "no sweep.json" in r.stderr
