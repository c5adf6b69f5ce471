"""CPU: serving an export — LatestExporter's self-describing signature, Predictor.from_export (columns, FieldPlan and a
weights-only engine rebuilt from the export alone), the request checks, DeepFM.predict_fused's host side and the
`python -m trainers.predict` CLI.  mi_predict_fused is stood in by a numpy restatement of include/mi355x_rec.h
(tests.cpu_kernels.NumpyKernels); the real kernel is tested in test_hip_serve.py."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.feature_column import FieldPlan, column_from_json
from mi355x_rec.predictor import Predictor
from oracle import deepfm as O
from tests.cpu_kernels import NumpyKernels, cpu_kernels  # noqa: F401  (a fixture)
from tests.util import _requests, make_problem, max_err_scaled
from trainers import _cli, ml_100k, predict, recommend

def _train(tmp_path, model, extra=()):
    trainer, opt = recommend.MODELS[model]
    job = str(tmp_path / ("job_" + model))
    argv = ["--synthetic", "300", "--job-dir", job, "--train-steps", "25", "--batch-size", "16", "--device", "cpu"] + list(extra)
    est = trainer.train_and_evaluate(_cli.make_parser(model, opt).parse_args(argv))
    return est, job


@pytest.mark.parametrize("model,extra", [("deep_fm", ["--hidden-units", "8", "8"]), ("linear", []),
                                         ("deep", ["--hidden-units", "8"]), ("linear_deep", ["--hidden-units", "8"])])
def test_export_round_trip(tmp_path, cpu_kernels, model, extra):
    est, job = _train(tmp_path, model, extra)
    root = os.path.join(job, "export", "exporter")
    newest = os.path.join(root, sorted(os.listdir(root))[-1])
    assert sorted(os.listdir(newest)) == ["signature.json", "variables.pt"]          # no file added to the export
    sig = json.load(open(os.path.join(newest, "signature.json")))
    assert sig["receiver_tensors"] == {k: str(v) for k, v in ml_100k.serving_input_fn().receiver_tensors.items()}
    assert sig["outputs"] == ["logits", "logistic", "probabilities", "class_ids", "classes"]
    assert sig["global_step"] == est.global_step and "sharding" not in sig
    m = sig["model"]
    assert m["tf_model"] == est.params.get("tf_model", "deep_fm")
    assert m["engine"] == {"activation": "relu", "reduction": "mean" if model == "deep_fm" else "sum"}
    assert json.loads(json.dumps(m)) == m                                            # plain JSON
    # "model" rebuilds columns whose transforms give the ids of the originals
    feats = _requests()
    plan0 = est.params["_store"]["plan"]
    plan1 = FieldPlan([column_from_json(c) for c in m["categorical_columns"]], [column_from_json(c) for c in m["numeric_columns"]])
    assert [c.name for c in plan1.categorical] == [c.name for c in plan0.categorical]
    assert plan1.vocab_sizes == plan0.vocab_sizes
    ids0, x0 = plan0.transform(feats)
    ids1, x1 = plan1.transform(feats)
    assert np.array_equal(ids0, ids1) and (x0 is None) == (x1 is None)
    assert {c["kind"] for c in m["categorical_columns"]} == {"hash_bucket", "bucketized", "vocabulary_list", "identity"}
    # the predictor against Estimator.predict on the same rows
    want = list(est.predict(lambda: iter([feats])))
    want_logits = np.asarray([w["logits"][0] for w in want], np.float64)
    want_cls = np.asarray([w["class_ids"][0] for w in want])
    for mode in ("layered", "fused", "auto"):
        p = Predictor.from_export(root if mode != "fused" else newest, device="cpu", mode=mode)
        got = p(feats)
        assert set(got) == set(sig["outputs"])
        assert got["logits"].shape == (30, 1) and got["probabilities"].shape == (30, 2) and got["class_ids"].dtype == np.int64
        if mode == "layered":
            assert np.max(np.abs(got["logits"][:, 0] - want_logits)) < 1e-6
            assert np.array_equal(got["class_ids"][:, 0], want_cls)
        else:
            assert max_err_scaled(got["logits"][:, 0], want_logits) < 1e-5
        assert np.array_equal(got["classes"], got["class_ids"])
        assert np.allclose(got["probabilities"].sum(1), 1.0, atol=1e-6)
    # the weights-only engine: no optimizer slot anywhere
    eng = p.engine
    assert all(getattr(eng, k) is None for k in ("t_s0", "t_s1", "l_s0", "l_s1", "d_s0", "d_s1"))
    assert eng.table is None or eng.ts == eng.E


def test_request_checks(tmp_path, cpu_kernels):
    est, job = _train(tmp_path, "deep_fm", ["--hidden-units", "8"])
    root = os.path.join(job, "export", "exporter")
    p = Predictor.from_export(root, device="cpu", mode="fused")
    feats = _requests(12)
    full = p(feats)
    # omitted genre keys = explicit zeros
    zeros = dict(feats)
    for g in ml_100k.GENRE:
        zeros[g] = np.zeros(12, np.int32)
    base = {k: v for k, v in feats.items() if k not in ml_100k.GENRE}
    assert np.array_equal(p(base)["logits"], p(zeros)["logits"])
    assert not np.array_equal(p(base)["logits"], full["logits"])
    assert np.array_equal(p({k: list(v) for k, v in feats.items()})["logits"], full["logits"])     # sequences of any kind
    with pytest.raises(ValueError, match="zipcode"):
        p({k: v for k, v in feats.items() if k != "zipcode"})
    with pytest.raises(ValueError, match="rating"):
        p(dict(feats, rating=np.ones(12, np.int32)))
    with pytest.raises(ValueError, match="age"):
        p(dict(feats, age=feats["age"][:5]))
    with pytest.raises(ValueError, match="mode"):
        Predictor.from_export(root, device="cpu", mode="eager")
    newest = os.path.join(root, sorted(os.listdir(root))[-1])
    sig = json.load(open(os.path.join(newest, "signature.json")))
    # an export written before signatures described their model
    old = tmp_path / "old"
    os.makedirs(old)
    json.dump({k: v for k, v in sig.items() if k != "model"}, open(old / "signature.json", "w"))
    with pytest.raises(ValueError, match="\"model\""):
        Predictor.from_export(str(old), device="cpu")
    # a row-sharded export
    sh = tmp_path / "sharded"
    os.makedirs(sh)
    json.dump(dict(sig, sharding={"world": 2, "files": ["variables.rank0.pt", "variables.rank1.pt"], "rule": "row r: file r % world"}),
              open(sh / "signature.json", "w"))
    with pytest.raises(ValueError, match="sharded"):
        Predictor.from_export(str(sh), device="cpu")
    with pytest.raises(FileNotFoundError):
        Predictor.from_export(str(tmp_path / "nothing"), device="cpu")


VOCAB = [11, 7, 5, 9, 13, 6]


def _model(**kw):
    kw.setdefault("hidden_units", [8, 4])
    m = DeepFM(VOCAB, embedding_size=4, device="cpu", _kernels=NumpyKernels(), **kw)
    p, ids, x, _ = make_problem(1, VOCAB, 4, kw["hidden_units"], 9, n_numeric=kw.get("n_numeric", 0), use_dnn=kw.get("use_dnn", True))
    if kw.get("numeric") == "raw":                                    # kernel_0: one row per raw numeric column
        k0, b0 = p.mlp[0]
        tail = (np.random.default_rng(1).standard_normal((kw["n_numeric"], k0.shape[1])) * 0.3).astype(np.float32)
        p.mlp[0] = (np.concatenate([k0[:len(VOCAB) * 4], tail]), b0)
    m.load_oracle_params(p)
    return m, p, ids, x


@pytest.mark.parametrize("kw", [dict(), dict(hidden_units=[]), dict(use_dnn=False), dict(use_linear=False, use_mf=False),
                                dict(n_numeric=2), dict(n_numeric=2, numeric="raw", use_mf=False), dict(activation="tanh")])
def test_predict_fused_host_side_matches_oracle(kw):
    m, p, ids, x = _model(**kw)
    out = m.predict_fused(torch.from_numpy(ids), None if x is None else torch.from_numpy(x))
    flags = dict(use_linear=kw.get("use_linear", True), use_mf=kw.get("use_mf", True), use_dnn=kw.get("use_dnn", True))
    ref = O.forward(p.astype(np.float64), ids, None if x is None else x.astype(np.float64), numeric=kw.get("numeric", "embed"),
                    activation=kw.get("activation", "relu"), **flags)["logits"]
    assert max_err_scaled(out["logits"].numpy()[:, 0], ref) < 1e-5
    assert out["logits"].shape == (9, 1) and out["logistic"].shape == (9, 1) and out["probabilities"].shape == (9, 2)
    assert out["class_ids"].dtype == torch.int64 and out["classes"] is out["class_ids"]
    lay = m.predict_logits(torch.from_numpy(ids), None if x is None else torch.from_numpy(x))
    assert max_err_scaled(out["logits"].numpy()[:, 0], lay.numpy()) < 1e-5


def test_predict_fused_argument_errors_and_refusals():
    m, _, ids, _ = _model()
    t = torch.from_numpy(ids)
    assert m.fused_predict_ok()
    with pytest.raises(ValueError):
        m.predict_fused(t.long())                                     # dtype
    with pytest.raises(ValueError):
        m.predict_fused(t[:, :3].contiguous())                        # width
    with pytest.raises(ValueError):
        m.predict_fused(t, torch.zeros(9, 1))                         # no numeric column in the model
    with pytest.raises(ValueError):
        m.predict_fused(t[:0])                                        # no rows
    big = DeepFM(VOCAB, embedding_size=4, hidden_units=[1024, 8], device="cpu", _kernels=NumpyKernels())
    assert not big.fused_predict_ok()
    with pytest.raises(ValueError, match="1024"):
        big.predict_fused(t)
    deep = DeepFM(VOCAB, embedding_size=4, hidden_units=[4] * 9, device="cpu", _kernels=NumpyKernels())
    with pytest.raises(ValueError, match="9 hidden layers"):
        deep.predict_fused(t)
    m.shard = object()                                                # a row-sharded engine
    assert not m.fused_predict_ok()
    with pytest.raises(NotImplementedError):
        m.predict_fused(t)


def test_predict_fused_scores_lazily_updated_adam_rows_at_their_caught_up_value():
    rng = np.random.default_rng(3)
    m = DeepFM(VOCAB, embedding_size=4, hidden_units=[8], optimizer=OptimizerSpec("Adam", 0.01), device="cpu", _kernels=NumpyKernels())
    p, _, _, _ = make_problem(2, VOCAB, 4, [8], 4)
    m.load_oracle_params(p)
    for _ in range(3):
        ids = np.stack([rng.integers(0, v, 4) for v in VOCAB], 1).astype(np.int32)
        m.train_step(torch.from_numpy(ids), torch.from_numpy((rng.random(4) < 0.5).astype(np.uint8)))
    q = torch.from_numpy(np.stack([rng.integers(0, v, 20) for v in VOCAB], 1).astype(np.int32))
    assert m._final_step != m.step
    got = m.predict_fused(q)["logits"].numpy()[:, 0]
    assert m._final_step == m.step                                   # finalize_rows ran
    assert max_err_scaled(got, m.predict_logits(q).numpy()) < 1e-5


def test_predict_cli_scores_a_csv(tmp_path, cpu_kernels):
    est, job = _train(tmp_path, "linear_deep", ["--hidden-units", "8"])
    cols, n = ml_100k._read_csv("synthetic:23:5")
    path = tmp_path / "in.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(ml_100k.COLUMNS)
        for i in range(n):
            w.writerow([cols[c][i] for c in ml_100k.COLUMNS])
    outs = {}
    for mode in ("fused", "layered"):
        out = predict.main(["--job-dir", job, "--input", str(path), "--mode", mode, "--device", "cpu", "--batch-size", "10",
                            "--output", str(tmp_path / (mode + ".csv"))])
        rows = list(csv.DictReader(open(out)))
        assert len(rows) == n and set(rows[0]) == {"logit", "probability", "class_id"}
        outs[mode] = np.asarray([float(r["logit"]) for r in rows])
    assert max_err_scaled(outs["fused"], outs["layered"]) < 2e-5
    feats = {k: v for k, v in cols.items() if k in ml_100k.serving_input_fn().receiver_tensors}
    want = np.asarray([w["logits"][0] for w in est.predict(lambda: iter([feats]))], np.float64)
    assert np.max(np.abs(outs["layered"] - want)) < 1e-6
    default = predict.main(["--job-dir", job, "--input", "synthetic:7:1", "--device", "cpu"])
    assert default == os.path.join(job, "predict", "predictions.csv") and len(list(csv.DictReader(open(default)))) == 7
