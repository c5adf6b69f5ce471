"""CPU: the host side of top-K recommendation — DeepFM.top_k's argument checks and per-side decomposition, the feature
dicts' split into sides by key, the CLI's user / item tables, exclusion CSR and ranking metrics.  mi_pair_topk is stood
in by numpy (tests.cpu_kernels.NumpyKernels); the real kernel is tested in test_hip_rank.py."""
import math
import os

import numpy as np
import pytest
import torch

from mi355x_rec.engine import DeepFM
from mi355x_rec.feature_column import FieldPlan
from mi355x_rec.model import split_sides
from oracle import deepfm as O
from tests.cpu_kernels import NumpyKernels
from tests.util import make_problem, max_err_scaled
from trainers import ml_100k, recommend

VOCAB = [11, 7, 5, 9, 13, 6]


def _model(**kw):
    kw.setdefault("hidden_units", [8, 4])
    m = DeepFM(VOCAB, embedding_size=4, device="cpu", _kernels=NumpyKernels(), **kw)
    p, _, _, _ = make_problem(1, VOCAB, 4, kw["hidden_units"], 4, n_numeric=kw.get("n_numeric", 0),
                              use_dnn=kw.get("use_dnn", True))
    m.load_oracle_params(p)
    return m, p


def _ids(rng, fields, n):
    return torch.from_numpy(np.stack([rng.integers(0, VOCAB[f], n) for f in fields], 1).astype(np.int32))


@pytest.mark.parametrize("hidden,flags", [([8, 4], (True, True, True)), ([], (True, True, True)),
                                          ([8, 4], (True, False, True)), ([8], (False, True, False))])
def test_top_k_decomposition_matches_oracle(hidden, flags):
    lin, mf, dnn = flags
    m, p = _model(hidden_units=hidden, use_linear=lin, use_mf=mf, use_dnn=dnn)
    rng = np.random.default_rng(0)
    qf, cf = [1, 4], [0, 2, 3, 5]
    qi, ci = _ids(rng, qf, 5), _ids(rng, cf, 9)
    score, idx, scores = m.top_k(qi, ci, qf, 3, return_scores=True)
    ids = np.zeros((45, 6), np.int32)
    ids[:, qf] = np.repeat(qi.numpy(), 9, 0)
    ids[:, cf] = np.tile(ci.numpy(), (5, 1))
    ref = O.forward(p.astype(np.float64), ids, use_linear=lin, use_mf=mf, use_dnn=dnn)["logits"].reshape(5, 9)
    assert max_err_scaled(scores.numpy(), ref) < 1e-5
    assert np.array_equal(idx.numpy(), np.argsort(-scores.numpy(), 1, kind="stable")[:, :3])


def test_top_k_numeric_column_on_either_side():
    m, p = _model(n_numeric=2)
    rng = np.random.default_rng(1)
    qf = [0, 6]                                  # field 0 and numeric column 0 (= F + 0)
    cf = [1, 2, 3, 4, 5]
    qi, ci = _ids(rng, [0], 4), _ids(rng, cf, 6)
    qx = torch.from_numpy(rng.standard_normal((4, 1)).astype(np.float32))
    cx = torch.from_numpy(rng.standard_normal((6, 1)).astype(np.float32))
    _, _, scores = m.top_k(qi, ci, qf, 2, qx, cx, return_scores=True)
    ids = np.zeros((24, 6), np.int32)
    ids[:, [0]] = np.repeat(qi.numpy(), 6, 0)
    ids[:, cf] = np.tile(ci.numpy(), (4, 1))
    x = np.stack([np.repeat(qx.numpy()[:, 0], 6), np.tile(cx.numpy()[:, 0], 4)], 1)
    ref = O.forward(p.astype(np.float64), ids, x.astype(np.float64))["logits"].reshape(4, 6)
    assert max_err_scaled(scores.numpy(), ref) < 1e-5


def test_top_k_argument_validation():
    m, _ = _model()
    rng = np.random.default_rng(2)
    qi, ci = _ids(rng, [0, 1], 3), _ids(rng, [2, 3, 4, 5], 4)
    for bad in ([0, 0], [0, 6], [-1, 1], [], list(range(6))):
        with pytest.raises(ValueError):
            m.top_k(qi, ci, bad, 2)
    for k in (0, 257):
        with pytest.raises(ValueError):
            m.top_k(qi, ci, [0, 1], k)
    with pytest.raises(ValueError):
        m.top_k(qi.long(), ci, [0, 1], 2)                       # dtype
    with pytest.raises(ValueError):
        m.top_k(qi[:, :1].contiguous(), ci, [0, 1], 2)           # width
    with pytest.raises(ValueError):
        m.top_k(qi, ci, [0, 1], 2, query_x=torch.zeros(3, 1))    # no numeric column on that side
    with pytest.raises(ValueError):
        m.top_k(qi, ci, [0, 1], 2, exclude=[[0]])                # one row per query
    with pytest.raises(ValueError):
        m.top_k(qi, ci, [0, 1], 2, exclude=[[0], [4], []])       # candidate index out of range
    with pytest.raises(ValueError):
        m.top_k(qi, ci, [0, 1], 2, exclude=(np.array([0, 1, 1]), np.array([0], np.int32)))   # offsets [U + 1]
    s, i = m.top_k(qi, ci, [0, 1], 3, exclude=[[0, 1, 2, 3], [1], []])
    assert (i.numpy()[0] == -1).all() and np.isneginf(s.numpy()[0]).all() and 1 not in i.numpy()[1]
    m.shard = object()                                           # a row-sharded engine
    with pytest.raises(NotImplementedError):
        m.top_k(qi, ci, [0, 1], 2)


def test_features_split_into_sides_by_key():
    cols = ml_100k.get_feature_columns(4)
    plan = FieldPlan(cols["linear"])
    names = [c.name for c in plan.categorical]
    user = {k: [1] for k in recommend.QUERY_KEYS}
    item = {k: [1] for k in ["item_id", "release_year"] + ml_100k.GENRE}
    qf = split_sides(plan, user, item)
    assert sorted(names[f] for f in qf) == sorted(["user_id", "age_bucketized", "gender", "occupation", "zipcode"])
    with pytest.raises(ValueError, match="both"):
        split_sides(plan, dict(user, item_id=[1]), item)
    with pytest.raises(ValueError, match="neither"):
        split_sides(plan, user, {k: v for k, v in item.items() if k != "action"})


def test_cli_tables_and_exclusions():
    train = {"user_id": np.array([3, 1, 3, 2]), "item_id": np.array([20, 10, 30, 20]), "age": np.array([30, 40, 31, 50]),
             "gender": np.array(["M", "F", "F", "M"], object), "occupation": np.array(["a", "b", "c", "d"], object),
             "zipcode": np.array(["1", "2", "3", "4"], object), "release_year": np.array([1990, 1980, 1970, 1991]),
             "rating": np.array([5, 1, 2, 3])}
    test = {k: v[[1, 0]].copy() for k, v in train.items()}
    test["item_id"] = np.array([40, 10])
    users, qf, items, cf = recommend.tables(train, test)
    assert users.tolist() == [1, 3]
    assert qf["age"].tolist() == [40, 30] and qf["gender"].tolist() == ["F", "M"]   # first test row of each user
    assert set(qf) == set(recommend.QUERY_KEYS) and not set(qf) & set(cf)
    assert items.tolist() == [10, 20, 30, 40]
    assert cf["release_year"].tolist() == [1980, 1990, 1970, 1980]                   # first row of train + test
    off, idx = recommend.exclusion_csr(users, items, train)
    assert off.tolist() == [0, 1, 3] and idx.tolist() == [0, 1, 2]                   # user 1: item 10; user 3: items 20, 30


def test_ranking_metrics_hand_computed():
    top = {1: [5, 6, 7], 2: [8, 9, 10], 3: [1, 2, 3]}
    pos = {1: {6, 11}, 2: {12}, 3: {1, 3}, 4: set()}
    m = recommend.ranking_metrics(top, pos, 3)
    assert m["users"] == 3
    assert m["hit_rate@3"] == pytest.approx(2 / 3)
    assert m["recall@3"] == pytest.approx((0.5 + 0 + 1) / 3)
    d1 = (1 / math.log2(3)) / (1 + 1 / math.log2(3))
    d3 = (1 + 1 / math.log2(4)) / (1 + 1 / math.log2(3))
    assert m["ndcg@3"] == pytest.approx((d1 + 0 + d3) / 3)


def _write_rows(path, rng, n, users, items):
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(ml_100k.COLUMNS)
        for _ in range(n):
            u, i = int(rng.choice(users)), int(rng.choice(items))
            g = {k: int((i * 7 + j) % 3 == 0) for j, k in enumerate(ml_100k.GENRE)}
            r = dict(user_id=u, item_id=i, rating=5 if g["action"] else int(rng.integers(1, 5)), age=20 + u % 40,
                     gender="MF"[u % 2], occupation=["student", "engineer"][u % 2], zipcode="%05d" % (u * 37),
                     release_year=1930 + i % 60, **g)
            w.writerow([r.get(c, 0 if d[0] == 0 else "null") for c, d in zip(ml_100k.COLUMNS, ml_100k.DEFAULTS)])


@pytest.mark.parametrize("model", ["deep_fm", "linear", "deep", "linear_deep"])
def test_recommend_cli_every_model(tmp_path, monkeypatch, model):
    """the CLI's path (make_estimator, checkpoint restore, Estimator.recommend, recommend_batch) for DeepFM and the three
    canned classifiers, kernels stood in by numpy: K rows per test user, no training item, logits = Estimator.predict"""
    import csv
    import json
    from mi355x_rec import engine
    from trainers import _cli
    from trainers.conf_utils import get_run_config
    monkeypatch.setattr(engine, "HipKernels", NumpyKernels)
    rng = np.random.default_rng(3)
    users, items = np.arange(1, 13), np.arange(1, 31)
    _write_rows(tmp_path / "train.csv", rng, 200, users, items)
    _write_rows(tmp_path / "test.csv", rng, 40, users[:8], items)
    trainer, opt = recommend.MODELS[model]
    job = str(tmp_path / "job")
    base = ["--train-csv", str(tmp_path / "train.csv"), "--test-csv", str(tmp_path / "test.csv"), "--job-dir", job,
            "--device", "cpu"]
    trainer.train_and_evaluate(_cli.make_parser(model, opt).parse_args(base + ["--train-steps", "20"]))
    K = 4
    metrics = recommend.main(["--model", model] + base + ["--top-k", str(K)])
    assert {"hit_rate@4", "recall@4", "ndcg@4"} <= set(metrics)
    assert set(json.load(open(os.path.join(job, "recommend", "top4_metrics.json")))) == set(metrics)
    rows = list(csv.DictReader(open(os.path.join(job, "recommend", "top4.csv"))))
    train, _ = ml_100k._read_csv(str(tmp_path / "train.csv"))
    test, _ = ml_100k._read_csv(str(tmp_path / "test.csv"))
    u_ids, qf, i_ids, cf = recommend.tables(train, test)
    assert len(rows) == K * len(u_ids)
    seen = set(zip(train["user_id"].tolist(), train["item_id"].tolist()))
    assert not any((int(r["user_id"]), int(r["item_id"])) in seen for r in rows)
    est = trainer.make_estimator(_cli.make_parser(model, opt).parse_args(base), ml_100k.get_feature_columns(4), get_run_config())
    est.params["device"] = "cpu"
    ui = {int(u): j for j, u in enumerate(u_ids)}
    ii = {int(i): j for j, i in enumerate(i_ids)}
    feats = {}
    for r in rows:
        for k_, v in qf.items():
            feats.setdefault(k_, []).append(v[ui[int(r["user_id"])]])
        for k_, v in cf.items():
            feats.setdefault(k_, []).append(v[ii[int(r["item_id"])]])
    feats = {k_: np.asarray(v, dtype=object if isinstance(v[0], str) else None) for k_, v in feats.items()}
    want = np.asarray([p["logits"][0] for p in est.predict(lambda: iter([feats]))], np.float64)
    got = np.asarray([float(r["logit"]) for r in rows])
    assert max_err_scaled(got, want) < 1e-5
