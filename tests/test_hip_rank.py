"""GPU: top-K recommendation (mi_pair_topk, DeepFM.top_k, Estimator.recommend, python -m trainers.recommend).

Pair scores against the fp64 oracle on the explicit cross product, the selection bit for bit against a host sort of the
kernel's own scores, DeepFM.top_k against the engine's own forward after lazily-updated Adam steps, and the CLI end to
end."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mi355x_rec.engine import DeepFM, OptimizerSpec
from oracle import deepfm as O
from tests.cases import RANK_CASES, VOCAB26
from tests.util import host_topk, make_problem, max_err_scaled

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "recommender-tensorflow_amd")
Q5 = [0, 1, 2, 3, 4]


def _sides(rng, vocab, qf, U, I, n_numeric=0):
    F = len(vocab)
    cat_q = [f for f in qf if f < F]
    cat_c = [f for f in range(F) if f not in qf]
    num_q = [j for j in range(n_numeric) if F + j in qf]
    num_c = [j for j in range(n_numeric) if F + j not in qf]
    qid = np.stack([rng.integers(0, vocab[f], U) for f in cat_q], 1).astype(np.int32)
    cid = np.stack([rng.integers(0, vocab[f], I) for f in cat_c], 1).astype(np.int32)
    qx = rng.standard_normal((U, len(num_q))).astype(np.float32) if num_q else None
    cx = rng.standard_normal((I, len(num_c))).astype(np.float32) if num_c else None
    return (cat_q, cat_c, num_q, num_c), qid, cid, qx, cx


def _pairs(parts, qid, cid, qx, cx, F, n_numeric):
    """the explicit cross product: ids [U*I, F] and x [U*I, n_numeric] (pair (u, i) at row u*I + i)"""
    cat_q, cat_c, num_q, num_c = parts
    U, I = qid.shape[0], cid.shape[0]
    ids = np.zeros((U * I, F), np.int32)
    ids[:, cat_q] = np.repeat(qid, I, 0)
    ids[:, cat_c] = np.tile(cid, (U, 1))
    x = None
    if n_numeric:
        x = np.zeros((U * I, n_numeric), np.float32)
        if num_q:
            x[:, num_q] = np.repeat(qx, I, 0)
        if num_c:
            x[:, num_c] = np.tile(cx, (U, 1))
    return ids, x


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(m, parts, qid, cid, qx, cx, qf, k=10, exclude=None):
    return m.top_k(_t(qid), _t(cid), qf, k, _t(qx), _t(cx), exclude=exclude, return_scores=True)


@pytest.mark.parametrize("E,hidden,act,flags,U,I", RANK_CASES)
def test_pair_scores_match_oracle(E, hidden, act, flags, U, I):
    use_linear, use_mf, use_dnn = flags
    p, _, _, _ = make_problem(3, VOCAB26, E, hidden, 4, use_dnn=use_dnn)
    m = DeepFM(VOCAB26, embedding_size=E, hidden_units=hidden, use_linear=use_linear, use_mf=use_mf, use_dnn=use_dnn,
               activation=act, device="cuda")
    m.load_oracle_params(p)
    rng = np.random.default_rng(U * 7 + I)
    parts, qid, cid, qx, cx = _sides(rng, VOCAB26, Q5, U, I)
    score, idx, scores = _run(m, parts, qid, cid, qx, cx, Q5, k=min(10, I))
    ids, _ = _pairs(parts, qid, cid, qx, cx, 26, 0)
    ref = O.forward(p.astype(np.float64), ids, use_linear=use_linear, use_mf=use_mf, use_dnn=use_dnn,
                    activation=act if act != "identity" else None)["logits"].reshape(U, I)
    err = max_err_scaled(scores.cpu().numpy(), ref)
    assert err < 1e-5, err


@pytest.mark.parametrize("numeric,qf", [("embed", [0, 3, 6]), ("raw", [1, 2, 7])])
def test_pair_scores_numeric_columns(numeric, qf):
    vocab = VOCAB26[:6]
    p, _, _, _ = make_problem(5, vocab, 4, [16, 16], 4, n_numeric=2, use_dnn=True)
    use_mf = numeric == "embed"
    if numeric == "raw":
        k0, b0 = p.mlp[0]
        rng0 = np.random.default_rng(1)
        p.mlp[0] = (np.concatenate([k0[:6 * 4], (rng0.standard_normal((2, k0.shape[1])) * 0.3).astype(np.float32)]), b0)
    m = DeepFM(vocab, n_numeric=2, embedding_size=4, hidden_units=[16, 16], use_mf=use_mf, numeric=numeric, device="cuda")
    m.load_oracle_params(p)
    rng = np.random.default_rng(2)
    parts, qid, cid, qx, cx = _sides(rng, vocab, qf, 19, 77, n_numeric=2)
    _, _, scores = _run(m, parts, qid, cid, qx, cx, qf)
    ids, x = _pairs(parts, qid, cid, qx, cx, 6, 2)
    ref = O.forward(p.astype(np.float64), ids, x.astype(np.float64), use_mf=use_mf, numeric=numeric)["logits"].reshape(19, 77)
    assert max_err_scaled(scores.cpu().numpy(), ref) < 1e-5


def test_pair_scores_canned_wide_and_deep():
    """DNNLinearCombinedClassifier with narrower embedding columns and columns outside the wide part"""
    vocab = VOCAB26[:8]
    dims = [4, 2, 4, 3, 4, 1, 4, 4]
    wide = [True, False, True, True, False, True, True, False]
    rng = np.random.default_rng(4)
    p, _, _, _ = make_problem(6, vocab, 4, [16, 8], 4, use_dnn=True)
    p.emb = [a[:, :d].copy() for a, d in zip(p.emb, dims)]
    k0, b0 = p.mlp[0]
    keep = [f * 4 + j for f, d in enumerate(dims) for j in range(d)]
    p.mlp[0] = (k0[keep].copy(), b0)
    p.lin_w = [w if on else np.zeros_like(w) for w, on in zip(p.lin_w, wide)]
    m = DeepFM(vocab, embedding_size=4, hidden_units=[16, 8], use_mf=False, reduction="sum", field_dims=dims,
               wide_fields=wide, device="cuda")
    m.load_oracle_params(p)
    qf = [0, 5]
    parts, qid, cid, qx, cx = _sides(rng, vocab, qf, 21, 90)
    _, _, scores = _run(m, parts, qid, cid, qx, cx, qf)
    ids, _ = _pairs(parts, qid, cid, qx, cx, 8, 0)
    ref = O.forward(p.astype(np.float64), ids, use_mf=False, wide_fields=wide)["logits"].reshape(21, 90)
    assert max_err_scaled(scores.cpu().numpy(), ref) < 1e-5


@pytest.mark.parametrize("k,I", [(1, 300), (10, 300), (100, 300), (256, 300), (100, 50), (256, 131)])
def test_selection_bit_for_bit(k, I):
    p, _, _, _ = make_problem(7, VOCAB26, 4, [16, 16], 4)
    m = DeepFM(VOCAB26, embedding_size=4, hidden_units=[16, 16], device="cuda")
    m.load_oracle_params(p)
    rng = np.random.default_rng(k + I)
    U = 37
    parts, qid, cid, qx, cx = _sides(rng, VOCAB26, Q5, U, I)
    cid[I // 2] = cid[3]                        # equal candidates: equal scores, decided by the index
    cid[I - 1] = cid[3]
    excl = [sorted(set(rng.integers(0, I, rng.integers(0, I // 3 + 1)).tolist())) for _ in range(U)]
    excl[5] = list(range(I))                    # every candidate excluded
    excl[6] = []
    score, idx, scores = _run(m, parts, qid, cid, qx, cx, Q5, k=k, exclude=excl)
    s_ref, i_ref = host_topk(scores.cpu().numpy(), k, excl)
    got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(got_i, i_ref)
    assert np.array_equal(got_s.view(np.uint32), s_ref.view(np.uint32))
    for u in range(U):
        assert not set(got_i[u].tolist()) & set(excl[u])
    assert (got_i[5] == -1).all() and np.isneginf(got_s[5]).all()
    # the same selection through the CSR form of the exclusions
    off = np.concatenate([[0], np.cumsum([len(r) for r in excl])]).astype(np.int64)
    ix = np.asarray([c for r in excl for c in r], np.int32)
    s2, i2 = m.top_k(_t(qid), _t(cid), Q5, k, exclude=(off, ix))
    assert np.array_equal(i2.cpu().numpy(), got_i) and np.array_equal(s2.cpu().numpy().view(np.uint32), got_s.view(np.uint32))


def test_selection_mfma_path_bit_for_bit():
    p, _, _, _ = make_problem(8, VOCAB26, 64, [512, 256, 128], 4)
    m = DeepFM(VOCAB26, embedding_size=64, hidden_units=[512, 256, 128], device="cuda")
    m.load_oracle_params(p)
    rng = np.random.default_rng(9)
    parts, qid, cid, qx, cx = _sides(rng, VOCAB26, Q5, 40, 700)
    excl = [sorted(set(rng.integers(0, 700, 50).tolist())) for _ in range(40)]
    score, idx, scores = _run(m, parts, qid, cid, qx, cx, Q5, k=100, exclude=excl)
    s_ref, i_ref = host_topk(scores.cpu().numpy(), 100, excl)
    assert np.array_equal(idx.cpu().numpy(), i_ref)
    assert np.array_equal(score.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))


@pytest.mark.parametrize("k,U,I", [(256, 37, 100000), (60, 64, 40000)])
def test_selection_under_heavy_survivor_traffic(k, U, I):
    """candidates in ascending score order: every candidate beats the K-th of its query, so every one is appended and
    the survivor slots fill every 15 rounds (thousands of candidates per split, merges back to back)"""
    vocab = [7, I]
    m = DeepFM(vocab, use_mf=False, use_dnn=False, device="cuda")
    rng = np.random.default_rng(k)
    lin = [rng.standard_normal(7).astype(np.float32) * 0.01, np.arange(I, dtype=np.float32) * np.float32(1e-3)]
    lin[1][I // 3:I // 3 + 50] = lin[1][I // 3]                 # ties inside the stream
    m.lin_w.copy_(torch.from_numpy(np.concatenate(lin)).cuda())
    qid = rng.integers(0, 7, (U, 1)).astype(np.int32)
    cid = np.arange(I, dtype=np.int32).reshape(I, 1)
    excl = [sorted(set(rng.integers(I - 3 * k, I, k // 2).tolist())) for _ in range(U)]
    s1, i1, scores = m.top_k(_t(qid), _t(cid), [0], k, exclude=excl, return_scores=True)
    s_ref, i_ref = host_topk(scores.cpu().numpy(), k, excl)
    assert np.array_equal(i1.cpu().numpy(), i_ref)
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    for _ in range(2):
        s2, i2 = m.top_k(_t(qid), _t(cid), [0], k, exclude=excl)
        assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))


@pytest.mark.parametrize("E,hidden", [(4, [16, 16]), (64, [512, 256, 128])])
def test_top_k_matches_engine_forward_after_lazy_adam(E, hidden):
    vocab = [50 + 3 * i for i in range(26)]
    rng = np.random.default_rng(11)
    p, _, _, _ = make_problem(12, vocab, E, hidden, 4)
    m = DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=OptimizerSpec("Adam", 0.01), device="cuda")
    m.load_oracle_params(p)
    for _ in range(4):                          # small batches: most rows sit out most steps (lazy catch-up)
        ids = np.stack([rng.integers(0, v, 16) for v in vocab], 1).astype(np.int32)
        y = (rng.random(16) < 0.4).astype(np.uint8)
        m.train_step(_t(ids), _t(y))
    U, I = 23, 61
    parts, qid, cid, qx, cx = _sides(rng, vocab, Q5, U, I)
    s1, i1, sc1 = _run(m, parts, qid, cid, qx, cx, Q5, k=20)
    ids, _ = _pairs(parts, qid, cid, qx, cx, 26, 0)
    ref = m.predict_logits(_t(ids)).cpu().numpy().reshape(U, I)
    assert max_err_scaled(sc1.cpu().numpy(), ref) < 1e-5
    got = s1.cpu().numpy()
    sel = np.take_along_axis(ref, i1.cpu().numpy().astype(np.int64), 1)
    assert max_err_scaled(got, sel) < 1e-5
    s2, i2, sc2 = _run(m, parts, qid, cid, qx, cx, Q5, k=20)
    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert torch.equal(sc1.view(torch.int32), sc2.view(torch.int32))


# ---- end to end: train, then python -m trainers.recommend -----------------------------------------------------------
def _write_csv(path, rows):
    from trainers import ml_100k
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(ml_100k.COLUMNS)
        for r in rows:
            w.writerow([r.get(c, 0 if d[0] == 0 else "null") for c, d in zip(ml_100k.COLUMNS, ml_100k.DEFAULTS)])


def _rows(rng, n, users, items):
    from trainers import ml_100k
    out = []
    for _ in range(n):
        u, i = int(rng.choice(users)), int(rng.choice(items))
        g = {k: int((i * 7 + j) % 3 == 0) for j, k in enumerate(ml_100k.GENRE)}
        out.append(dict(user_id=u, item_id=i, rating=5 if g["action"] else int(rng.integers(1, 5)), age=20 + u % 40,
                        gender="MF"[u % 2], occupation=["student", "engineer", "none"][u % 3], zipcode="%05d" % (u * 37),
                        release_year=1930 + i % 60, **g))
    return out


def _run_cli(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([PKG, ROOT])
    r = subprocess.run([sys.executable, "-m", "trainers.recommend"] + args, cwd=PKG, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("model", ["deep_fm", "linear", "deep", "linear_deep"])
def test_recommend_cli_end_to_end(tmp_path, model):
    from trainers import _cli
    from trainers.recommend import MODELS
    from trainers.ml_100k import get_feature_columns
    from trainers.conf_utils import get_run_config
    rng = np.random.default_rng(0)
    users, items = np.arange(1, 41), np.arange(1, 121)
    train, test = _rows(rng, 800, users, items), _rows(rng, 120, users[:25], items)
    _write_csv(tmp_path / "train.csv", train)
    _write_csv(tmp_path / "test.csv", test)
    job = str(tmp_path / "job")
    trainer, opt = MODELS[model]
    base = ["--train-csv", str(tmp_path / "train.csv"), "--test-csv", str(tmp_path / "test.csv"), "--job-dir", job]
    trainer.train_and_evaluate(_cli.make_parser(model, opt).parse_args(base + ["--train-steps", "60"]))
    K = 7
    _run_cli(["--model", model] + base + ["--top-k", str(K)])
    out = os.path.join(job, "recommend", "top%d.csv" % K)
    rows = list(csv.DictReader(open(out)))
    test_users = sorted({r["user_id"] for r in test})
    per_user = {}
    for r in rows:
        per_user.setdefault(int(r["user_id"]), []).append(r)
    assert sorted(per_user) == test_users and all(len(v) == K for v in per_user.values())
    seen = {}
    for r in train:
        seen.setdefault(r["user_id"], set()).add(r["item_id"])
    assert all(int(r["item_id"]) not in seen.get(int(r["user_id"]), set()) for r in rows)
    metrics = json.load(open(os.path.join(job, "recommend", "top%d_metrics.json" % K)))
    assert {"hit_rate@%d" % K, "recall@%d" % K, "ndcg@%d" % K} <= set(metrics)
    # a handful of (user, item) logits against Estimator.predict on those pairs
    config = get_run_config()
    est = trainer.make_estimator(_cli.make_parser(model, opt).parse_args(base), get_feature_columns(4), config)
    first_u = {}
    for r in test:
        first_u.setdefault(r["user_id"], r)
    first_i = {}
    for r in train + test:
        first_i.setdefault(r["item_id"], r)
    from trainers.recommend import QUERY_KEYS
    pick = rows[::max(1, len(rows) // 6)][:6]
    feats = {}
    for r in pick:
        u, i = first_u[int(r["user_id"])], first_i[int(r["item_id"])]
        row = {c: (u[c] if c in QUERY_KEYS else i[c]) for c in set(u) | set(i) if c != "rating"}
        for c, v in row.items():
            feats.setdefault(c, []).append(v)
    feats = {c: np.asarray(v, dtype=object if isinstance(v[0], str) else np.int32) for c, v in feats.items()}
    pred = list(est.predict(lambda: iter([feats])))
    got = np.asarray([float(r["logit"]) for r in pick])
    want = np.asarray([float(p["logits"][0]) for p in pred])
    assert max_err_scaled(got, want) < 1e-5, (got, want)
    # --include-seen: training items may come back
    _run_cli(["--model", model] + base + ["--top-k", str(K), "--include-seen", "--output", str(tmp_path / "all.csv")])
    assert len(list(csv.DictReader(open(tmp_path / "all.csv")))) == K * len(test_users)
