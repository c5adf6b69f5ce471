"""CPU: the host side of exact target ranks under an ensemble's MEAN logit — engine.target_ranks_mean (ragged targets, passes
of 64 columns, what it does once per call), EnsemblePredictor.rank_targets (its modes and refusals), trainers.sweep
--ensemble N --rank-metrics and trainers.recommend --top N --mean-metrics-at.  mi_pair_target_ranks_mean is stood in by a
numpy restatement of its definition in include/mi355x_rec.h (tests.rank_kernels.RankKernels: the mean in fp32 in
member order, the rank counted, not read off a sorted list); the real kernel is tested in test_hip_target_ranks_mean.py.  The
binding and the library's host-side refusals are checked against the real library."""
import json

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from mi355x_rec.engine import DeepFM
from mi355x_rec.predictor import EnsemblePredictor, Predictor
from tests.cases import _sweep_args
from tests.rank_kernels import RankKernels, oracle_ranks, rank_kernels  # noqa: F401  (rank_kernels: a fixture)
from tests.util import _header_decls, _train_deep_fm_export, make_problem
from trainers import ml_100k, recommend

VOCAB = [11, 7, 5, 9, 13, 6]
QF, CF = [1, 4], [0, 2, 3, 5]


def _model(seed, E, hidden, **kw):
    m = DeepFM(VOCAB, embedding_size=E, hidden_units=hidden, device="cpu", _kernels=RankKernels(), **kw)
    p, _, _, _ = make_problem(seed, VOCAB, E, hidden, 4, use_dnn=kw.get("use_dnn", True))
    m.load_oracle_params(p)
    return m


def _ids(rng, fields, n):
    return torch.from_numpy(np.stack([rng.integers(0, VOCAB[f], n) for f in fields], 1).astype(np.int32))


@pytest.fixture(scope="module")
def problem():
    """3 members, U = 37, I = 131; 0, 1, 5 and 70 targets per query (70: two passes); duplicate candidates, an excluded target,
    a target >= I, a padding -1 inside a row, a duplicate target, one query with everything excluded"""
    rng = np.random.default_rng(11)
    U, I = 37, 131
    qi, ci = _ids(rng, QF, U), _ids(rng, CF, I)
    ci[I // 2] = ci[3]                                   # equal candidates: equal scores, decided by the index
    ci[I - 1] = ci[3]
    excl = [sorted(set(rng.integers(0, I, int(rng.integers(0, I // 3 + 1))).tolist())) for _ in range(U)]
    excl[5] = list(range(I))
    excl[6] = []
    targets = [rng.choice(I, (0, 1, 5, 70)[u % 4], replace=False).tolist() for u in range(U)]
    targets[2] = [3, I // 2, I - 1, 3, 40]               # the equal candidates, one of them twice
    targets[6] = [7, I, -1, 9, I + 5]                    # not a candidate, padding in the middle
    targets[9] = [excl[9][0]] if excl[9] else [0]        # an excluded target
    targets[5] = [1, 2, 3, 4, 5]                         # every candidate of this query is excluded
    members = [_model(1, 4, [8, 4]), _model(2, 8, [16]), _model(3, 4, [], use_dnn=False)]
    return members, qi, ci, excl, targets


def test_ranks_equal_the_host_oracle_on_the_group_scores(problem):
    members, qi, ci, excl, targets = problem
    counted = {"sides": 0}
    real = DeepFM._top_k_sides
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(DeepFM, "_top_k_sides", lambda self, *a: counted.__setitem__("sides", counted["sides"] + 1) or real(self, *a))
        members[0].k.calls.clear()
        ranks, scores = engine.target_ranks_mean(members, qi, ci, QF, targets, exclude=excl, return_scores=True)
    assert tuple(ranks.shape) == (37, 70) and ranks.dtype == torch.int32 and tuple(scores.shape) == (37, 70)
    assert members[0].k.calls["mi_pair_target_ranks_mean"] == 2 and counted["sides"] == 3    # two passes, the sides once per member
    z = engine.top_k_group(members, qi, ci, QF, 1, return_scores=True)[2].numpy()
    want = oracle_ranks(z, targets, excl)
    assert np.array_equal(ranks.numpy(), want)
    got_s = scores.numpy()
    for u in range(37):
        for j, t in enumerate(targets[u]):
            assert (np.isnan(got_s[u, j]) if want[u, j] < 0 else got_s[u, j] == z[u, t]), (u, j)
    assert np.isnan(got_s[want < 0]).all()
    # the cases the problem was built for
    assert want[2, 0] == want[2, 3] and want[2, 2] > want[2, 1] > want[2, 0] and (want[6, [1, 2, 4]] == -1).all() and want[6, 0] >= 0
    assert want[9, 0] == -1 and (want[5] == -1).all() and (want[0] == -1).all()
    assert (want >= 0).sum() > 0.6 * sum(len(t) for t in targets)
    # the mean's order is no member's own
    own = engine.target_ranks_group(members, qi, ci, QF, targets, exclude=excl).numpy()
    assert all(not np.array_equal(own[i], want) for i in range(3))
    # the CSR form of targets and of the exclusions, without the scores: the same integers
    off = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
    idx = np.asarray([c for t in targets for c in t], np.int64)
    eo = np.concatenate([[0], np.cumsum([len(r) for r in excl])]).astype(np.int64)
    ei = np.asarray([c for r in excl for c in r], np.int32)
    assert torch.equal(engine.target_ranks_mean(members, qi, ci, QF, (off, idx), exclude=(eo, ei)), ranks)
    # a group of one is that member's own ranking (z / 1.0f is exact); no query with a target: no launch, no column
    assert torch.equal(engine.target_ranks_mean(members[1:2], qi, ci, QF, targets, exclude=excl), torch.from_numpy(own[1]))
    assert tuple(engine.target_ranks_mean(members, qi, ci, QF, [[] for _ in range(37)]).shape) == (37, 0)
    # the member order is part of the definition: the reversed group against ITS scores
    back = members[::-1]
    zb = engine.top_k_group(back, qi, ci, QF, 1, return_scores=True)[2].numpy()
    assert np.array_equal(engine.target_ranks_mean(back, qi, ci, QF, targets, exclude=excl).numpy(), oracle_ranks(zb, targets, excl))


def test_arguments_are_validated(problem):
    members, qi, ci, excl, targets = problem
    with pytest.raises(ValueError, match="targets: 36 rows for 37 queries"):
        engine.target_ranks_mean(members, qi, ci, QF, targets[:-1])
    with pytest.raises(ValueError, match="target_ranks_mean: member 1: the model has a hidden layer of 64 units"):
        engine.target_ranks_mean([members[0], _model(4, 4, [64, 64])], qi, ci, QF, targets)
    with pytest.raises(ValueError, match="target_ranks_mean: no members"):
        engine.target_ranks_mean([], qi, ci, QF, targets)


@pytest.fixture(scope="module")
def exports(tmp_path_factory):
    """three small trained deep_fm exports: two inside the kernel's scope, one ([64, 64]) outside it"""
    root = str(tmp_path_factory.mktemp("rankmean"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine, "HipKernels", RankKernels)
        return [_train_deep_fm_export(root, "a", ["--embedding-size", "4", "--hidden-units", "8", "8"]),
                _train_deep_fm_export(root, "b", ["--embedding-size", "8", "--hidden-units", "8"]),
                _train_deep_fm_export(root, "c", ["--embedding-size", "4", "--hidden-units", "64", "64"])]


@pytest.fixture(scope="module")
def sides():
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:30:2")
    users, qf, items, cf = recommend.tables(train, test)
    return qf, cf, recommend.positive_targets(users, items, test), recommend.exclusion_csr(users, items, train), len(items)


def test_ensemble_rank_targets_fused_and_layered_give_equal_integers(rank_kernels, exports, sides):
    qf, cf, targets, excl, I = sides
    ens = EnsemblePredictor([Predictor.from_export(d, device="cpu") for d in exports[:2]])
    k = ens.k
    k.calls.clear()
    fused, fs = ens.rank_targets(qf, cf, targets, exclude=excl, mode="fused", return_scores=True)
    assert k.calls.get("mi_pair_target_ranks_mean", 0) == 1 and "mi_pair_topk" not in k.calls
    layered, ls = ens.rank_targets(qf, cf, targets, exclude=excl, mode="layered", return_scores=True)
    assert fused.dtype == np.int32 and fused.shape == (len(targets), max(len(t) for t in targets))
    assert np.array_equal(fused, layered) and np.array_equal(fs.view(np.uint32), ls.view(np.uint32))
    assert np.array_equal(ens.rank_targets(qf, cf, targets, exclude=excl), fused)            # auto: every member in scope
    assert (fused >= 0).sum() >= 0.9 * sum(len(t) for t in targets) > 0 and fused.max() < I
    # the rank says where the target stands in recommend's list
    top = ens.recommend(qf, cf, 20, exclude=excl, mode="fused")["indices"]
    for u, row in enumerate(targets):
        for j, t in enumerate(row):
            assert (top[u, fused[u, j]] == t) if 0 <= fused[u, j] < 20 else (t not in top[u]), (u, j)
    # a member outside the scope: fused names it, auto is layered
    mixed = EnsemblePredictor([Predictor.from_export(exports[i], device="cpu") for i in (0, 2)])
    with pytest.raises(ValueError, match=r"mode='fused': member 1: the model has a hidden layer of 64 units after the first \(below 32\)"):
        mixed.rank_targets(qf, cf, targets, mode="fused")
    for p in mixed.members:
        p.engine.k.calls.clear()
    auto = mixed.rank_targets(qf, cf, targets, exclude=excl)
    assert all("mi_pair_target_ranks_mean" not in p.engine.k.calls and p.engine.k.calls.get("mi_pair_topk", 0) == 1
               for p in mixed.members)
    z = mixed.recommend(qf, cf, 1, exclude=excl, mode="layered", return_scores=True)["scores"]
    off, idx = excl
    assert np.array_equal(auto, oracle_ranks(z, targets, [idx[off[u]:off[u + 1]].tolist() for u in range(len(targets))]))
    with pytest.raises(ValueError, match="mode"):
        ens.rank_targets(qf, cf, targets, mode="eager")


def test_sweep_ranks_its_ensemble_as_recommend_does(rank_kernels, tmp_path, capsys, monkeypatch):
    from trainers import sweep
    real = EnsemblePredictor.from_sweep.__func__

    def registered(cls, *a, **kw):                       # (the stand-in of mi_predict_group finds a member's engine by register())
        ens = real(cls, *a, **kw)
        RankKernels.register([p.engine for p in ens.members])
        return ens
    monkeypatch.setattr(EnsemblePredictor, "from_sweep", classmethod(registered))
    job = tmp_path / "job"
    flags = ["--train-steps", "12", "--learning-rate", "0.001", "0.01", "--ensemble", "2"]
    sweep.train_and_evaluate(_sweep_args(job, "--rank-metrics", "5", "10", "--select", "ndcg@10", *flags))
    out = capsys.readouterr().out
    doc = json.load(open(job / "sweep.json"))
    ens, rows = doc["ensemble"], doc["members"]
    assert set(ens) == {"members", "metrics", "ranking"} and set(ens["ranking"]) == set(rows[0]["ranking"])
    assert ens["ranking"]["users"] == rows[0]["ranking"]["users"] > 0
    # the existing line (evaluation metrics) and the new one (the selected ranking metric against the best member's)
    assert "INFO: ensemble of the 2 best members (%s): auc = " % ", ".join(str(m) for m in ens["members"]) in out
    assert "INFO: ensemble of the 2 best members by its mean logit: ndcg@10 = %.6g, the best single member (member %d) has %.6g" % (
        ens["ranking"]["ndcg@10"], rows[0]["member"], rows[0]["ranking"]["ndcg@10"]) in out
    base = ["--model", "deep_fm", "--job-dir", str(job), "--synthetic", "300", "--device", "cpu", "--top-k", "5", "--top", "2"]
    before = recommend.main(base)
    m = recommend.main(base + ["--mean-metrics-at", "5", "10"])
    assert {key: m[key] for key in ens["ranking"]} == ens["ranking"]
    assert set(m) == set(before) | set(ens["ranking"]) and all(m[key] == before[key] for key in before)
    assert json.load(open(job / "recommend" / "top5_ensemble2_metrics.json")) == m
    # an evaluation --select: no second line; without --rank-metrics: no "ranking"
    sweep.train_and_evaluate(_sweep_args(job, "--rank-metrics", "5", *flags))
    assert "by its mean logit" not in capsys.readouterr().out
    assert set(json.load(open(job / "sweep.json"))["ensemble"]["ranking"]) == {"hit_rate@5", "recall@5", "ndcg@5", "mrr", "mean_rank", "users"}
    sweep.train_and_evaluate(_sweep_args(job, *flags))
    doc = json.load(open(job / "sweep.json"))
    assert set(doc["ensemble"]) == {"members", "metrics"} and all("ranking" not in r for r in doc["members"])
    # the flag's own refusals, and the old one's, word for word
    with pytest.raises(SystemExit, match="--mean-metrics-at 0 5: cutoffs are at least 1"):
        recommend.main(base + ["--mean-metrics-at", "0", "5"])
    with pytest.raises(SystemExit, match="--mean-metrics-at: needs --top N: .* --metrics-at"):
        recommend.main(base[:-2] + ["--mean-metrics-at", "5"])
    with pytest.raises(SystemExit, match="--metrics-at: not with --top 2"):
        recommend.main(base + ["--metrics-at", "5"])
    assert recommend.parse_args(base).mean_metrics_at is None


def _raw(keep, hidden_after):
    """mi_rank_member_t with layers 16 -> hidden_after -> 1 and pointers that a host-side refusal never follows"""
    ms = (_lib.RankMember * len(hidden_after))()
    for m, after in zip(ms, hidden_after):
        w = [16] + list(after) + [1]
        widths, off, o = np.asarray(w, np.int32), [], 0
        for a, b in zip(w[:-1], w[1:]):
            off += [o, o + a * b]
            o += a * b + b
        layer_off = np.asarray(off, np.int64)
        keep.extend([widths, layer_off])
        for name in ("a_q", "s_q", "w_q", "a_c", "s_c", "w_c", "dense"):
            setattr(m, name, 4096)
        m.layer_off, m.widths = layer_off.ctypes.data, widths.ctypes.data
        m.H1, m.E, m.n_layers, m.activation = 16, 4, len(w) - 1, 1
    return ms


def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    err = lambda: lib.mi_last_error().decode()
    keep = []
    ok = _raw(keep, [[16], [16]])
    U, I, Tq = 70, 333, 10
    size = lib.mi_pair_target_ranks_mean_workspace_bytes
    need = size(ok, 2, U, I, Tq)
    assert need > size(ok, 1, U, I, Tq) > 0 and size(ok, 2, U, I, 64) > need
    # the members are a loop, not a grid axis: one set of partial counts, so less than the per-member entry needs
    assert need < lib.mi_pair_target_ranks_workspace_bytes(ok, 2, U, I, Tq)
    assert size(ok, 0, U, I, Tq) == 0 and size(None, 2, U, I, Tq) == 0 and size(ok, 257, U, I, Tq) == 0
    assert size(ok, 2, U, I, 0) == 0 and size(ok, 2, U, I, 65) == 0
    call = lambda ms, M, tq=Tq, tg=8192, rk=8192, ws=8192, wsb=1 << 40, eo=None, ei=None: lib.mi_pair_target_ranks_mean(
        ms, M, U, I, eo, ei, tg, tq, rk, None, ws, wsb, None)
    assert call(ok, 0) == -1 and "pair_target_ranks_mean: 0 members (at least 1)" in err()
    assert call(ok, 257) == -2 and "257 members (at most 256" in err()
    assert call(_raw(keep, [[16], [64]]), 2) == -2 and "member 1:" in err() and "hidden width of 64" in err() and "below 32" in err()
    assert call(_raw(keep, [[16], [16, 16, 300]]), 2) == -1 and "member 1: pair_topk: hidden widths after layer 1" in err()
    for tq in (0, 65):
        assert call(ok, 2, tq=tq) == -1 and "Tq=%d targets per query (1 to 64" % tq in err()
    assert call(ok, 2, eo=8192) == -1 and "excl_off and excl_idx go together" in err()
    assert call(ok, 2, rk=None) == -1 and "targets / ranks" in err()
    assert call(ok, 2, tg=None) == -1 and "targets / ranks" in err()
    assert call(ok, 2, wsb=need - 1) == -1 and "pair_target_ranks_mean: workspace %d < %d bytes" % (need - 1, need) in err()
    assert call(ok, 2, ws=None) == -1 and "workspace" in err()
    assert call(None, 2) == -1 and "members" in err()
    # the per-member entry keeps its name in its messages
    assert lib.mi_pair_target_ranks(ok, 0, U, I, None, None, 8192, Tq, 8192, None, 8192, 1 << 40, None) == -1
    assert err().startswith("pair_target_ranks: 0 members")


def test_header_binding_and_library_agree_on_the_new_entry(lib):
    decls = _header_decls()
    for name, nargs in (("mi_pair_target_ranks_mean_workspace_bytes", 5), ("mi_pair_target_ranks_mean", 13)):
        assert decls[name] == nargs == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    # the argument types are the per-member entry's: the two entries differ in the shape of their outputs only
    for suffix in ("_workspace_bytes", ""):
        assert _lib.SIGNATURES["mi_pair_target_ranks_mean" + suffix] == _lib.SIGNATURES["mi_pair_target_ranks" + suffix]
    assert lib.mi_abi_version() == 21 == _lib.ABI_VERSION
