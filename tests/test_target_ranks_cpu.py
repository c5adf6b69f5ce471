"""CPU: the host side of exact target ranks — engine.target_ranks_group (ragged targets, passes of 64 columns, what it
does once per call), DeepFM.target_ranks' fallback outside the kernel's scope, metrics.ranking_metrics_from_ranks,
trainers.sweep --rank-metrics / --select and trainers.recommend --metrics-at.  mi_pair_target_ranks is stood in by a numpy
restatement of its definition in include/mi355x_rec.h (tests.rank_kernels.RankKernels: the rank is counted, not read off a
sorted list); the real kernel is tested in test_hip_target_ranks.py.  The binding and the library's host-side refusals are
checked against the real library."""
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from mi355x_rec.engine import DeepFM
from mi355x_rec.metrics import ranking_metrics_from_ranks
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


def test_ranks_equal_the_host_oracle(problem):
    members, qi, ci, excl, targets = problem
    counted = {"sides": 0}
    real = DeepFM._top_k_sides
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(DeepFM, "_top_k_sides", lambda self, *a: counted.__setitem__("sides", counted["sides"] + 1) or real(self, *a))
        members[0].k.calls.clear()
        ranks, scores = engine.target_ranks_group(members, qi, ci, QF, targets, exclude=excl, return_scores=True)
    assert tuple(ranks.shape) == (3, 37, 70) and ranks.dtype == torch.int32 and tuple(scores.shape) == (3, 37, 70)
    assert members[0].k.calls["mi_pair_target_ranks"] == 2 and counted["sides"] == 3      # two passes, the sides once per member
    eligible = 0
    for i, m in enumerate(members):
        z = m.top_k(qi, ci, QF, 1, return_scores=True)[2].numpy()
        want = oracle_ranks(z, targets, excl)
        assert np.array_equal(ranks[i].numpy(), want), i
        eligible += int((want >= 0).sum())
        got_s = scores[i].numpy()
        for u in range(37):
            for j, t in enumerate(targets[u]):
                assert (np.isnan(got_s[u, j]) if want[u, j] < 0 else got_s[u, j] == z[u, t]), (i, u, j)
        assert np.isnan(got_s[want < 0]).all()
        # the cases the problem was built for
        assert want[2, 0] == want[2, 3] and want[2, 1] > want[2, 0] and (want[6, [1, 2, 4]] == -1).all() and want[6, 0] >= 0
        assert want[9, 0] == -1 and (want[5] == -1).all() and (want[0] == -1).all()
    assert eligible > 0.6 * 3 * sum(len(t) for t in targets)
    # the CSR form of targets and of the exclusions, without the scores: the same integers
    off = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
    idx = np.asarray([c for t in targets for c in t], np.int64)
    eo = np.concatenate([[0], np.cumsum([len(r) for r in excl])]).astype(np.int64)
    ei = np.asarray([c for r in excl for c in r], np.int32)
    again = engine.target_ranks_group(members, qi, ci, QF, (off, idx), exclude=(eo, ei))
    assert torch.equal(again, ranks)
    # one model is a group of one; no query with a target: no launch, no column
    own = members[1].target_ranks(qi, ci, QF, targets, exclude=excl, mode="fused")
    assert torch.equal(own, ranks[1])
    assert tuple(engine.target_ranks_group(members, qi, ci, QF, [[] for _ in range(37)]).shape) == (3, 37, 0)


def test_targets_are_validated(problem):
    members, qi, ci, excl, targets = problem
    with pytest.raises(ValueError, match="targets: 36 rows for 37 queries"):
        engine.target_ranks_group(members, qi, ci, QF, targets[:-1])
    with pytest.raises(ValueError, match="targets: offsets"):
        engine.target_ranks_group(members, qi, ci, QF, (np.zeros(37, np.int64), np.zeros(0, np.int32)))
    with pytest.raises(ValueError, match="member 1: the model has a hidden layer of 64 units"):
        engine.target_ranks_group([members[0], _model(4, 4, [64, 64])], qi, ci, QF, targets)
    with pytest.raises(ValueError, match="mode"):
        members[0].target_ranks(qi, ci, QF, targets, mode="layered")


def test_a_model_outside_the_scope_falls_back_to_its_own_scores(problem):
    _, qi, ci, excl, targets = problem
    m = _model(4, 4, [64, 64])
    with pytest.raises(ValueError, match=r"mode='fused': the model has a hidden layer of 64 units after the first \(below 32\)"):
        m.target_ranks(qi, ci, QF, targets, mode="fused")
    m.k.calls.clear()
    ranks, scores = m.target_ranks(qi, ci, QF, targets, exclude=excl, return_scores=True)
    assert "mi_pair_target_ranks" not in m.k.calls and m.k.calls["mi_pair_topk"] == 1
    z = m.top_k(qi, ci, QF, 1, return_scores=True)[2].numpy()
    want = oracle_ranks(z, targets, excl)
    assert ranks.dtype == torch.int32 and np.array_equal(ranks.numpy(), want)
    assert np.isnan(scores.numpy()[want < 0]).all() and scores[2, 0] == z[2, 3]
    # NaN below every number and -0 as +0, in the fallback's torch keys as in the header
    keys = torch.tensor([[1.0, float("nan"), -0.0, 0.0, float("-inf"), float("nan")]])
    m.top_k = lambda *a, **kw: (None, None, keys)
    m._top_k_check = lambda *a: (None, 1, 6, 1)
    assert m.target_ranks(None, None, None, [[0, 1, 2, 3, 4, 5]]).tolist() == [[0, 4, 1, 2, 3, 5]]


def test_metrics_from_ranks_are_the_list_metrics():
    rng = np.random.default_rng(3)
    U, I = 40, 60
    order = np.stack([rng.permutation(I) for _ in range(U)])              # user u's full ranking of the items
    positives = {u: set(rng.choice(I, int(rng.integers(0, 6)), replace=False).tolist()) for u in range(U)}
    positives[7] = {5, I + 3}                                             # a positive that is no candidate: never a hit
    top = {u: order[u].tolist() for u in range(U)}
    ranks = [[int(np.flatnonzero(order[u] == it)[0]) if it < I else -1 for it in sorted(positives[u])] for u in range(U)]
    n_pos = [len(positives[u]) for u in range(U)]
    got = ranking_metrics_from_ranks(ranks, n_pos, [1, 3, 10])
    for k in (1, 3, 10):
        want = recommend.ranking_metrics(top, positives, k)
        for key in ("hit_rate@%d" % k, "recall@%d" % k, "ndcg@%d" % k):
            assert abs(got[key] - want[key]) <= 1e-12, key
        assert got["users"] == want["users"]
    # by hand: user 0 ranks 2 and 9 of 3 positives (one without a rank), user 1 has no ranked positive, user 2 no positive
    m = ranking_metrics_from_ranks(np.asarray([[9, 2, -1], [-1, -1, -1], [-1, -1, -1]]), [3, 1, 0], [3])
    assert m["users"] == 2 and m["mrr"] == (1.0 / 3.0 + 0.0) / 2 and m["mean_rank"] == 5.5
    assert m["hit_rate@3"] == 0.5 and m["recall@3"] == (1.0 / 3.0) / 2
    assert abs(m["ndcg@3"] - (0.5 / (1.0 + 1.0 / np.log2(3) + 0.5)) / 2) <= 1e-15
    with pytest.raises(ValueError):
        ranking_metrics_from_ranks([[1, 2]], [1], [3])
    with pytest.raises(ValueError):
        ranking_metrics_from_ranks([[1]], [1], [0])


def test_sweep_rank_metrics_and_select(rank_kernels, tmp_path, capsys):
    from trainers import sweep
    job = tmp_path / "job"
    flags = ["--train-steps", "12", "--learning-rate", "0.001", "0.01", "--hidden-units", "64", "64"]   # (after the default 8 8)
    members = sweep.train_and_evaluate(_sweep_args(job, "--rank-metrics", "5", "10", "--select", "ndcg@10", *flags))
    out = capsys.readouterr().out
    assert len(members) == 4
    doc = json.load(open(job / "sweep.json"))
    rows = doc["members"]
    assert doc["select"] == "ndcg@10" and "best of 4 members by ndcg@10" in out
    keys = {"%s@%d" % (n, k) for n in ("hit_rate", "recall", "ndcg") for k in (5, 10)} | {"mrr", "mean_rank", "users"}
    assert all(set(r["ranking"]) == keys and r["ranking"]["users"] > 0 for r in rows)
    vals = [r["ranking"]["ndcg@10"] for r in rows]
    assert vals == sorted(vals, reverse=True)
    # ONE group call for the two members inside the scope; the [64, 64] members one by one, and a line says so
    calls = [m._engine().k.calls for m in members]
    assert sum(c.get("mi_pair_target_ranks", 0) for c in calls) == 1
    assert [c.get("mi_pair_topk", 0) for c in calls] == [0, 0, 1, 1]
    assert out.count("--rank-metrics: member") == 2 and "member 2: the model has a hidden layer of 64 units" in out
    # a member's ranking is what trainers.recommend --metrics-at reports for its directory
    by = {r["member"]: r for r in rows}
    m = recommend.main(["--model", "deep_fm", "--job-dir", str(job / "member_1"), "--synthetic", "300", "--device", "cpu",
                        "--metrics-at", "5", "10"] + by[1]["flags"])
    assert {key: m[key] for key in keys} == by[1]["ranking"]
    # mean_rank sorts ascending; without the flag sweep.json has no ranking
    sweep.train_and_evaluate(_sweep_args(job, "--rank-metrics", "5", "--select", "mean_rank", *flags))
    vals = [r["ranking"]["mean_rank"] for r in json.load(open(job / "sweep.json"))["members"]]
    assert vals == sorted(vals)
    sweep.train_and_evaluate(_sweep_args(job, *flags))
    doc = json.load(open(job / "sweep.json"))
    assert doc["select"] == "auc" and all("ranking" not in r for r in doc["members"])
    # --select: today's names, the ranking names with their cutoff among --rank-metrics, nothing else
    for bad in (["--select", "ndcg@10"], ["--select", "ndcg@10", "--rank-metrics", "5"], ["--select", "mrr"],
                ["--rank-metrics", "0"]):
        with pytest.raises(SystemExit):
            sweep.train_and_evaluate(_sweep_args(job, *bad))
    for bad in ("precision", "ndcg@", "ndcg@0", "hit_rate@x"):
        with pytest.raises(SystemExit):
            _sweep_args(job, "--select", bad)
    assert _sweep_args(job, "--select", "loss").select == "loss" and _sweep_args(job).rank_metrics is None


def test_recommend_metrics_at(rank_kernels, tmp_path):
    export = _train_deep_fm_export(str(tmp_path), "a", ["--embedding-size", "4", "--hidden-units", "8", "8"])
    job = os.path.dirname(os.path.dirname(export))
    base = ["--model", "deep_fm", "--job-dir", job, "--synthetic", "300", "--device", "cpu", "--top-k", "5", "--embedding-size", "4",
            "--hidden-units", "8", "8"]
    before = recommend.main(base)
    assert recommend.parse_args(base).metrics_at is None and set(before) == {"hit_rate@5", "recall@5", "ndcg@5", "users"}
    saved = json.load(open(os.path.join(job, "recommend", "top5_metrics.json")))
    got = recommend.main(base + ["--metrics-at", "5", "300"])
    assert set(got) == set(before) | {"hit_rate@300", "recall@300", "ndcg@300", "mrr", "mean_rank"}
    assert json.load(open(os.path.join(job, "recommend", "top5_metrics.json"))) == got
    assert all(got[key] == before[key] == saved[key] for key in before)
    # the exact ranks say what the list says at the list's own cutoff, and everything eligible is inside a long enough list
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:30:2")
    users, _, items, _ = recommend.tables(train, test)
    targets = recommend.positive_targets(users, items, test)
    assert got["users"] == sum(1 for t in targets if t) > 0 and 0 < got["mrr"] <= 1 and 0 <= got["mean_rank"] < len(items)
    assert got["hit_rate@300"] >= got["hit_rate@5"] and got["recall@300"] >= got["recall@5"]
    with pytest.raises(SystemExit, match="--metrics-at: not with --top 2"):
        recommend.main(base + ["--metrics-at", "5", "--top", "2"])
    with pytest.raises(SystemExit, match="--metrics-at 0"):
        recommend.main(base + ["--metrics-at", "0"])


def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    err = lambda: lib.mi_last_error().decode()
    keep = []

    def raw(hidden_after):
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
                setattr(m, name, 4096)                   # (pointers a host-side refusal never follows)
            m.layer_off, m.widths = layer_off.ctypes.data, widths.ctypes.data
            m.H1, m.E, m.n_layers, m.activation = 16, 4, len(w) - 1, 1
        return ms

    ok = raw([[16], [16]])
    U, I, Tq = 70, 333, 10
    size = lib.mi_pair_target_ranks_workspace_bytes
    need = size(ok, 2, U, I, Tq)
    assert need > size(ok, 1, U, I, Tq) > 0 and size(ok, 2, U, I, 64) > need
    assert size(ok, 0, U, I, Tq) == 0 and size(None, 2, U, I, Tq) == 0 and size(ok, 257, U, I, Tq) == 0
    assert size(ok, 2, U, I, 0) == 0 and size(ok, 2, U, I, 65) == 0
    call = lambda ms, M, tq=Tq, tg=8192, rk=8192, ws=8192, wsb=1 << 40, eo=None, ei=None: lib.mi_pair_target_ranks(
        ms, M, U, I, eo, ei, tg, tq, rk, None, ws, wsb, None)
    assert call(ok, 0) == -1 and "0 members (at least 1)" in err()
    assert call(ok, 257) == -2 and "257 members (at most 256" in err()
    assert call(raw([[16], [64]]), 2) == -2 and "member 1:" in err() and "hidden width of 64" in err() and "below 32" in err()
    assert call(raw([[16], [16, 16, 300]]), 2) == -1 and "member 1: pair_topk: hidden widths after layer 1" in err()
    for tq in (0, 65):
        assert call(ok, 2, tq=tq) == -1 and "Tq=%d targets per query (1 to 64" % tq in err()
    assert call(ok, 2, eo=8192) == -1 and "excl_off and excl_idx go together" in err()
    assert call(ok, 2, rk=None) == -1 and "targets / ranks" in err()
    assert call(ok, 2, tg=None) == -1 and "targets / ranks" in err()
    assert call(ok, 2, wsb=need - 1) == -1 and "workspace %d < %d bytes" % (need - 1, need) in err()
    assert call(ok, 2, ws=None) == -1 and "workspace" in err()
    assert call(None, 2) == -1 and "members" in err()


def test_header_binding_and_library_agree_on_the_new_entry(lib):
    decls = _header_decls()
    for name, nargs in (("mi_pair_target_ranks_workspace_bytes", 5), ("mi_pair_target_ranks", 13)):
        assert decls[name] == nargs == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_rec.h")).read()
    assert "#define MI_PAIR_RANKS_MAX_TARGETS %d" % _lib.PAIR_RANKS_MAX_TARGETS in src
    assert lib.mi_abi_version() == _lib.ABI_VERSION
