"""GPU: exact ranks of named targets under an ensemble's MEAN logit in one launch (mi_pair_target_ranks_mean,
engine.target_ranks_mean, EnsemblePredictor.rank_targets, python -m trainers.sweep --ensemble N --rank-metrics, python -m
trainers.recommend --top N --mean-metrics-at).

A rank is an integer function of the mean scores mi_pair_topk_group writes, which the rank-group tests already hold to
fp64, so everything here is exact: the ranks against the header's selection rule applied to top_k_group's own `scores`,
the targets' scores against that matrix bit for bit, the top-K list position by position, an analytic case over many
splits, nine members (two launches of the member table), NaN and infinities through the raw entry, the fallback outside
the kernel's scope, the refusals of the raw entry with guarded outputs, and the CLIs end to end."""
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from mi355x_rec.engine import DeepFM
from mi355x_rec.predictor import EnsemblePredictor
from tests.cases import VOCAB26
from tests.rank_kernels import oracle_ranks
from tests.util import (GUARD, dev, exact_workspace, guarded_nan, guards_intact, make_problem,
                        workspace_surroundings_intact)

pytestmark = pytest.mark.gpu

F32 = np.float32
Q5 = [0, 1, 2, 3, 4]
# (E, hidden, activation, (linear, mf, dnn)): the three kinds of member the kernel takes
MIXED = [(4, [16, 16], "relu", (True, True, True)), (8, [64, 16], "tanh", (False, True, True)), (4, [], "relu", (True, True, False))]


def _ids(rng, U, I):
    qid = np.stack([rng.integers(0, VOCAB26[f], U) for f in Q5], 1).astype(np.int32)
    cid = np.stack([rng.integers(0, VOCAB26[f], I) for f in range(5, 26)], 1).astype(np.int32)
    return qid, cid


def _engine(seed, E, hidden, act, flags):
    lin, mf, dnn = flags
    p, _, _, _ = make_problem(seed, VOCAB26, E, hidden, 4, use_dnn=dnn)
    m = DeepFM(VOCAB26, embedding_size=E, hidden_units=hidden, use_linear=lin, use_mf=mf, use_dnn=dnn, activation=act,
               device="cuda")
    m.load_oracle_params(p)
    return m


@pytest.fixture(scope="module")
def mixed():
    return [_engine(20 + i, *spec) for i, spec in enumerate(MIXED)]


def _group_scores(engines, qid, cid, fields=Q5):
    """the mean score matrix as mi_pair_topk_group writes it"""
    return engine.top_k_group(engines, dev(qid), dev(cid), fields, 1, return_scores=True)[2].cpu().numpy()


@pytest.fixture(scope="module")
def mixed_run(mixed):
    """M = 3 mixed members, U = 70 (three query blocks, the last partial), I = 333 (6 splits of 56, a tail round of one
    candidate), 0 / 1 / 7 / 64 targets per query: one call with the scores, and top_k_group's mean score matrix"""
    rng = np.random.default_rng(5)
    U, I = 70, 333
    qid, cid = _ids(rng, U, I)
    cid[I // 2] = cid[3]                                 # equal candidates: equal scores, decided by the index
    targets = [rng.choice(I, (0, 1, 7, 64)[u % 4], replace=False).tolist() for u in range(U)]
    targets[2] = [3, I // 2, 9, 3, 40, 41, 42]           # both equal candidates, one of them twice
    targets[6] = [7, I, 11, -1, 12, I + 70, 13]          # a target >= I, a -1 in the middle of the row
    excl = [sorted(set(rng.integers(0, I, int(rng.integers(0, I // 20 + 1))).tolist())) for _ in range(U)]
    excl[2] = sorted(set(excl[2]) - set(targets[2]))     # (the rows built by hand keep their targets eligible)
    excl[6] = sorted(set(excl[6]) - set(targets[6]))
    for u in (3, 10, 18):                                # exclusions that cover targets
        excl[u] = sorted(set(excl[u]) | {targets[u][0]})
    excl[5] = list(range(I))                             # every candidate of a query with one target excluded
    ranks, scores = engine.target_ranks_mean(mixed, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    return qid, cid, targets, excl, ranks.cpu().numpy(), scores.cpu().numpy(), _group_scores(mixed, qid, cid)


def test_ranks_equal_the_rule_on_the_groups_mean_scores(mixed, mixed_run):
    qid, cid, targets, excl, ranks, scores, z = mixed_run
    U, I = 70, 333
    assert ranks.shape == (U, 64) and ranks.dtype == np.int32 and scores.shape == (U, 64)
    real = sum(1 for t in targets for c in t if 0 <= c < I)
    assert np.array_equal(z[:, I // 2].view(np.uint32), z[:, 3].view(np.uint32))
    want = oracle_ranks(z, targets, excl)
    # (the test cannot pass on empty output: by construction at least 90 % of the real targets have a rank)
    assert (want >= 0).sum() >= 0.9 * real, ((want >= 0).sum(), real)
    assert np.array_equal(ranks, want), np.argwhere(ranks != want)[:8].tolist()
    assert want[2, 1] == want[2, 0] + 1 and want[2, 3] == want[2, 0]
    assert (want[6, [1, 3, 5]] == -1).all() and (want[6, [0, 2, 4, 6]] >= 0).all()
    assert want[3, 0] == want[10, 0] == want[18, 0] == -1 and (want[5] == -1).all()
    for u in range(U):
        t = np.asarray(targets[u] + [-1] * (64 - len(targets[u])))
        has = want[u] >= 0
        assert np.array_equal(scores[u, has].view(np.uint32), z[u, t[has]].view(np.uint32)), u
        assert np.isnan(scores[u, ~has]).all(), u
    # the mean's order is no member's own: the launch ranked by the mean
    own = engine.target_ranks_group(mixed, dev(qid), dev(cid), Q5, targets, exclude=excl).cpu().numpy()
    assert all(not np.array_equal(own[i], ranks) for i in range(3))


def test_a_second_call_and_a_group_of_one_give_the_same_integers(mixed, mixed_run):
    qid, cid, targets, excl, ranks, scores, _ = mixed_run
    again, s2 = engine.target_ranks_mean(mixed, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    assert np.array_equal(again.cpu().numpy(), ranks)
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), scores.view(np.uint32))
    # member 1 alone: z_0 / 1.0f is exact, so the mean's ranking is that member's own
    alone, sa = engine.target_ranks_mean([mixed[1]], dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    own, so = engine.target_ranks_group([mixed[1]], dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    assert torch.equal(alone, own[0]) and torch.equal(sa.view(torch.int32), so[0].view(torch.int32))
    assert not np.array_equal(alone.cpu().numpy(), ranks)


def test_the_member_order_is_part_of_the_definition(mixed, mixed_run):
    qid, cid, targets, excl, _, _, _ = mixed_run
    back = mixed[::-1]
    ranks, scores = engine.target_ranks_mean(back, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    z = _group_scores(back, qid, cid)
    want = oracle_ranks(z, targets, excl)
    assert np.array_equal(ranks.cpu().numpy(), want)
    t = np.asarray([row + [-1] * (64 - len(row)) for row in targets])
    has = want >= 0
    assert np.array_equal(scores.cpu().numpy()[has].view(np.uint32), np.take_along_axis(z, np.where(has, t, 0), 1)[has].view(np.uint32))


def test_a_rank_below_k_is_the_position_in_the_groups_top_k_list(mixed):
    """k = 256, I = 300, 70 targets per query (two passes of the entry): target t with rank r < 256 sits at top_idx[q, r]"""
    rng = np.random.default_rng(7)
    U, I, k = 37, 300, 256
    qid, cid = _ids(rng, U, I)
    cid[I // 2] = cid[3]
    excl = [sorted(set(rng.integers(0, I, 12).tolist())) for _ in range(U)]
    targets = [rng.choice(I, 70, replace=False).tolist() for _ in range(U)]
    ranks = engine.target_ranks_mean(mixed[:2], dev(qid), dev(cid), Q5, targets, exclude=excl).cpu().numpy()
    assert ranks.shape == (U, 70)
    top = engine.top_k_group(mixed[:2], dev(qid), dev(cid), Q5, k, exclude=excl)[1].cpu().numpy()
    inside = 0
    for u in range(U):
        for j, t in enumerate(targets[u]):
            r = ranks[u, j]
            assert (r == -1) == (t in excl[u]) and r < I - len(excl[u])
            if 0 <= r < k:
                assert top[u, r] == t, (u, j)
                inside += 1
            elif r >= k:
                assert t not in top[u]
    assert inside > U * 40


def _linear_members(rng, I, n=2):
    """n linear-only members over the columns [7, I]: member j's wide weight of candidate c is c * 1e-3 * (j + 1), so every
    member's score, and the mean, ascend with the candidate index"""
    engines = []
    for j in range(n):
        m = DeepFM([7, I], use_mf=False, use_dnn=False, device="cuda")
        lin = [rng.standard_normal(7).astype(F32) * F32(0.01), np.arange(I, dtype=F32) * F32(1e-3 * (j + 1))]
        m.lin_w.copy_(torch.from_numpy(np.concatenate(lin)).cuda())
        engines.append(m)
    return engines


def test_many_splits_with_an_analytic_answer():
    """M = 2 linear-only members with ascending wide weights, U = 40, I = 4096: 64 splits of 64 candidates; the rank of t is
    the number of non-excluded candidates above it"""
    U, I = 40, 4096
    rng = np.random.default_rng(3)
    engines = _linear_members(rng, I)
    qid = rng.integers(0, 7, (U, 1)).astype(np.int32)
    cid = np.arange(I, dtype=np.int32).reshape(I, 1)
    excl = [sorted(set(rng.integers(0, I, 300).tolist())) for _ in range(U)]
    targets = [rng.choice(I, 10, replace=False).tolist() + [0, I - 1] for _ in range(U)]
    ranks = engine.target_ranks_mean(engines, dev(qid), dev(cid), [0], targets, exclude=excl).cpu().numpy()
    want = np.zeros((U, 12), np.int32)
    for u in range(U):
        ok = np.ones(I, bool)
        ok[excl[u]] = False
        above = np.concatenate([np.cumsum(ok[::-1])[::-1][1:], [0]])        # eligible candidates with a larger index
        want[u] = [above[t] if ok[t] else -1 for t in targets[u]]
    assert (want >= 0).mean() > 0.85
    assert np.array_equal(ranks, want), np.argwhere(ranks != want)[:8].tolist()


def test_nine_members_cross_the_member_tables_chunk(mixed):
    """the member table reaches the workspace 8 members a launch: 9 members take two; U = 33 (a partial second block), I = 65"""
    engines = mixed + [_engine(40 + i, *MIXED[i % 3]) for i in range(6)]
    rng = np.random.default_rng(14)
    U, I = 33, 65
    qid, cid = _ids(rng, U, I)
    excl = [sorted(set(rng.integers(0, I, 4).tolist())) for _ in range(U)]
    targets = [rng.choice(I, 9, replace=False).tolist() for _ in range(U)]
    ranks, scores = engine.target_ranks_mean(engines, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    z = _group_scores(engines, qid, cid)
    want = oracle_ranks(z, targets, excl)
    assert (want >= 0).mean() > 0.85 and np.array_equal(ranks.cpu().numpy(), want)
    has = want >= 0
    assert np.array_equal(scores.cpu().numpy()[has].view(np.uint32), np.take_along_axis(z, np.asarray(targets), 1)[has].view(np.uint32))
    # and the last member counts: without it the integers differ
    assert not np.array_equal(engine.target_ranks_mean(engines[:8], dev(qid), dev(cid), Q5, targets, exclude=excl).cpu().numpy(), want)


def _raw_members(engines, qid, cid, fields=Q5):
    """the mi_rank_member_t array engine.target_ranks_mean would pass, and what keeps its tensors alive"""
    sides, U, I, _ = engines[0]._top_k_check(dev(qid), dev(cid), fields, 1, None, None)
    args = [e._top_k_sides(sides) for e in engines]
    return engine._rank_members(engines, args), args


def test_nan_and_infinite_means_rank_as_the_header_says():
    """two linear-only members, so the order is known by hand: the mean ascends with the index, but candidates 7 and 20 are NaN
    in member 0, candidate 50 is +inf in member 0 and -inf in member 1 (a NaN mean) and candidate 60 is +inf in member 0 alone"""
    lib = _lib.load()
    rng = np.random.default_rng(12)
    U, I, Tq = 33, 150, 7
    engines = _linear_members(rng, I)
    qid = rng.integers(0, 7, (U, 1)).astype(np.int32)
    cid = np.arange(I, dtype=np.int32).reshape(I, 1)
    ms, args = _raw_members(engines, qid, cid, [0])
    args[0]["w_c"][[7, 20]] = float("nan")               # (the side tensors are this call's own: the models are untouched)
    args[0]["w_c"][[50, 60]] = float("inf")
    args[1]["w_c"][50] = float("-inf")
    order = [60] + [c for c in range(I - 1, -1, -1) if c not in (7, 20, 50, 60)] + [7, 20, 50]   # best first; NaNs by index
    pos = {c: r for r, c in enumerate(order)}
    targets = [[7, 20, 50, 60, 3, 149, int(rng.integers(61, 149))] for _ in range(U)]
    tg = dev(np.asarray(targets, np.int32))
    ranks = torch.full((U, Tq), -9, dtype=torch.int32, device="cuda")
    scores = torch.zeros(U, Tq, device="cuda")
    ws = torch.empty(lib.mi_pair_target_ranks_mean_workspace_bytes(ms, 2, U, I, Tq), dtype=torch.uint8, device="cuda")
    rc = lib.mi_pair_target_ranks_mean(ms, 2, U, I, None, None, tg.data_ptr(), Tq, ranks.data_ptr(), scores.data_ptr(),
                                       ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mi_last_error().decode()
    got, s = ranks.cpu().numpy(), scores.cpu().numpy()
    assert np.array_equal(got, np.asarray([[pos[t] for t in row] for row in targets], np.int32)), got[:2].tolist()
    assert (got[:, :4] == [I - 3, I - 2, I - 1, 0]).all()
    assert np.isnan(s[:, :3]).all() and np.isposinf(s[:, 3]).all() and np.isfinite(s[:, 4:]).all()


def _exports(root, specs):
    """one small trained deep_fm export per (name, flags)"""
    from trainers import _cli, recommend
    trainer, opt = recommend.MODELS["deep_fm"]
    out = []
    for name, extra in specs:
        job = os.path.join(root, name)
        trainer.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(
            ["--synthetic", "300", "--job-dir", job, "--train-steps", "2", "--batch-size", "16"] + extra))
        out.append(os.path.join(job, "export", "exporter"))
    return out


def test_outside_the_scope_auto_is_layered_and_fused_names_the_member(tmp_path):
    from trainers import ml_100k, recommend
    ens = EnsemblePredictor.from_exports(_exports(str(tmp_path), [("a", ["--embedding-size", "4", "--hidden-units", "16", "16"]),
                                                                  ("b", ["--embedding-size", "4", "--hidden-units", "64", "64"])]))
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:30:2")
    users, qf, items, cf = recommend.tables(train, test)
    off, idx = recommend.exclusion_csr(users, items, train)
    excl = [idx[off[u]:off[u + 1]].tolist() for u in range(len(users))]
    rng = np.random.default_rng(13)
    I = len(items)
    targets = [rng.choice(I, 5, replace=False).tolist() + [I + 1] for _ in users]
    with pytest.raises(ValueError, match=r"mode='fused': member 1: the model has a hidden layer of 64 units after the first \(below 32\)"):
        ens.rank_targets(qf, cf, targets, mode="fused")
    ranks, scores = ens.rank_targets(qf, cf, targets, exclude=excl, return_scores=True)        # auto
    z = ens.recommend(qf, cf, 1, exclude=excl, mode="layered", return_scores=True)["scores"]
    want = oracle_ranks(z, targets, excl)
    assert ranks.dtype == np.int32 and (want >= 0).mean() > 0.6 and np.array_equal(ranks, want)
    has = want >= 0
    assert np.array_equal(scores[has].view(np.uint32), np.take_along_axis(z, np.where(has, np.asarray(targets), 0), 1)[has].view(np.uint32))
    assert np.isnan(scores[~has]).all()


def test_refusals_write_nothing(mixed):
    lib = _lib.load()
    err = lambda: lib.mi_last_error().decode()
    U, I, Tq = 33, 70, 5
    rng = np.random.default_rng(9)
    qid, cid = _ids(rng, U, I)
    out_of_scope = _engine(30, 4, [64, 64], "relu", (True, True, True))
    good, keep = _raw_members([mixed[0], mixed[1]], qid, cid)
    bad, keep2 = _raw_members([mixed[0], out_of_scope], qid, cid)
    need = lib.mi_pair_target_ranks_mean_workspace_bytes(good, 2, U, I, Tq)
    wbuf, ws = exact_workspace(need)
    bsc, scores = guarded_nan(U, Tq)
    rbuf = torch.full((U * Tq + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    ranks = rbuf[GUARD:GUARD + U * Tq]
    tg = dev(rng.integers(0, I, (U, Tq)).astype(np.int32))
    eo = torch.zeros(U + 1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(ms, M, tq=Tq, t=tg.data_ptr(), rk=ranks.data_ptr(), wsb=ws.numel(), off=None):
        return lib.mi_pair_target_ranks_mean(ms, M, U, I, off, None, t, tq, rk, scores.data_ptr(), ws.data_ptr(), wsb, st)

    assert call(good, 0) == -1 and "0 members" in err()
    assert call(good, 257) == -2 and "257 members (at most 256" in err()
    assert call(bad, 2) == -2 and "member 1:" in err() and "below 32" in err()
    for tq in (0, 65):
        assert call(good, 2, tq=tq) == -1 and "Tq=%d targets per query (1 to 64" % tq in err()
    assert call(good, 2, off=eo.data_ptr()) == -1 and "excl_off and excl_idx go together" in err()
    assert call(good, 2, rk=None) == -1 and "targets / ranks" in err()
    assert call(good, 2, t=None) == -1 and "targets / ranks" in err()
    assert call(good, 2, wsb=need - 1) == -1 and "workspace %d < %d bytes" % (need - 1, need) in err()
    torch.cuda.synchronize()
    assert bool(torch.isnan(bsc).all()) and bool((rbuf == -7).all()) and bool((wbuf == 0xA5).all())
    # and the same arguments, accepted: the outputs are written, the guards and the workspace's surroundings stay
    assert call(good, 2) == 0, err()
    torch.cuda.synchronize()
    assert guards_intact(bsc) and bool((rbuf[:GUARD] == -7).all()) and bool((rbuf[-GUARD:] == -7).all())
    assert workspace_surroundings_intact(wbuf, ws)
    assert not bool(torch.isnan(scores).any()) and bool((ranks >= 0).all()) and bool((ranks < I).all())
    assert keep and keep2


def test_sweep_ranks_its_ensemble_as_recommend_does_end_to_end(tmp_path, capsys):
    from trainers import recommend, sweep
    job = tmp_path / "job"
    sweep.train_and_evaluate(sweep.make_parser().parse_args(
        ["--synthetic", "300", "--job-dir", str(job), "--batch-size", "16", "--train-steps", "20", "--seeds", "3", "--ensemble", "2",
         "--rank-metrics", "10", "--select", "ndcg@10"]))
    out = capsys.readouterr().out
    doc = json.load(open(job / "sweep.json"))
    ens, rows = doc["ensemble"], doc["members"]
    assert len(rows) == 3 and ens["members"] == [r["member"] for r in rows[:2]]
    assert set(ens["ranking"]) == set(rows[0]["ranking"]) and ens["ranking"]["users"] == rows[0]["ranking"]["users"] > 0
    assert "ensemble of the 2 best members by its mean logit: ndcg@10 = %.6g" % ens["ranking"]["ndcg@10"] in out
    m = recommend.main(["--model", "deep_fm", "--job-dir", str(job), "--synthetic", "300", "--top", "2", "--mean-metrics-at", "10"])
    assert json.load(open(job / "recommend" / "top10_ensemble2_metrics.json")) == m
    # the exact ranks say what the ensemble's top-10 list says: hit_rate@10, recall@10 and ndcg@10 in m are the list's
    assert {key: m[key] for key in ens["ranking"]} == ens["ranking"]
    assert 0 < m["mrr"] <= 1 and 0 <= m["mean_rank"]
