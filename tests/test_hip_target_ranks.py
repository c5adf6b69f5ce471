"""GPU: exact ranks of named targets for every member in one launch (mi_pair_target_ranks, engine.target_ranks_group,
DeepFM.target_ranks, python -m trainers.sweep --rank-metrics, python -m trainers.recommend --metrics-at).

A rank is an integer function of scores the rank tests already hold to fp64, so everything here is exact: the ranks against
the header's selection rule applied to each member's OWN mi_pair_topk score matrix, the targets' scores against that
matrix bit for bit, the top-K list position by position, an analytic case over many splits, NaN through the raw entry, the
fallback outside the kernel's scope, the refusals of the raw entry with guarded outputs, and the CLIs end to end."""
import json

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from mi355x_rec.engine import DeepFM
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


def _own_scores(m, qid, cid):
    return m.top_k(dev(qid), dev(cid), Q5, 1, return_scores=True)[2].cpu().numpy()


@pytest.fixture(scope="module")
def mixed_run(mixed):
    """M = 3 mixed members, U = 70 (three query blocks, the last partial), I = 333 (6 splits of 56, a tail round of one
    candidate), 0 / 1 / 7 / 64 targets per query: one group call with the scores, and every member's own score matrix"""
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
    ranks, scores = engine.target_ranks_group(mixed, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    own = [_own_scores(m, qid, cid) for m in mixed]
    return qid, cid, targets, excl, ranks.cpu().numpy(), scores.cpu().numpy(), own


def test_ranks_equal_the_rule_on_each_members_own_scores(mixed, mixed_run):
    qid, cid, targets, excl, ranks, scores, own = mixed_run
    U, I = 70, 333
    assert ranks.shape == (3, U, 64) and ranks.dtype == np.int32 and scores.shape == (3, U, 64)
    real = sum(1 for t in targets for c in t if 0 <= c < I)
    for i in range(3):
        z = own[i]
        assert np.array_equal(z[:, I // 2].view(np.uint32), z[:, 3].view(np.uint32))
        want = oracle_ranks(z, targets, excl)
        # (the test cannot pass on empty output: by construction at least 90 % of the real targets have a rank)
        assert (want >= 0).sum() >= 0.9 * real, ((want >= 0).sum(), real)
        assert np.array_equal(ranks[i], want), (i, np.argwhere(ranks[i] != want)[:8].tolist())
        assert want[2, 1] == want[2, 0] + 1 and want[2, 3] == want[2, 0]
        assert (want[6, [1, 3, 5]] == -1).all() and (want[6, [0, 2, 4, 6]] >= 0).all()
        assert want[3, 0] == want[10, 0] == want[18, 0] == -1 and (want[5] == -1).all()
        for u in range(U):
            t = np.asarray(targets[u] + [-1] * (64 - len(targets[u])))
            has = want[u] >= 0
            assert np.array_equal(scores[i, u, has].view(np.uint32), z[u, t[has]].view(np.uint32)), (i, u)
            assert np.isnan(scores[i, u, ~has]).all(), (i, u)
    # the members rank differently: the launch took each member's own logit
    assert not np.array_equal(ranks[0], ranks[1]) and not np.array_equal(ranks[0], ranks[2])


def test_a_second_call_and_a_group_of_one_give_the_same_integers(mixed, mixed_run):
    qid, cid, targets, excl, ranks, scores, _ = mixed_run
    again, s2 = engine.target_ranks_group(mixed, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    assert np.array_equal(again.cpu().numpy(), ranks)
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), scores.view(np.uint32))
    # member 1 alone (a group of one): the same integers
    alone = mixed[1].target_ranks(dev(qid), dev(cid), Q5, targets, exclude=excl, mode="fused")
    assert np.array_equal(alone.cpu().numpy(), ranks[1])


def test_a_rank_below_k_is_the_position_in_the_top_k_list(mixed):
    """k = 256, I = 300, 70 targets per query (two passes of the entry): target t with rank r < 256 sits at top_idx[q, r]"""
    rng = np.random.default_rng(7)
    U, I, k = 37, 300, 256
    qid, cid = _ids(rng, U, I)
    cid[I // 2] = cid[3]
    excl = [sorted(set(rng.integers(0, I, 12).tolist())) for _ in range(U)]
    targets = [rng.choice(I, 70, replace=False).tolist() for _ in range(U)]
    ranks = engine.target_ranks_group(mixed[:2], dev(qid), dev(cid), Q5, targets, exclude=excl).cpu().numpy()
    assert ranks.shape == (2, U, 70)
    for i, m in enumerate(mixed[:2]):
        top = m.top_k(dev(qid), dev(cid), Q5, k, exclude=excl)[1].cpu().numpy()
        inside = 0
        for u in range(U):
            for j, t in enumerate(targets[u]):
                r = ranks[i, u, j]
                assert (r == -1) == (t in excl[u]) and r < I - len(excl[u])
                if 0 <= r < k:
                    assert top[u, r] == t, (i, u, j)
                    inside += 1
                elif r >= k:
                    assert t not in top[u]
        assert inside > U * 40


def test_many_splits_with_an_analytic_answer():
    """M = 2 linear-only members with ascending wide weights, U = 40, I = 4096: 64 splits of 64 candidates; the rank of t is
    the number of non-excluded candidates above it"""
    U, I = 40, 4096
    rng = np.random.default_rng(3)
    engines = []
    for j in range(2):
        m = DeepFM([7, I], use_mf=False, use_dnn=False, device="cuda")
        lin = [rng.standard_normal(7).astype(F32) * F32(0.01), np.arange(I, dtype=F32) * F32(1e-3 * (j + 1))]
        m.lin_w.copy_(torch.from_numpy(np.concatenate(lin)).cuda())
        engines.append(m)
    qid = rng.integers(0, 7, (U, 1)).astype(np.int32)
    cid = np.arange(I, dtype=np.int32).reshape(I, 1)
    excl = [sorted(set(rng.integers(0, I, 300).tolist())) for _ in range(U)]
    targets = [rng.choice(I, 10, replace=False).tolist() + [0, I - 1] for _ in range(U)]
    ranks = engine.target_ranks_group(engines, dev(qid), dev(cid), [0], targets, exclude=excl).cpu().numpy()
    want = np.zeros((U, 12), np.int32)
    for u in range(U):
        ok = np.ones(I, bool)
        ok[excl[u]] = False
        above = np.concatenate([np.cumsum(ok[::-1])[::-1][1:], [0]])        # eligible candidates with a larger index
        want[u] = [above[t] if ok[t] else -1 for t in targets[u]]
    assert (want >= 0).mean() > 0.85
    assert np.array_equal(ranks[0], want) and np.array_equal(ranks[1], want)


def test_nine_members_cross_the_member_tables_chunk(mixed):
    """the member table reaches the workspace 8 members a launch: 9 members take two; U = 37 (a partial second block),
    I = 131 (a ragged last split), 3 targets per query, one of them -1 and one excluded"""
    engines = mixed + [_engine(40 + i, *MIXED[i % 3]) for i in range(6)]
    rng = np.random.default_rng(14)
    U, I = 37, 131
    qid, cid = _ids(rng, U, I)
    targets = [[int(t[0]), -1, int(t[1])] for t in (rng.choice(I, 2, replace=False) for _ in range(U))]
    excl = [sorted(set(rng.integers(0, I, 4).tolist()) - {targets[u][0]} | {targets[u][2]}) for u in range(U)]
    ranks, scores = engine.target_ranks_group(engines, dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True)
    ranks, scores = ranks.cpu().numpy(), scores.cpu().numpy()
    assert ranks.shape == (9, U, 3) and (ranks[:, :, 0] >= 0).all() and (ranks[:, :, 1:] == -1).all()
    # the last member, from the table's second launch, ranks as it does alone and as the rule says on its own scores
    alone, s1 = engines[8].target_ranks(dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True, mode="fused")
    assert np.array_equal(ranks[8], alone.cpu().numpy())
    assert np.array_equal(scores[8, :, 0].view(np.uint32), s1.cpu().numpy()[:, 0].view(np.uint32))
    z = _own_scores(engines[8], qid, cid)
    assert np.array_equal(ranks[8], oracle_ranks(z, targets, excl))
    assert np.array_equal(scores[8, :, 0].view(np.uint32), z[np.arange(U), [t[0] for t in targets]].view(np.uint32))
    assert np.isnan(scores[8, :, 1:]).all()


def _raw_members(engines, qid, cid):
    """the mi_rank_member_t array engine.target_ranks_group would pass, and what keeps its tensors alive"""
    sides, U, I, _ = engines[0]._top_k_check(dev(qid), dev(cid), Q5, 1, None, None)
    args = [e._top_k_sides(sides) for e in engines]
    return engine._rank_members(engines, args), args


def test_nan_ranks_below_every_number_and_among_nans_by_index(mixed):
    lib = _lib.load()
    rng = np.random.default_rng(12)
    U, I, Tq = 33, 150, 6
    qid, cid = _ids(rng, U, I)
    m = mixed[0]
    z = _own_scores(m, qid, cid)
    ms, args = _raw_members([m], qid, cid)
    args[0]["w_c"][[20, 7]] = float("nan")               # (the side tensors are this call's own: the model is untouched)
    z[:, [20, 7]] = np.nan
    targets = [[7, 20, 3, int(rng.integers(21, 149)), 149, 0] for _ in range(U)]
    tg = dev(np.asarray(targets, np.int32))
    ranks = torch.full((1, U, Tq), -9, dtype=torch.int32, device="cuda")
    scores = torch.zeros(1, U, Tq, device="cuda")
    ws = torch.empty(lib.mi_pair_target_ranks_workspace_bytes(ms, 1, U, I, Tq), dtype=torch.uint8, device="cuda")
    rc = lib.mi_pair_target_ranks(ms, 1, U, I, None, None, tg.data_ptr(), Tq, ranks.data_ptr(), scores.data_ptr(), ws.data_ptr(),
                                  ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mi_last_error().decode()
    got = ranks.cpu().numpy()[0]
    assert (got[:, 0] == I - 2).all() and (got[:, 1] == I - 1).all()          # the two NaNs last, the lower index first
    assert np.array_equal(got, oracle_ranks(z, targets, [[] for _ in range(U)]))
    assert np.isnan(scores.cpu().numpy()[0, :, :2]).all() and not np.isnan(scores.cpu().numpy()[0, :, 2:]).any()


def test_outside_the_scope_auto_falls_back_and_fused_raises():
    m = _engine(30, 4, [64, 64], "relu", (True, True, True))
    rng = np.random.default_rng(13)
    U, I = 45, 200
    qid, cid = _ids(rng, U, I)
    cid[I // 2] = cid[3]
    excl = [sorted(set(rng.integers(0, I, 20).tolist())) for _ in range(U)]
    targets = [[3, I // 2] + rng.choice(I, 5, replace=False).tolist() + [I + 1] for _ in range(U)]
    with pytest.raises(ValueError, match=r"mode='fused': the model has a hidden layer of 64 units after the first \(below 32\)"):
        m.target_ranks(dev(qid), dev(cid), Q5, targets, mode="fused")
    ranks, scores = m.target_ranks(dev(qid), dev(cid), Q5, targets, exclude=excl, return_scores=True, mode="auto")
    z = _own_scores(m, qid, cid)
    want = oracle_ranks(z, targets, excl)
    assert (want >= 0).mean() > 0.6 and np.array_equal(ranks.cpu().numpy(), want)
    got_s = scores.cpu().numpy()
    t = np.asarray(targets)
    has = want >= 0
    assert np.array_equal(got_s[has].view(np.uint32), np.take_along_axis(z, np.where(has, t, 0), 1)[has].view(np.uint32))
    assert np.isnan(got_s[~has]).all()


def test_refusals_write_nothing(mixed):
    lib = _lib.load()
    err = lambda: lib.mi_last_error().decode()
    U, I, Tq = 33, 70, 5
    rng = np.random.default_rng(9)
    qid, cid = _ids(rng, U, I)
    out_of_scope = _engine(30, 4, [64, 64], "relu", (True, True, True))
    good, keep = _raw_members([mixed[0], mixed[1]], qid, cid)
    bad, keep2 = _raw_members([mixed[0], out_of_scope], qid, cid)
    need = lib.mi_pair_target_ranks_workspace_bytes(good, 2, U, I, Tq)
    wbuf, ws = exact_workspace(need)
    bsc, scores = guarded_nan(2, U, Tq)
    rbuf = torch.full((2 * U * Tq + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    ranks = rbuf[GUARD:GUARD + 2 * U * Tq]
    tg = dev(rng.integers(0, I, (U, Tq)).astype(np.int32))
    eo = torch.zeros(U + 1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(ms, M, tq=Tq, rk=ranks.data_ptr(), wsb=ws.numel(), off=None):
        return lib.mi_pair_target_ranks(ms, M, U, I, off, None, tg.data_ptr(), tq, rk, scores.data_ptr(), ws.data_ptr(), wsb, st)

    assert call(good, 0) == -1 and "0 members" in err()
    assert call(good, 257) == -2 and "257 members (at most 256" in err()
    assert call(bad, 2) == -2 and "member 1:" in err() and "below 32" in err()
    for tq in (0, 65):
        assert call(good, 2, tq=tq) == -1 and "Tq=%d targets per query (1 to 64" % tq in err()
    assert call(good, 2, off=eo.data_ptr()) == -1 and "excl_off and excl_idx go together" in err()
    assert call(good, 2, rk=None) == -1 and "targets / ranks" in err()
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


def test_sweep_rank_metrics_are_recommends_metrics_at_end_to_end(tmp_path, capsys):
    from trainers import recommend, sweep
    job = tmp_path / "job"
    sweep.train_and_evaluate(sweep.make_parser().parse_args(
        ["--synthetic", "300", "--job-dir", str(job), "--batch-size", "16", "--train-steps", "20", "--learning-rate", "0.001",
         "0.01", "--rank-metrics", "10", "--select", "ndcg@10"]))
    assert "--rank-metrics: member" not in capsys.readouterr().out           # (both members took the one launch)
    doc = json.load(open(job / "sweep.json"))
    rows = doc["members"]
    assert doc["select"] == "ndcg@10" and sorted(r["member"] for r in rows) == [0, 1]
    vals = [r["ranking"]["ndcg@10"] for r in rows]
    assert vals == sorted(vals, reverse=True)
    for r in rows:
        m = recommend.main(["--model", "deep_fm", "--job-dir", r["dir"], "--synthetic", "300", "--metrics-at", "10"] + r["flags"])
        assert r["ranking"]["users"] > 0 and {key: m[key] for key in r["ranking"]} == r["ranking"], r["member"]
