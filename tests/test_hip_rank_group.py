"""GPU: top-K recommendation with an ensemble (mi_pair_topk_group, engine.top_k_group, EnsemblePredictor.recommend,
python -m trainers.recommend --top).

Every member's score bit for bit against its own mi_pair_topk, the mean bit for bit against the fp32 sum in member order
over a division and within 1e-5 of the fp64 oracle, the selection bit for bit against the header's rule applied to the
kernel's own mean scores, the refusals of the raw entry with guarded outputs, and the CLI end to end."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from mi355x_rec.engine import DeepFM
from mi355x_rec.predictor import EnsemblePredictor, Predictor
from oracle import deepfm as O
from tests.cases import VOCAB26
from tests.util import _fake_sweep, dev, guarded_nan, guards_intact, host_topk, make_problem, max_err_scaled

pytestmark = pytest.mark.gpu

F32 = np.float32
Q5 = [0, 1, 2, 3, 4]
# (E, hidden, activation, (linear, mf, dnn)): the three kinds of member the group kernel takes
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
    return m, p


@pytest.fixture(scope="module")
def mixed():
    return [_engine(20 + i, *spec) for i, spec in enumerate(MIXED)]


@pytest.fixture(scope="module")
def mixed_run(mixed):
    """M = 3 mixed members, U = 70 (three query blocks, the last partial), I = 333 (6 splits of 56, a tail round of one
    candidate), k = 10: the group call with both optional outputs, once for the tests that read it"""
    rng = np.random.default_rng(5)
    qid, cid = _ids(rng, 70, 333)
    engines = [m for m, _ in mixed]
    top_s, top_i, scores, member_scores = engine.top_k_group(engines, dev(qid), dev(cid), Q5, 10, return_scores=True,
                                                             return_member_scores=True)
    return qid, cid, top_s.cpu(), top_i.cpu(), scores.cpu(), member_scores.cpu()


def test_member_scores_are_the_members_own_bits_and_the_mean_is_fp32_in_member_order(mixed, mixed_run):
    qid, cid, top_s, top_i, scores, member_scores = mixed_run
    assert tuple(member_scores.shape) == (3, 70, 333) and tuple(scores.shape) == (70, 333)
    for i, (m, _) in enumerate(mixed):
        own = m.top_k(dev(qid), dev(cid), Q5, 10, return_scores=True)[2].cpu()
        assert torch.equal(member_scores[i].view(torch.int32), own.view(torch.int32)), i
    z = member_scores
    want = ((z[0] + z[1]) + z[2]) / torch.full_like(z[0], 3.0)
    assert torch.equal(scores.view(torch.int32), want.view(torch.int32))
    # the selection saw the mean: the best candidate of every query carries its mean score
    best = torch.gather(scores, 1, top_i[:, :1].long())
    assert torch.equal(best.view(torch.int32), top_s[:, :1].view(torch.int32))


def test_mean_scores_match_the_fp64_oracle(mixed, mixed_run):
    qid, cid, _, _, scores, _ = mixed_run
    U, I = 70, 333
    ids = np.zeros((U * I, 26), np.int32)
    ids[:, Q5] = np.repeat(qid, I, 0)
    ids[:, list(range(5, 26))] = np.tile(cid, (U, 1))
    ref = np.zeros((U, I))
    for (m, p), (E, hidden, act, (lin, mf, dnn)) in zip(mixed, MIXED):
        ref += O.forward(p.astype(np.float64), ids, use_linear=lin, use_mf=mf, use_dnn=dnn, activation=act)["logits"].reshape(U, I)
    err = max_err_scaled(scores.numpy(), ref / 3.0)
    print("group mean vs fp64 oracle: max_err_scaled = %.3g" % err)
    assert err < 1e-5, err


@pytest.mark.parametrize("k,I", [(1, 300), (10, 300), (256, 300), (1, 131), (10, 131), (256, 131)])
def test_selection_bit_for_bit(mixed, k, I):
    engines = [m for m, _ in mixed[:2]]
    rng = np.random.default_rng(k + I)
    U = 37
    qid, cid = _ids(rng, U, I)
    cid[I // 2] = cid[3]                        # equal candidates: equal means, decided by the index
    cid[I - 1] = cid[3]
    excl = [sorted(set(rng.integers(0, I, rng.integers(0, I // 3 + 1)).tolist())) for _ in range(U)]
    excl[5] = list(range(I))                    # every candidate excluded
    excl[6] = []
    score, idx, scores = engine.top_k_group(engines, dev(qid), dev(cid), Q5, k, exclude=excl, return_scores=True)
    sc = scores.cpu().numpy()
    assert np.array_equal(sc[:, I // 2].view(np.uint32), sc[:, 3].view(np.uint32))
    s_ref, i_ref = host_topk(sc, k, excl)
    got_s, got_i = score.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(got_i, i_ref)
    assert np.array_equal(got_s.view(np.uint32), s_ref.view(np.uint32))
    assert (got_i[5] == -1).all() and np.isneginf(got_s[5]).all()
    # the same selection through the CSR form of the exclusions, without the optional outputs
    off = np.concatenate([[0], np.cumsum([len(r) for r in excl])]).astype(np.int64)
    ix = np.asarray([c for r in excl for c in r], np.int32)
    s2, i2 = engine.top_k_group(engines, dev(qid), dev(cid), Q5, k, exclude=(off, ix))
    assert np.array_equal(i2.cpu().numpy(), got_i) and np.array_equal(s2.cpu().numpy().view(np.uint32), got_s.view(np.uint32))


def test_selection_with_merges_inside_the_candidate_loop():
    """M = 2 linear-only members with ascending wide weights, U = 40, I = 4096, k = 256: 32 splits of 128 candidates, every
    candidate beats the K-th of its query, so every one is appended and the 64 survivor slots fill twice per split"""
    U, I, k = 40, 4096, 256
    rng = np.random.default_rng(3)
    engines = []
    for j in range(2):
        m = DeepFM([7, I], use_mf=False, use_dnn=False, device="cuda")
        lin = [rng.standard_normal(7).astype(F32) * F32(0.01), np.arange(I, dtype=F32) * F32(1e-3 * (j + 1))]
        lin[1][I // 3:I // 3 + 50] = lin[1][I // 3]                  # ties inside the stream
        m.lin_w.copy_(torch.from_numpy(np.concatenate(lin)).cuda())
        engines.append(m)
    qid = rng.integers(0, 7, (U, 1)).astype(np.int32)
    cid = np.arange(I, dtype=np.int32).reshape(I, 1)
    excl = [sorted(set(rng.integers(I - 3 * k, I, k // 2).tolist())) for _ in range(U)]
    s1, i1, scores = engine.top_k_group(engines, dev(qid), dev(cid), [0], k, exclude=excl, return_scores=True)
    s_ref, i_ref = host_topk(scores.cpu().numpy(), k, excl)
    assert np.array_equal(i1.cpu().numpy(), i_ref)
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    for _ in range(2):
        s2, i2 = engine.top_k_group(engines, dev(qid), dev(cid), [0], k, exclude=excl)
        assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))


def test_one_member_is_that_members_top_k(mixed):
    m = mixed[0][0]
    rng = np.random.default_rng(8)
    qid, cid = _ids(rng, 45, 200)
    excl = [sorted(set(rng.integers(0, 200, 20).tolist())) for _ in range(45)]
    s1, i1, sc1 = m.top_k(dev(qid), dev(cid), Q5, 10, exclude=excl, return_scores=True)
    s2, i2, sc2, ms = engine.top_k_group([m], dev(qid), dev(cid), Q5, 10, exclude=excl, return_scores=True, return_member_scores=True)
    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert torch.equal(sc1.view(torch.int32), sc2.view(torch.int32)) and torch.equal(sc1.view(torch.int32), ms[0].view(torch.int32))


def test_nine_members_cross_the_member_tables_chunk(mixed):
    """the member table reaches the workspace 8 members a launch: 9 members take two; U = 37 (a partial second block),
    I = 131 (a ragged last split), k = 10"""
    engines = [m for m, _ in mixed] + [_engine(40 + i, *MIXED[i % 3])[0] for i in range(6)]
    rng = np.random.default_rng(14)
    U, I, k = 37, 131, 10
    qid, cid = _ids(rng, U, I)
    excl = [sorted(set(rng.integers(0, I, 4).tolist())) for _ in range(U)]
    top_s, top_i, scores, member_scores = engine.top_k_group(engines, dev(qid), dev(cid), Q5, k, exclude=excl, return_scores=True,
                                                             return_member_scores=True)
    # the last member, from the table's second launch, scores as it does alone
    own = engines[8].top_k(dev(qid), dev(cid), Q5, k, return_scores=True)[2]
    assert torch.equal(member_scores[8].view(torch.int32), own.view(torch.int32))
    z = member_scores.cpu()
    acc = z[0]
    for i in range(1, 9):
        acc = acc + z[i]
    mean = (acc / torch.full_like(acc, 9.0)).numpy()
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), mean.view(np.uint32))
    s_ref, i_ref = host_topk(mean, k, excl)
    assert np.array_equal(top_i.cpu().numpy(), i_ref)
    assert np.array_equal(top_s.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))


def _raw_members(engines, qid, cid):
    """the mi_rank_member_t array engine.top_k_group would pass, and what keeps its tensors alive"""
    sides, U, I, _ = engines[0]._top_k_check(dev(qid), dev(cid), Q5, 10, None, None)
    args = [e._top_k_sides(sides) for e in engines]
    ms = (_lib.RankMember * len(engines))()
    for m, e, a in zip(ms, engines, args):
        for name in ("a_q", "s_q", "w_q", "a_c", "s_c", "w_c", "layer_off", "widths"):
            setattr(m, name, _lib.ptr(a[name]))
        m.dense = _lib.ptr(e.dense)
        m.H1, m.E, m.n_layers, m.activation = a["H1"], a["E"], a["n_layers"], e.act
    return ms, args


def test_refusals_write_nothing(mixed):
    lib = _lib.load()
    err = lambda: lib.mi_last_error().decode()
    U, I, k = 33, 70, 10
    rng = np.random.default_rng(9)
    qid, cid = _ids(rng, U, I)
    out_of_scope, _ = _engine(30, 4, [64, 64], "relu", (True, True, True))
    good, keep = _raw_members([mixed[0][0], mixed[1][0]], qid, cid)
    bad, keep2 = _raw_members([mixed[0][0], out_of_scope], qid, cid)
    need = lib.mi_pair_topk_group_workspace_bytes(good, 2, U, I, k)
    ws = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    bs, top_s = guarded_nan(U, k)
    bsc, scores = guarded_nan(U, I)
    bms, member_scores = guarded_nan(2, U, I)
    top_i = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(ms, M, ts=top_s.data_ptr(), ti=top_i.data_ptr(), wsb=ws.numel()):
        return lib.mi_pair_topk_group(ms, M, U, I, None, None, k, ts, ti, scores.data_ptr(), member_scores.data_ptr(),
                                      ws.data_ptr(), wsb, st)

    assert call(good, 0) == -1 and "0 members" in err()
    assert call(good, 257) == -2 and "257 members (at most 256" in err()
    assert call(bad, 2) == -2 and "member 1:" in err() and "below 32" in err()
    assert call(good, 2, wsb=need - 1) == -1 and "workspace" in err()
    assert call(good, 2, ts=None) == -1 and call(good, 2, ti=None) == -1 and "top_score / top_idx" in err()
    torch.cuda.synchronize()
    for buf in (bs, bsc, bms):
        assert bool(torch.isnan(buf).all())
    assert bool((top_i == -7).all()) and bool((ws == 0xA5).all())
    # and the same arguments, accepted: the outputs are written, the guards stay
    assert call(good, 2) == 0, err()
    torch.cuda.synchronize()
    assert guards_intact(bs) and guards_intact(bsc) and guards_intact(bms)
    assert not bool(torch.isnan(top_s).any()) and not bool(torch.isnan(member_scores).any()) and bool((top_i >= 0).all())
    assert bool((ws[need:] == 0xA5).all())
    assert keep and keep2


def test_cli_top_and_predictor_recommend_end_to_end(tmp_path):
    from trainers import _cli, ml_100k, recommend
    from trainers.conf_utils import get_run_config
    trainer, opt = recommend.MODELS["deep_fm"]
    exports, flags = [], (["--embedding-size", "4", "--hidden-units", "16", "16"], ["--embedding-size", "8", "--hidden-units", "16"])
    for name, extra in zip("ab", flags):
        job = str(tmp_path / name)
        trainer.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(
            ["--synthetic", "300", "--job-dir", job, "--train-steps", "10", "--batch-size", "16"] + extra))
        exports.append(os.path.join(job, "export", "exporter"))
    sweep = _fake_sweep(str(tmp_path), exports)
    metrics = recommend.main(["--model", "deep_fm", "--job-dir", sweep, "--synthetic", "300", "--top", "2", "--top-k", "6"])
    assert set(json.load(open(os.path.join(sweep, "recommend", "top6_ensemble2_metrics.json")))) == set(metrics)
    rows = list(csv.DictReader(open(os.path.join(sweep, "recommend", "top6_ensemble2.csv"))))
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:30:2")
    users, qf, items, cf = recommend.tables(train, test)
    excl = recommend.exclusion_csr(users, items, train)
    ens = EnsemblePredictor.from_sweep(sweep, top=2)
    assert ens.rank_fused_limit() is None                                # (the CLI took the group launch)
    want = ens.recommend(qf, cf, 6, exclude=excl, mode="layered")
    flat = [(int(users[u]), int(items[i]), want["logits"][u, r]) for u in range(len(users)) for r, i in enumerate(want["indices"][u])
            if i >= 0]
    assert [(int(r["user_id"]), int(r["item_id"])) for r in rows] == [(u, i) for u, i, _ in flat]
    assert max_err_scaled(np.asarray([float(r["logit"]) for r in rows]), np.asarray([z for _, _, z in flat], np.float64)) < 1e-5
    # one export recommends what the checkpoint it was written from recommends
    job = os.path.dirname(os.path.dirname(exports[0]))
    est = trainer.make_estimator(_cli.make_parser("deep_fm", opt).parse_args(["--job-dir", job] + flags[0]),
                                 ml_100k.get_feature_columns(embedding_size=4), get_run_config())
    a = est.recommend(qf, cf, 6, exclude=excl)
    b = Predictor.from_export(exports[0]).recommend(qf, cf, 6, exclude=excl)
    for key in ("logits", "probabilities", "indices"):
        assert np.array_equal(a[key].view(np.uint32) if a[key].dtype == np.float32 else a[key],
                              b[key].view(np.uint32) if b[key].dtype == np.float32 else b[key]), key
