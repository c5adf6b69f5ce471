"""CPU: the host side of ranking with an ensemble — engine.top_k_group, Predictor.recommend, EnsemblePredictor.recommend
(its three modes, its refusals, what it does once per call) and trainers.recommend --top.  mi_pair_topk_group is stood in
by a numpy restatement of its contract in include/mi355x_rec.h (tests.cpu_kernels.NumpyKernels: member m's score is the numpy
mi_pair_topk's, the mean is formed in fp32 in member order, the selection is the header's rule); the real kernel is tested
in test_hip_rank_group.py.  The binding and the library's host-side refusals are checked against the real library."""
import ctypes as C
import csv
import json
import os

import numpy as np
import pytest

from mi355x_rec import _lib, engine, predictor
from mi355x_rec.engine import DeepFM
from mi355x_rec.predictor import EnsemblePredictor, Predictor
from tests.cpu_kernels import NumpyKernels, cpu_kernels  # noqa: F401  (a fixture)
from tests.util import _fake_sweep, _header_decls, _train_deep_fm_export, max_err_scaled
from trainers import _cli, ml_100k, recommend
from trainers.conf_utils import get_run_config

@pytest.fixture(scope="module")
def exports(tmp_path_factory):
    """three small trained deep_fm exports: two inside the group kernel's scope, one ([64, 64]) outside it"""
    root = str(tmp_path_factory.mktemp("rankens"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine, "HipKernels", NumpyKernels)
        return [_train_deep_fm_export(root, "a", ["--embedding-size", "4", "--hidden-units", "8", "8"]),
                _train_deep_fm_export(root, "b", ["--embedding-size", "8", "--hidden-units", "8"]),
                _train_deep_fm_export(root, "c", ["--embedding-size", "4", "--hidden-units", "64", "64"])]


@pytest.fixture(scope="module")
def sides():
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:30:2")
    users, qf, items, cf = recommend.tables(train, test)
    return users, qf, items, cf, recommend.exclusion_csr(users, items, train)


def _members(exports, which=(0, 1)):
    return [Predictor.from_export(exports[i], device="cpu") for i in which]


def test_fused_and_layered_agree(cpu_kernels, exports, sides):
    users, qf, items, cf, excl = sides
    ens = EnsemblePredictor(_members(exports))
    out = {mode: ens.recommend(qf, cf, 7, exclude=excl, mode=mode, return_scores=True) for mode in ("fused", "layered", "auto")}
    U, I = len(users), len(items)
    for got in out.values():
        assert set(got) == {"logits", "probabilities", "indices", "scores"}
        assert got["logits"].shape == (U, 7) and got["indices"].dtype == np.int32 and got["scores"].shape == (U, I)
    assert np.array_equal(out["fused"]["indices"], out["layered"]["indices"])
    assert max_err_scaled(out["fused"]["logits"], out["layered"]["logits"]) < 1e-5
    assert np.array_equal(out["auto"]["indices"], out["fused"]["indices"])
    # the mean is the fp32 sum in member order over a division, and only eligible candidates come back
    solo = [p.engine for p in ens.members]
    assert "scores" not in ens.recommend(qf, cf, 7, exclude=excl)
    off, idx = excl
    for u in range(U):
        assert not set(out["fused"]["indices"][u].tolist()) & set(idx[off[u]:off[u + 1]].tolist())
    sel = np.take_along_axis(out["fused"]["scores"], out["fused"]["indices"].astype(np.int64), 1)
    assert np.array_equal(sel, out["fused"]["logits"])
    # one member: that member's own recommendation
    one = EnsemblePredictor(_members(exports, (0,))).recommend(qf, cf, 7, exclude=excl, mode="fused")
    own = Predictor.from_export(exports[0], device="cpu").recommend(qf, cf, 7, exclude=excl)
    assert np.array_equal(one["indices"], own["indices"]) and np.array_equal(one["logits"], own["logits"])
    assert len(solo) == 2


def test_auto_follows_the_members_scope_and_fused_names_the_member(cpu_kernels, exports, sides):
    users, qf, items, cf, excl = sides
    inside, mixed = EnsemblePredictor(_members(exports)), EnsemblePredictor(_members(exports, (0, 2)))
    assert inside.rank_fused_limit() is None and mixed.rank_fused_limit()[0] == 1
    k = inside.k
    k.calls.clear()
    inside.recommend(qf, cf, 3)
    assert k.calls.get("mi_pair_topk_group", 0) == 1 and "mi_pair_topk" not in k.calls
    for e in (p.engine.k for p in mixed.members):
        e.calls.clear()
    got = mixed.recommend(qf, cf, 3, exclude=excl)                       # auto: every member by its own top_k
    assert all("mi_pair_topk_group" not in p.engine.k.calls and p.engine.k.calls.get("mi_pair_topk", 0) == 1 for p in mixed.members)
    want = mixed.recommend(qf, cf, 3, exclude=excl, mode="layered")
    assert np.array_equal(got["indices"], want["indices"]) and np.array_equal(got["logits"], want["logits"])
    with pytest.raises(ValueError, match=r"mode='fused': member 1: the model has a hidden layer of 64 units after the first \(below 32\)"):
        mixed.recommend(qf, cf, 3, mode="fused")
    with pytest.raises(ValueError, match="member 1: the model has a hidden layer of 64 units"):
        engine.top_k_group([p.engine for p in mixed.members], None, None, [0], 3)
    with pytest.raises(ValueError, match="mode"):
        inside.recommend(qf, cf, 3, mode="eager")
    # the scope is the pair kernel's VALU path
    lim = lambda hidden: DeepFM([5, 6], hidden_units=hidden, device="cpu")._top_k_group_limit()
    assert all(lim(h) is None for h in ([16, 16], [64, 16], [64], [], [4096, 31]))
    assert all(lim(h) is not None for h in ([64, 64], [16, 32], [16, 8, 40]))


@pytest.mark.parametrize("mode", ["fused", "layered"])
def test_ids_are_transformed_once_and_exclusions_built_once(cpu_kernels, exports, sides, monkeypatch, mode):
    users, qf, items, cf, excl = sides
    ens = EnsemblePredictor(_members(exports))
    count = {"side_inputs": 0, "exclusions": 0, "sides": 0}
    real_inputs, real_excl, real_sides = predictor.side_inputs, DeepFM._top_k_exclusions, DeepFM._top_k_sides
    monkeypatch.setattr(predictor, "side_inputs", lambda *a: count.__setitem__("side_inputs", count["side_inputs"] + 1) or real_inputs(*a))
    monkeypatch.setattr(DeepFM, "_top_k_exclusions",
                        lambda self, *a: count.__setitem__("exclusions", count["exclusions"] + 1) or real_excl(self, *a))
    monkeypatch.setattr(DeepFM, "_top_k_sides", lambda self, *a: count.__setitem__("sides", count["sides"] + 1) or real_sides(self, *a))
    ens.recommend(qf, cf, 4, exclude=excl, mode=mode)
    assert count == {"side_inputs": 2, "exclusions": 1, "sides": 2}    # one per side; once; one per member


def test_predictor_recommend_is_estimator_recommend(cpu_kernels, exports, sides):
    users, qf, items, cf, excl = sides
    trainer, opt = recommend.MODELS["deep_fm"]
    job = os.path.dirname(os.path.dirname(exports[0]))
    args = _cli.make_parser("deep_fm", opt).parse_args(["--job-dir", job, "--device", "cpu", "--embedding-size", "4",
                                                        "--hidden-units", "8", "8"])
    config = get_run_config()
    config.device = "cpu"
    est = trainer.make_estimator(args, ml_100k.get_feature_columns(embedding_size=4), config)
    want = est.recommend(qf, cf, 6, exclude=excl)
    got = Predictor.from_export(exports[0], device="cpu").recommend(dict(qf, unread=[0] * len(users)), cf, 6, exclude=excl)
    for key in ("logits", "probabilities", "indices"):
        assert np.array_equal(got[key], want[key]), key


def test_cli_top(cpu_kernels, exports, sides, tmp_path):
    job = _fake_sweep(str(tmp_path), exports[:2])
    base = ["--model", "deep_fm", "--job-dir", job, "--synthetic", "300", "--device", "cpu", "--top-k", "5"]
    assert recommend.parse_args(base).top is None
    metrics = recommend.main(base + ["--top", "2"])
    assert {"hit_rate@5", "recall@5", "ndcg@5", "users"} <= set(metrics)
    out = os.path.join(job, "recommend", "top5_ensemble2.csv")
    assert set(json.load(open(os.path.join(job, "recommend", "top5_ensemble2_metrics.json")))) == set(metrics)
    rows = list(csv.DictReader(open(out)))
    assert list(rows[0]) == ["user_id", "rank", "item_id", "logit", "probability"]
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:30:2")
    users, qf, items, cf = recommend.tables(train, test)
    want = EnsemblePredictor.from_sweep(job, top=2, device="cpu").recommend(
        qf, cf, 5, exclude=recommend.exclusion_csr(users, items, train), mode="layered")
    flat = [(int(users[u]), int(items[i]), want["logits"][u, r]) for u in range(len(users)) for r, i in enumerate(want["indices"][u])
            if i >= 0]
    assert [(int(r["user_id"]), int(r["item_id"])) for r in rows] == [(u, i) for u, i, _ in flat]
    assert max_err_scaled(np.asarray([float(r["logit"]) for r in rows]), np.asarray([z for _, _, z in flat], np.float64)) < 1e-5
    # the three errors
    single = os.path.dirname(os.path.dirname(exports[0]))
    with pytest.raises(SystemExit, match="--top 1: .* has no sweep.json"):
        recommend.main(["--model", "deep_fm", "--job-dir", single, "--synthetic", "300", "--device", "cpu", "--top", "1"])
    with pytest.raises(SystemExit, match=r"--top 2: an ensemble is made of .* deep_fm models \(--model linear\)"):
        recommend.main(["--model", "linear", "--job-dir", job, "--synthetic", "300", "--device", "cpu", "--top", "2"])
    for top in (0, 3):
        with pytest.raises(SystemExit, match="--top %d out of range: .* has 2 members" % top):
            recommend.main(base + ["--top", str(top)])
    # without --top nothing changes: the job directory's checkpoint, <job-dir>/recommend/top<K>.csv
    recommend.main(["--model", "deep_fm", "--job-dir", single, "--synthetic", "300", "--device", "cpu", "--top-k", "4",
                    "--embedding-size", "4", "--hidden-units", "8", "8"])
    assert os.path.exists(os.path.join(single, "recommend", "top4.csv"))
    assert os.path.exists(os.path.join(single, "recommend", "top4_metrics.json"))


def _raw_members(hidden_after, n=1):
    """n mi_rank_member_t with layers H1 -> hidden_after -> 1, pointers that a host-side refusal never follows"""
    keep = []
    ms = (_lib.RankMember * n)()
    for i, after in enumerate(hidden_after):
        w = [16] + list(after) + [1]
        widths = np.asarray(w, np.int32)
        off, o = [], 0
        for a, b in zip(w[:-1], w[1:]):
            off += [o, o + a * b]
            o += a * b + b
        layer_off = np.asarray(off, np.int64)
        keep += [widths, layer_off]
        m = ms[i]
        for name in ("a_q", "s_q", "w_q", "a_c", "s_c", "w_c", "dense"):
            setattr(m, name, 4096)
        m.layer_off, m.widths = layer_off.ctypes.data, widths.ctypes.data
        m.H1, m.E, m.n_layers, m.activation = 16, 4, len(w) - 1, 1
    return ms, keep


def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    err = lambda: lib.mi_last_error().decode()
    ok, keep = _raw_members([[16], [16]], 2)
    U, I, k = 70, 333, 10
    need = lib.mi_pair_topk_group_workspace_bytes(ok, 2, U, I, k)
    assert need > lib.mi_pair_topk_group_workspace_bytes(ok, 1, U, I, k) > 0
    assert lib.mi_pair_topk_group_workspace_bytes(ok, 0, U, I, k) == 0 and lib.mi_pair_topk_group_workspace_bytes(None, 2, U, I, k) == 0
    assert lib.mi_pair_topk_group_workspace_bytes(ok, 257, U, I, k) == 0 and lib.mi_pair_topk_group_workspace_bytes(ok, 2, U, I, 257) == 0
    call = lambda ms, M, ts=8192, ti=8192, ws=8192, wsb=1 << 40, eo=None, ei=None: lib.mi_pair_topk_group(
        ms, M, U, I, eo, ei, k, ts, ti, None, None, ws, wsb, None)
    assert call(ok, 0) == -1 and "0 members (at least 1)" in err()
    assert call(ok, 257) == -2 and "257 members (at most 256" in err()
    bad, keep2 = _raw_members([[16], [64]], 2)
    assert call(bad, 2) == -2
    assert "member 1:" in err() and "hidden width of 64" in err() and "below 32" in err()
    wide, keep3 = _raw_members([[16], [16, 16, 300]], 2)                 # mi_pair_topk's own check, prefixed
    assert call(wide, 2) == -1 and "member 1: pair_topk: hidden widths after layer 1" in err()
    assert call(ok, 2, wsb=need - 1) == -1 and "workspace %d < %d bytes" % (need - 1, need) in err()
    assert call(ok, 2, ws=None) == -1 and "workspace" in err()
    assert call(ok, 2, ts=None) == -1 and "top_score / top_idx" in err()
    assert call(ok, 2, ti=None) == -1 and "top_score / top_idx" in err()
    assert call(ok, 2, eo=8192) == -1 and "excl_off and excl_idx go together" in err()
    assert call(None, 2) == -1 and "members" in err()
    # the single-model entry keeps its checks and messages
    assert lib.mi_pair_topk(None, None, None, 4, None, None, None, 4, 0, 0, None, None, None, 0, 9, None, None, 2, 8192, 8192,
                            None, None, 0, None) == -1 and "pair_topk: activation 9" in err()
    assert keep and keep2 and keep3


def test_header_binding_and_library_agree_on_the_new_entries(lib):
    decls = _header_decls()
    for name, nargs in (("mi_pair_topk_group_workspace_bytes", 5), ("mi_pair_topk_group", 14)):
        assert decls[name] == nargs == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    assert lib.mi_abi_version() == 21 == _lib.ABI_VERSION
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_rec.h")).read()
    assert "#define MI_PAIR_TOPK_GROUP_MAX_MEMBERS %d" % _lib.PAIR_TOPK_GROUP_MAX_MEMBERS in src
    assert _lib.PAIR_TOPK_GROUP_MAX_MEMBERS == _lib.PREDICT_GROUP_MAX_MEMBERS
    # mi_rank_member_t: 9 pointers and 4 ints, as the header lays them out
    assert C.sizeof(_lib.RankMember) == 9 * 8 + 4 * 4
    fields = [f for f, _ in _lib.RankMember._fields_]
    struct = src[src.index("typedef struct mi_rank_member {"):src.index("} mi_rank_member_t;")]
    assert [f for f in fields if f in struct] == fields and all(struct.index(a) < struct.index(b) for a, b in zip(fields, fields[1:]))
