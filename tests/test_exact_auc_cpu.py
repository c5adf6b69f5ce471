"""CPU: the exact AUC / GAUC of mi355x_rec.exact_auc — the host side (layouts, metrics, FusedPopulation.evaluate(exact=...),
trainers.sweep's --exact-auc / --gauc-by) over the numpy stand-ins of tests.auc_kernels, and what the real library decides
on the host.  The real kernel is tested in test_hip_exact_auc.py.

The reference everywhere is the brute force on the header's key, a few lines of numpy below; it is cross-checked once
against the midrank Mann-Whitney statistic."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.exact_auc import ExactAuc
from mi355x_rec.metrics import auc_from_pair_counts, exact_auc_from_counts, gauc_from_counts, metrics_from_counters
from mi355x_rec.population import FusedPopulation
from mi355x_rec.predictor import EnsemblePredictor
from tests.auc_kernels import AucKernels, auc_kernels  # noqa: F401  (a fixture)
from tests.cases import _numpy_engine
from tests.cpu_kernels import NumpyKernels, counters
from tests.util import _fresh_ids, _header_decls, _t

F32 = np.float32
NEW_KEYS = {"auc_exact", "auc_exact_pairs"}
GAUC_KEYS = {"gauc", "gauc_groups"}


# ---- the reference ------------------------------------------------------------------------------------------------------
def key(z):
    """the header's key of fp32 logits: monotone bits, NaN -> 0, -0 as +0"""
    z = np.asarray(z, F32)
    u = z.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[z == 0] = 0x80000000
    k[np.isnan(z)] = 0
    return k


def brute(z, y):
    p, n = key(z[y == 1])[:, None], key(z[y == 0])[None, :]
    return int((p > n).sum()), int((p == n).sum())


def brute_groups(z, y, g):
    """per group in ascending order of its value: (gt, eq, positives, negatives)"""
    return [brute(z[g == v], y[g == v]) + (int(y[g == v].sum()), int((1 - y[g == v]).sum())) for v in np.unique(g)]


def gauc_reference(rows):
    num = den = 0.0
    n = 0
    for gt, eq, p, q in rows:
        if p and q:
            num += (p + q) * ((2 * gt + eq) / (2 * p * q))
            den += p + q
            n += 1
    return (num / den if n else 0.0), n


def problem(N=4096, seed=7, scale=1.0):
    """the issue's set: labels rng.random(N) < 0.55, logits normal(0, 1) + label as fp32"""
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.55).astype(np.uint8)
    z = (rng.normal(0, 1, N) + y).astype(F32)
    return (F32(scale) * z).astype(F32), y


def exact(y, groups=None):
    return ExactAuc(y, groups, device="cpu", kernels=AucKernels())


# ---- layout and stand-in against the brute force ------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(11)
    N = 700
    y = (rng.random(N) < 0.4).astype(np.uint8)
    z = rng.normal(0, 2, N).astype(F32)
    sizes = np.array([1, 2, 300, 1, 2, 5, 389])
    g = np.repeat(np.arange(len(sizes)), sizes)[rng.permutation(N)]
    one = y.copy()
    one[g == 5] = 1                                                       # a group of five positives
    one[g == 4] = 0                                                       # a group of two negatives
    pm0 = np.where(rng.random(N) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    nan = z.copy()
    nan[rng.random(N) < 0.2] = np.nan
    nan[3] = -np.inf
    nan[4] = np.inf
    return {
        "N=1": (np.array([0.3], F32), np.array([1], np.uint8), None),
        "one class": (z, np.ones(N, np.uint8), None),
        "every logit equal": (np.full(N, 1.25, F32), y, None),
        "3 values": (rng.choice(np.array([-1.5, 0.0, 2.0], F32), N), y, g),
        "+0 against -0": (pm0, y, g),
        "NaN": (nan, y, g),
        "groups of 1, 2 and 300": (z, y, g),
        "groups with one class": (z, one, g),
        "groups given as strings": (z, y, np.array(["user-%d" % (7 * v % 11) for v in g], dtype=object)),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_counts_equal_the_brute_force(name):
    z, y, g = CASES[name]
    ex = exact(y, g)
    zt = _t(z)
    gt, eq = brute(z, y)
    whole = ex.counts(zt)
    assert whole.dtype == torch.int64 and tuple(whole.shape) == (1, 1, 2) and whole[0, 0].tolist() == [gt, eq]
    m = ex.metrics(zt)[0]
    P, Q = int(y.sum()), int((1 - y).sum())
    assert m["auc_exact_pairs"] == P * Q
    assert m["auc_exact"] == ((2 * gt + eq) / (2 * P * Q) if P * Q else 0.0)
    if name == "every logit equal":
        assert m["auc_exact"] == 0.5
    if name == "one class":
        h, c, s = counters(z, y)
        assert m["auc_exact"] == 0.0 == metrics_from_counters(h, c, s)["auc"]
    if name == "+0 against -0":
        assert (gt, eq) == (0, P * Q)
    if name == "NaN":
        assert eq >= int((np.isnan(z) & (y == 1)).sum()) * int((np.isnan(z) & (y == 0)).sum()) > 0
    if g is None:
        assert set(m) == NEW_KEYS
        with pytest.raises(ValueError, match="without groups"):
            ex.counts(zt, grouped=True)
        return
    rows = brute_groups(z, y, g)
    by = ex.counts(zt, grouped=True)
    assert tuple(by.shape) == (1, len(rows), 2) and by[0].tolist() == [[r[0], r[1]] for r in rows]
    assert ex.grouped.n_pos.tolist() == [r[2] for r in rows] and ex.grouped.n_neg.tolist() == [r[3] for r in rows]
    assert list(ex.group_values) == list(np.unique(g))                   # ascending order of the groups' values
    want, n = gauc_reference(rows)
    assert set(m) == NEW_KEYS | GAUC_KEYS and m["gauc_groups"] == n and m["gauc"] == pytest.approx(want, rel=1e-14, abs=0)
    if name == "groups with one class":
        assert n == sum(1 for r in rows if r[2] and r[3]) < len(rows)


def test_the_layout_is_segment_major_with_negatives_first():
    z, y, g = CASES["groups of 1, 2 and 300"]
    ex = exact(y, g)
    for lay, seg in ((ex.whole, np.zeros(len(y), np.int64)), (ex.grouped, g)):
        o, off, neg = lay.order.numpy(), lay.seg_off.numpy(), lay.seg_neg.numpy()
        assert o.dtype == np.int32 and sorted(o.tolist()) == list(range(len(y))) and off[0] == 0 and off[-1] == len(y)
        assert not np.array_equal(o, np.arange(len(y)))
        for s in range(lay.S):
            assert (seg[o[off[s]:off[s + 1]]] == s).all()
            assert (y[o[off[s]:off[s] + neg[s]]] == 0).all() and (y[o[off[s] + neg[s]:off[s + 1]]] == 1).all()


def test_the_reference_is_the_midrank_mann_whitney_statistic():
    rng = np.random.default_rng(3)
    y = (rng.random(500) < 0.5).astype(np.uint8)
    z = rng.choice(np.linspace(-2, 2, 37).astype(F32), 500)              # heavy ties, no NaN
    vals, inv, cnt = np.unique(z, return_inverse=True, return_counts=True)
    mid = (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv.reshape(-1)]             # 1-based midranks
    P = int(y.sum())
    u2 = 2 * mid[y == 1].sum() - P * (P + 1)                             # 2 U = 2 gt + eq
    gt, eq = brute(z, y)
    assert u2 == 2 * gt + eq and eq > 0


def test_many_members_strided_rows_and_argument_checks():
    z, y = problem(300)
    rng = np.random.default_rng(5)
    wide = torch.from_numpy(rng.normal(0, 1, (3, 305)).astype(F32))
    wide[0, :300] = _t(z)
    rows = wide[:, :300]                                                  # row stride 305
    ex = exact(y)
    got = ex.counts(rows)
    assert tuple(got.shape) == (3, 1, 2)
    for m in range(3):
        assert got[m, 0].tolist() == list(brute(rows[m].numpy(), y))
    assert [d["auc_exact"] for d in ex.metrics(rows)] == [auc_from_pair_counts(*got[m, 0].tolist(), int(y.sum()), int((1 - y).sum()))
                                                          for m in range(3)]
    for bad in (rows.double(), rows[:, :299], rows.numpy(), wide[:, :600:2], rows.reshape(3, 3, 100)):
        with pytest.raises(ValueError, match="ExactAuc: logits must be a float32"):
            ex.counts(bad)
    with pytest.raises(ValueError, match="uint8"):
        ExactAuc(y.astype(np.int64), device="cpu", kernels=AucKernels())
    with pytest.raises(ValueError, match="labels are 0 or 1"):
        ExactAuc(np.array([0, 2], np.uint8), device="cpu", kernels=AucKernels())
    with pytest.raises(ValueError, match="groups must be"):
        ExactAuc(y, np.zeros(len(y)), device="cpu", kernels=AucKernels())


# ---- the reason for the feature -----------------------------------------------------------------------------------------
def test_the_exact_auc_ignores_the_logit_scale_and_the_bucketed_one_does_not():
    z, y = problem()
    z8, _ = problem(scale=8.0)
    assert np.array_equal(z8, F32(8) * z)
    ex = exact(y)
    a, a8 = ex.metrics(_t(z))[0]["auc_exact"], ex.metrics(_t(z8))[0]["auc_exact"]
    assert a == a8 == 0.7698614222686063                                  # (a power of two keeps every order and every tie)
    bucketed = [metrics_from_counters(*counters(v, y))["auc"] for v in (z, z8)]
    print("bucketed auc %.6f (z), %.6f (8 z); exact %.16f" % (bucketed[0], bucketed[1], a))
    assert abs(bucketed[0] - bucketed[1]) > 1e-2
    assert abs(bucketed[0] - a) < 1e-3 < abs(bucketed[1] - a)


# ---- the pure-host half -------------------------------------------------------------------------------------------------
def test_counts_to_metrics_on_the_host():
    assert auc_from_pair_counts(3, 2, 2, 4) == 0.5 and auc_from_pair_counts(0, 0, 0, 9) == 0.0
    assert auc_from_pair_counts(2 ** 61, 0, 2 ** 31, 2 ** 31) == 0.5     # (integers, not fp64 products)
    assert exact_auc_from_counts(np.array([[6, 0]]), 2, 3) == {"auc_exact": 1.0, "auc_exact_pairs": 6}
    # three groups: AUC 1.0 with 5 examples, one class (skipped), AUC 0.25 with 4
    got = gauc_from_counts([[6, 0], [0, 0], [0, 2]], [2, 3, 2], [3, 0, 2])
    assert got == {"gauc": (5 * 1.0 + 4 * 0.25) / 9, "gauc_groups": 2}
    assert gauc_from_counts([[0, 0]], [4], [0]) == {"gauc": 0.0, "gauc_groups": 0}
    with pytest.raises(ValueError, match="gauc_from_counts"):
        gauc_from_counts([[1, 0]], [1, 1], [1])


# ---- FusedPopulation.evaluate(exact=...) --------------------------------------------------------------------------------
def test_evaluate_with_exact_adds_the_new_keys_and_keeps_the_old_values():
    vocab, N, B = [9, 13, 5, 6], 83, 16
    k = AucKernels()
    members = []
    for j, (E, hidden) in enumerate(((8, [16, 8]), (4, [8]), (4, []))):
        m = _numpy_engine(vocab, E, hidden, k)
        g = torch.Generator()
        g.manual_seed(j)
        m.init_variables(g, lin_scale=0.3)
        members.append(m)
    pop = FusedPopulation(members)
    rng = np.random.default_rng(1)
    ids, y = _t(_fresh_ids(rng, vocab, N)), _t((rng.random(N) < 0.4).astype(np.uint8))
    groups = rng.integers(0, 7, N)
    plain, logits = pop.evaluate(ids, y, batch_size=B, return_logits=True)
    logits = logits.clone()
    k.calls.clear()
    ex = ExactAuc(y, groups, device="cpu", kernels=k)
    both = pop.evaluate(ids, y, batch_size=B, exact=ex)
    assert k.calls == {"mi_auc_plan": 2, "mi_eval_group": 1, "mi_auc_pair_counts": 2}
    for i in range(3):
        assert set(both[i]) == set(plain[i]) | NEW_KEYS | GAUC_KEYS
        assert {key_: both[i][key_] for key_ in plain[i]} == plain[i]
        z = logits[i].numpy()
        gt, eq = brute(z, y.numpy())
        assert both[i]["auc_exact"] == (2 * gt + eq) / (2 * int(y.sum()) * int((1 - y).sum()))
        want, n = gauc_reference(brute_groups(z, y.numpy(), groups))
        assert both[i]["gauc"] == pytest.approx(want, rel=1e-14, abs=0) and both[i]["gauc_groups"] == n
    again = pop.evaluate(ids, y, batch_size=B)                            # exact=None: today's keys and values
    assert again == plain
    with pytest.raises(ValueError, match="exact was built for 83 examples"):
        pop.evaluate(ids[:80].contiguous(), y[:80].contiguous(), batch_size=B, exact=ex)


# ---- trainers.sweep -----------------------------------------------------------------------------------------------------
OLD_KEYS = {"accuracy", "accuracy_baseline", "auc", "auc_precision_recall", "average_loss", "label/mean", "prediction/mean",
            "precision", "recall", "loss"}


def _args(job, *extra):
    from trainers import sweep
    return sweep.make_parser().parse_args(["--synthetic", "400", "--train-steps", "20", "--job-dir", str(job), "--batch-size", "16",
                                           "--device", "cpu", "--hidden-units", "8", "8", "--learning-rate", "0.001", "0.01",
                                           "--seeds", "2"] + list(extra))


@pytest.fixture
def registered(monkeypatch):
    """the ensemble's members are found by the stand-in of mi_predict_group through NumpyKernels.register"""
    real = EnsemblePredictor.from_sweep.__func__

    def from_sweep(cls, *a, **kw):
        ens = real(cls, *a, **kw)
        NumpyKernels.register([p.engine for p in ens.members])
        return ens
    monkeypatch.setattr(EnsemblePredictor, "from_sweep", classmethod(from_sweep))


def test_sweep_with_exact_auc_and_gauc_end_to_end(auc_kernels, registered, tmp_path, capsys):  # noqa: F811
    from trainers import sweep
    job = tmp_path / "job"
    sweep.train_and_evaluate(_args(job, "--eval-every", "10", "--exact-auc", "--gauc-by", "user_id", "--select", "gauc",
                                   "--ensemble", "2"))
    doc = json.load(open(job / "sweep.json"))
    rows = doc["members"]
    assert doc["select"] == "gauc" and len(rows) == 4
    lines = [json.loads(line) for line in open(job / "sweep_eval.jsonl")]
    assert [rec["global_step"] for rec in lines] == [10, 20]
    for rec in lines:
        assert all(set(m) == OLD_KEYS | NEW_KEYS | GAUC_KEYS for m in rec["members"])
    for r in rows:
        assert set(r["metrics"]) == OLD_KEYS | NEW_KEYS | GAUC_KEYS | {"global_step"}
        last = lines[-1]["members"][r["member"]]
        assert all(r["metrics"][k_] == last[k_] for k_ in NEW_KEYS | GAUC_KEYS)      # (the population evaluation's, --final-eval layered)
        assert 0.0 <= r["metrics"]["auc_exact"] <= 1.0 and r["metrics"]["auc_exact_pairs"] > 0
        curve = [(-rec["members"][r["member"]]["gauc"], rec["global_step"]) for rec in lines]
        assert (-r["best_value"], r["best_step"]) == min(curve)
    gaucs = [r["metrics"]["gauc"] for r in rows]
    assert gaucs == sorted(gaucs, reverse=True)
    assert set(doc["ensemble"]["metrics"]) == OLD_KEYS | NEW_KEYS | GAUC_KEYS
    assert doc["ensemble"]["metrics"]["auc_exact_pairs"] == rows[0]["metrics"]["auc_exact_pairs"]
    out = capsys.readouterr().out
    assert "--exact-auc: the largest |auc - auc_exact| over the 4 members is" in out and "the order of the members by auc" in out
    # groups that have both classes: gender has two values
    job2 = tmp_path / "job2"
    sweep.train_and_evaluate(_args(job2, "--gauc-by", "gender", "--select", "auc_exact"))
    rows = json.load(open(job2 / "sweep.json"))["members"]
    assert all(r["metrics"]["gauc_groups"] == 2 and 0.0 < r["metrics"]["gauc"] < 1.0 for r in rows)
    exacts = [r["metrics"]["auc_exact"] for r in rows]
    assert exacts == sorted(exacts, reverse=True) and all("best_step" not in r for r in rows)


def test_sweep_select_needs_its_flag_and_the_default_run_writes_what_it_wrote(auc_kernels, tmp_path):  # noqa: F811
    from trainers import sweep
    with pytest.raises(SystemExit, match="--select gauc needs --gauc-by"):
        sweep.train_and_evaluate(_args(tmp_path / "a", "--select", "gauc"))
    with pytest.raises(SystemExit, match="--select gauc needs --gauc-by"):
        sweep.train_and_evaluate(_args(tmp_path / "a", "--select", "gauc", "--exact-auc"))
    with pytest.raises(SystemExit, match="--select auc_exact needs --exact-auc"):
        sweep.train_and_evaluate(_args(tmp_path / "a", "--select", "auc_exact"))
    with pytest.raises(SystemExit, match="--gauc-by nobody: the test file has no such column"):
        sweep.train_and_evaluate(_args(tmp_path / "a", "--gauc-by", "nobody"))
    a = sweep.make_parser().parse_args([])
    assert a.exact_auc is False and a.gauc_by is None
    job = tmp_path / "job"
    members = sweep.train_and_evaluate(_args(job, "--eval-every", "10"))
    for rec in map(json.loads, open(job / "sweep_eval.jsonl")):
        assert all(set(m) == OLD_KEYS for m in rec["members"])
    for r in json.load(open(job / "sweep.json"))["members"]:
        assert set(r["metrics"]) == OLD_KEYS | {"global_step"}
    assert all("mi_auc_pair_counts" not in m._engine().k.calls for m in members)


def test_sweep_restored_with_the_new_flags_measures_the_last_step_again(auc_kernels, registered, tmp_path):  # noqa: F811
    """--restore of a finished sweep that had no exact keys: the last step is evaluated again for them, best_* come from the
    lines that have the selected metric, and the ensemble is counted although no training step is left"""
    from trainers import sweep
    job = tmp_path / "job"
    sweep.train_and_evaluate(_args(job, "--eval-every", "10"))
    sweep.train_and_evaluate(_args(job, "--restore", "--eval-every", "10", "--gauc-by", "gender", "--select", "gauc", "--ensemble", "2"))
    lines = [json.loads(line) for line in open(job / "sweep_eval.jsonl")]
    assert [rec["global_step"] for rec in lines] == [10, 20, 20]
    assert ["gauc" in rec["members"][0] for rec in lines] == [False, False, True]
    doc = json.load(open(job / "sweep.json"))
    for r in doc["members"]:
        assert r["best_step"] == 20 and r["best_value"] == r["metrics"]["gauc"] == lines[-1]["members"][r["member"]]["gauc"]
    assert doc["ensemble"]["metrics"]["gauc_groups"] == 2 and 0.0 < doc["ensemble"]["metrics"]["auc_exact"] < 1.0


# ---- the real library, without a device ---------------------------------------------------------------------------------
def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    table = torch.zeros(4096, dtype=torch.uint8)
    err = lambda: lib.mi_last_error().decode()

    def plan_refused(status, match, off, neg, S, run=0, tab=table, nbytes=4096, with_plan=True):
        p = _lib.AucPlan()
        rc = lib.mi_auc_plan(_lib.ptr(off), _lib.ptr(neg), S, run, _lib.ptr(tab), nbytes, C.byref(p) if with_plan else None, None)
        assert rc == status and match in err(), (rc, err())
        assert p.magic == 0 and p.device_table is None and not bool(table.any())
        if off is not None and neg is not None and status != -4 and with_plan and tab is not None:
            assert lib.mi_auc_plan_bytes(_lib.ptr(off), _lib.ptr(neg), S, run) == 0
    ok_off, ok_neg = i64(0, 10), i64(4)
    plan_refused(-1, "auc_plan: seg_off / seg_neg", None, ok_neg, 1)
    plan_refused(-1, "auc_plan: seg_off / seg_neg", ok_off, None, 1)
    plan_refused(-1, "auc_plan: device_table", ok_off, ok_neg, 1, tab=None)
    plan_refused(-1, "auc_plan: plan", ok_off, ok_neg, 1, with_plan=False)
    plan_refused(-1, "auc_plan: 0 segments (at least 1)", ok_off, ok_neg, 0)
    plan_refused(-1, "auc_plan: seg_off[0]=1", i64(1, 10), ok_neg, 1)
    plan_refused(-1, "auc_plan: seg_off[2]=5 after seg_off[1]=6", i64(0, 6, 5), i64(1, 0), 2)
    plan_refused(-1, "auc_plan: seg_neg[0]=11 negatives in a segment of 10 examples", ok_off, i64(11), 1)
    plan_refused(-1, "auc_plan: seg_neg[1]=-1 negatives", i64(0, 6, 9), i64(1, -1), 2)
    plan_refused(-1, "auc_plan: N=0 examples", i64(0, 0), i64(0), 1)
    plan_refused(-1, "auc_plan: N=2147483648 examples", i64(0, 2 ** 31), i64(5), 1)
    plan_refused(-1, "auc_plan: neg_run=-1", ok_off, ok_neg, 1, run=-1)
    plan_refused(-1, "auc_plan: neg_run=16777217", ok_off, ok_neg, 1, run=2 ** 24 + 1)
    plan_refused(-4, "auc_plan: device table of 16 bytes, 32 needed", ok_off, ok_neg, 1, nbytes=16)
    # the table's size: 32 bytes an item, tiles of 64 positives x runs of C negatives, never 0 for an accepted layout
    size = lambda off, neg, run=0: lib.mi_auc_plan_bytes(_lib.ptr(off), _lib.ptr(neg), len(neg), run)
    assert size(ok_off, ok_neg) == 32 and size(i64(0, 10), i64(10)) == 32 and size(i64(0, 10), i64(0)) == 32
    assert size(i64(0, 400), i64(200), 64) == 32 * 4 * 4 and size(i64(0, 400), i64(200)) == 32 * 4
    assert size(i64(0, 400), i64(135), 64) == 32 * 5 * 3                  # 265 positives, 135 negatives
    assert size(i64(0, 3, 403, 410), i64(3, 200, 0), 100) == 32 * 4 * 2   # one-class segments yield no items

    counts = torch.zeros(3, 1, 2, dtype=torch.int64)
    z, order = torch.zeros(3, 10), torch.arange(10, dtype=torch.int32)

    def plan(magic=0x6d695f6175635f31, N=10, S=1, items=1, device_table=True):
        p = _lib.AucPlan()
        p.device_table, p.magic, p.N, p.n_segments, p.n_items = (table.data_ptr() if device_table else None), magic, N, S, items
        return p

    def refused(match, p=None, stride=10, M=3, **nulls):
        a = dict(z=z, order=order, counts=counts)
        a.update(nulls)
        p = plan() if p is None else p
        rc = lib.mi_auc_pair_counts(C.byref(p) if p is not False else None, _lib.ptr(a["z"]), stride, M, _lib.ptr(a["order"]),
                                    _lib.ptr(a["counts"]), None)
        assert rc == -1 and match in err(), (rc, err())
    refused("auc_pair_counts: plan (not written by mi_auc_plan)", p=_lib.AucPlan())
    refused("auc_pair_counts: plan (not written by mi_auc_plan)", p=plan(magic=0x1234))
    refused("auc_pair_counts: plan (not written by mi_auc_plan)", p=plan(device_table=False))
    refused("auc_pair_counts: plan (not written by mi_auc_plan)", p=False)
    refused("auc_pair_counts: plan (damaged)", p=plan(N=0))
    for name in ("z", "order", "counts"):
        refused("auc_pair_counts: logits / order / counts", **{name: None})
    refused("auc_pair_counts: 0 members (1 to 1024)", M=0)
    refused("auc_pair_counts: 1025 members (1 to 1024)", M=1025)
    refused("auc_pair_counts: member_stride=9 below N=10", stride=9)
    assert not bool(counts.any()) and lib.mi_abi_version() == 21


def test_header_binding_library_and_stand_ins_agree_on_the_new_entries(lib):
    decls = _header_decls()
    for name, nargs in (("mi_auc_plan_bytes", 4), ("mi_auc_plan", 8), ("mi_auc_pair_counts", 7)):
        assert decls[name] == nargs == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    for name in ("mi_auc_plan", "mi_auc_pair_counts"):
        params = list(inspect.signature(getattr(AucKernels, name)).parameters.values())[1:]
        assert len(params) == len(_lib.SIGNATURES[name][1]) - 1, name
    assert _lib.ABI_VERSION == 21 and [f[0] for f in _lib.AucPlan._fields_] == ["device_table", "magic", "N", "n_segments", "n_items"]
    src = open(_header_path()).read()
    assert "#define MI_AUC_MAX_MEMBERS %d" % _lib.AUC_MAX_MEMBERS in src and ExactAuc.MAX_MEMBERS == _lib.AUC_MAX_MEMBERS


def _header_path():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_rec.h")
