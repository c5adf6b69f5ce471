"""CPU: the exact AUC / GAUC by sorting — ExactAuc(method="sorted"), StreamingExactAuc, Estimator.evaluate with
params["exact_auc"] / params["gauc_by"], the trainers' --exact-auc / --gauc-by and trainers.sweep's --auc-method — over the
numpy stand-ins of tests.sorted_auc_kernels, and what the real library decides on the host (mi_auc_sorted_counts'
refusals).  The real kernels are tested in test_hip_sorted_auc.py.

The reference everywhere is the brute force on the header's key, a few lines of numpy below."""
import inspect
import json

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, exact_auc
from mi355x_rec.exact_auc import ExactAuc, StreamingExactAuc
from tests.sorted_auc_kernels import SortedAucKernels, sorted_auc_kernels  # noqa: F401  (a fixture)
from tests.util import _header_decls, _t
from trainers import _cli, deep, deep_fm, linear, linear_deep, ml_100k

F32 = np.float32
OLD_KEYS = {"accuracy", "accuracy_baseline", "auc", "auc_precision_recall", "average_loss", "label/mean", "prediction/mean",
            "precision", "recall", "loss", "global_step"}
NEW_KEYS = {"auc_exact", "auc_exact_pairs"}
GAUC_KEYS = {"gauc", "gauc_groups"}
DEEP_FM = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")


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
    return [int((p > n).sum()), int((p == n).sum())]


def brute_groups(z, y, g):
    """per group in ascending order of its value: [gt, eq]"""
    return [brute(z[g == v], y[g == v]) for v in np.unique(g)]


def metrics_reference(z, y, g=None):
    P, Q = int(y.sum()), int((1 - y).sum())
    gt, eq = brute(z, y)
    out = {"auc_exact": (2 * gt + eq) / (2 * P * Q) if P * Q else 0.0, "auc_exact_pairs": P * Q}
    if g is not None:
        num = den = 0.0
        n = 0
        for v in np.unique(g):
            p, q = int(y[g == v].sum()), int((1 - y[g == v]).sum())
            if p and q:
                gt, eq = brute(z[g == v], y[g == v])
                num += (p + q) * ((2 * gt + eq) / (2 * p * q))
                den += p + q
                n += 1
        out.update(gauc=(num / den if n else 0.0), gauc_groups=n)
    return out


def same_metrics(got, want):
    assert set(got) == set(want)
    for name, v in want.items():
        assert got[name] == (pytest.approx(v, rel=1e-14, abs=0) if name == "gauc" else v), name


def logits(rng, M, N):
    """heavy ties with -0 / +0 and NaN in the first member, continuous values in the others"""
    z = rng.normal(0, 2, (M, N)).astype(F32)
    z[0] = rng.choice(np.array([-1.5, -0.0, 0.0, 0.75, 3.0], F32), N)
    z[0, rng.choice(N, 3, replace=False)] = np.nan
    return z


# ---- ExactAuc(method="sorted") ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
def test_sorted_gives_the_integers_of_pairs_and_of_the_brute_force(grouped):
    rng = np.random.default_rng(3)
    N = 700
    y = (rng.random(N) < 0.4).astype(np.uint8)
    sizes = np.array([1, 2, 300, 1, 2, 5, 389])
    g = np.repeat(np.arange(len(sizes)) * 10 - 7, sizes)[rng.permutation(N)] if grouped else None
    k = SortedAucKernels()
    a, b = ExactAuc(y, g, device="cpu", kernels=k), ExactAuc(y, g, device="cpu", kernels=k, method="sorted")
    assert "mi_auc_sorted_counts" not in k.calls and k.calls["mi_auc_plan"] == (2 if grouped else 1)     # sorted plans nothing
    wide = torch.from_numpy(np.concatenate([logits(rng, 3, N), np.full((3, 5), np.nan, F32)], 1))
    rows = wide[:, :N]                                                    # [M, N] at a stride of N + 5
    for z in (rows[1].contiguous(), rows):
        zs = z.numpy().reshape(-1, N)
        whole = b.counts(z)
        assert whole.dtype == torch.int64 and tuple(whole.shape) == (len(zs), 1, 2)
        assert torch.equal(whole, a.counts(z)) and whole[:, 0].tolist() == [brute(zm, y) for zm in zs]
        if grouped:
            by = b.counts(z, grouped=True)
            assert torch.equal(by, a.counts(z, grouped=True)) and by.tolist() == [brute_groups(zm, y, g) for zm in zs]
            assert list(b.group_values) == list(a.group_values) == list(np.unique(g))
        got = b.metrics(z)
        assert got == a.metrics(z)
        for m, zm in enumerate(zs):
            same_metrics(got[m], metrics_reference(zm, y, g))
    assert k.calls["mi_auc_sorted_counts"] >= 4
    if not grouped:
        with pytest.raises(ValueError, match="without groups"):
            b.counts(rows, grouped=True)
    with pytest.raises(ValueError, match="method must be 'pairs', 'sorted' or 'auto'"):
        ExactAuc(y, g, device="cpu", kernels=k, method="sort")
    assert inspect.signature(ExactAuc.__init__).parameters["method"].default == "pairs"


def test_auto_chooses_by_the_whole_sets_pairs(monkeypatch):
    """the constant is the measured crossover (profiles/sorted_auc.md); at and below it the pairs are compared, above it sorted"""
    assert ExactAuc.AUTO_PAIRS == 500_000_000
    y = np.array([1] * 30 + [0] * 50, np.uint8)                           # 1,500 pairs
    z = _t(np.random.default_rng(0).normal(0, 1, 80).astype(F32))
    k = SortedAucKernels()
    assert ExactAuc(y, device="cpu", kernels=k, method="auto").method == "pairs"
    want = ExactAuc(y, device="cpu", kernels=k).metrics(z)
    for limit, method in ((1500, "pairs"), (1499, "sorted")):
        monkeypatch.setattr(ExactAuc, "AUTO_PAIRS", limit)
        ex = ExactAuc(y, device="cpu", kernels=k, method="auto")
        assert ex.method == method and ex.metrics(z) == want
    assert k.calls["mi_auc_sorted_counts"] == 1


# ---- StreamingExactAuc --------------------------------------------------------------------------------------------------
def test_streaming_in_uneven_batches_is_exact_auc_on_the_concatenation():
    rng = np.random.default_rng(8)
    N = 500
    y = (rng.random(N) < 0.45).astype(np.uint8)
    z = logits(rng, 1, N)[0]
    names = np.array(["user-%d" % (7 * v % 11) for v in rng.integers(0, 40, N)], dtype=object)
    cuts = [0, 1, 130, 131, 400, N]
    k = SortedAucKernels()
    for groups in (None, names, rng.integers(-5, 30, N)):
        acc = StreamingExactAuc("cpu", k)
        for turn in range(2):                                             # (the second turn after reset(): nothing is left over)
            for lo, hi in zip(cuts, cuts[1:]):
                g = None
                if groups is not None:
                    g = groups[lo:hi]
                    if groups is names:                                    # the strings of a batch in another order in every batch
                        assert len(set(g)) > 1 or hi - lo == 1
                acc.add(_t(z[lo:hi]), _t(y[lo:hi]), g)
            got = acc.metrics()
            whole = ExactAuc(y, groups, device="cpu", kernels=k).metrics(_t(z))[0]
            assert got == whole
            same_metrics(got, metrics_reference(z, y, groups))
            acc.reset()
        with pytest.raises(ValueError, match="nothing was added"):
            acc.metrics()
    # the first appearances of the strings differ from batch to batch, and the numbering is the values' ascending order
    firsts = [list(dict.fromkeys(names[lo:hi])) for lo, hi in zip(cuts, cuts[1:]) if hi - lo > 100]
    assert firsts[0][:5] != firsts[1][:5] and firsts[0][:5] != sorted(firsts[0][:5])
    acc = StreamingExactAuc("cpu", k)
    acc.add(_t(z[:10]), _t(y[:10]), names[:10])
    with pytest.raises(ValueError, match="every batch of a set comes with groups, or none does"):
        acc.add(_t(z[10:20]), _t(y[10:20]))
    with pytest.raises(ValueError, match="one label a logit"):
        acc.add(_t(z[:10]), _t(y[:9]), names[:10])
    with pytest.raises(ValueError, match="groups must be 10 integers or strings"):
        acc.add(_t(z[:10]), _t(y[:10]), np.zeros(10))
    # non-zero labels are positives, and the accumulator keeps its own copy of the logits
    acc = StreamingExactAuc("cpu", k)
    buf = _t(z[:50].copy())
    acc.add(buf, _t((y[:50] * 7).astype(np.uint8)))
    buf.zero_()
    same_metrics(acc.metrics(), metrics_reference(z[:50], y[:50]))


# ---- Estimator.evaluate -------------------------------------------------------------------------------------------------
def _estimator(tmp_path, *flags):
    return deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", DEEP_FM).parse_args(
        ["--synthetic", "400", "--train-steps", "20", "--batch-size", "16", "--device", "cpu", "--hidden-units", "8", "8",
         "--job-dir", str(tmp_path / "job")] + list(flags)))


@pytest.fixture
def recorded(monkeypatch):
    """what StreamingExactAuc.add was handed, batch by batch"""
    seen = []
    add = StreamingExactAuc.add

    def recording(self, z, y, groups=None):
        seen.append((z.detach().numpy().reshape(-1).copy(), y.detach().numpy().reshape(-1).copy(),
                     None if groups is None else np.asarray(groups).reshape(-1).copy()))
        return add(self, z, y, groups)
    monkeypatch.setattr(exact_auc.StreamingExactAuc, "add", recording)
    return seen


def test_evaluate_adds_exactly_the_four_keys_and_keeps_todays(sorted_auc_kernels, recorded, tmp_path, capsys):  # noqa: F811
    est = _estimator(tmp_path)
    line = [l for l in capsys.readouterr().out.splitlines() if "Saving dict for global step 20" in l][-1]
    assert " auc = " in line and "auc_exact" not in line and "gauc" not in line
    eval_fn = ml_100k.get_input_fn("synthetic:300:2", "eval", 64)
    plain = est.evaluate(eval_fn)
    assert set(plain) == OLD_KEYS and not recorded
    assert "mi_auc_sorted_counts" not in est._engine().k.calls and "exact_auc" not in est.params["_store"]
    est.params["exact_auc"] = True
    exact = est.evaluate(eval_fn)
    assert set(exact) == OLD_KEYS | NEW_KEYS and {name: exact[name] for name in plain} == plain
    assert len(recorded) == 5 and all(g is None for _, _, g in recorded)
    z, y = (np.concatenate(c) for c in list(zip(*recorded))[:2])
    same_metrics({name: exact[name] for name in NEW_KEYS}, metrics_reference(z, y))
    del recorded[:]
    est.params["gauc_by"] = "gender"
    both = est.evaluate(eval_fn)                                          # (the accumulator starts over with the evaluation)
    assert set(both) == OLD_KEYS | NEW_KEYS | GAUC_KEYS and {name: both[name] for name in exact} == exact
    z2, y2, g = (np.concatenate(c) for c in zip(*recorded))
    assert np.array_equal(z2, z) and len(g) == 300 and both["gauc_groups"] == 2
    same_metrics({name: both[name] for name in NEW_KEYS | GAUC_KEYS}, metrics_reference(z, y, g))
    del est.params["exact_auc"]                                           # gauc_by alone implies the exact AUC
    assert est.evaluate(eval_fn) == both
    est.params["gauc_by"] = "nosuch"
    with pytest.raises(ValueError, match=r"gauc_by='nosuch': the batch has no such feature \(it has action, adventure, age, .*user_id"):
        est.evaluate(eval_fn)
    del est.params["gauc_by"]
    assert est.evaluate(eval_fn) == plain


# ---- the four CLIs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trainer,extra", [(deep_fm, DEEP_FM), (linear, ()), (deep, ("hidden_units", "dropout")),
                                           (linear_deep, ("hidden_units", "dropout"))])
def test_the_trainers_take_the_flags(trainer, extra, sorted_auc_kernels, tmp_path, capsys):  # noqa: F811
    name = trainer.__name__.split(".")[-1]
    parser = _cli.make_parser(name, extra)
    a = parser.parse_args([])
    assert a.exact_auc is False and a.gauc_by is None
    a = parser.parse_args(["--exact-auc", "--gauc-by", "user_id"])
    assert a.exact_auc is True and a.gauc_by == "user_id"
    base = ["--synthetic", "300", "--train-steps", "5", "--batch-size", "16", "--device", "cpu", "--job-dir", str(tmp_path / "job")]
    with pytest.raises(SystemExit, match=r"--gauc-by nosuch: the test file has no such column \(it has action, adventure, age, .*user_id"):
        trainer.train_and_evaluate(parser.parse_args(base + ["--gauc-by", "nosuch"]))
    capsys.readouterr()
    est = trainer.train_and_evaluate(parser.parse_args(base + ["--gauc-by", "gender"]))      # implies --exact-auc
    assert est.params["exact_auc"] is True and est.params["gauc_by"] == "gender"
    line = [l for l in capsys.readouterr().out.splitlines() if "Saving dict for global step 5" in l][-1]
    assert all(" %s = " % key_ in line for key_ in ("auc", "auc_exact", "auc_exact_pairs", "gauc", "gauc_groups"))
    est = trainer.train_and_evaluate(parser.parse_args(base + ["--exact-auc"]))
    assert est.params["exact_auc"] is True and "gauc_by" not in est.params
    line = [l for l in capsys.readouterr().out.splitlines() if "Saving dict for global step 5" in l][-1]
    assert " auc_exact = " in line and "gauc" not in line


# ---- trainers.sweep -----------------------------------------------------------------------------------------------------
def test_sweep_counts_the_same_with_either_method(sorted_auc_kernels, tmp_path, monkeypatch):  # noqa: F811
    from trainers import sweep
    assert sweep.make_parser().parse_args([]).auc_method == "pairs"
    docs, built = {}, []

    class Recorded(ExactAuc):
        def __init__(self, *a, **kw):
            ExactAuc.__init__(self, *a, **kw)
            built.append(self)
    monkeypatch.setattr(sweep, "ExactAuc", Recorded)
    # both runs train on the same shuffle of the data: the same members, so the same logits to count
    real = sweep.get_input_fn
    monkeypatch.setattr(sweep, "get_input_fn", lambda path, mode="train", batch_size=32: real(path, mode, batch_size=batch_size, seed=0))
    for method in ("pairs", "sorted"):
        job = tmp_path / method
        sweep.train_and_evaluate(sweep.make_parser().parse_args(
            ["--synthetic", "400", "--train-steps", "20", "--job-dir", str(job), "--batch-size", "16", "--device", "cpu",
             "--hidden-units", "8", "8", "--learning-rate", "0.001", "0.01", "--exact-auc", "--gauc-by", "gender",
             "--auc-method", method]))
        calls = built[-1].k.calls
        assert built[-1].method == method and ("mi_auc_sorted_counts" in calls) == (method == "sorted")
        assert ("mi_auc_pair_counts" in calls) == (method == "pairs")
        docs[method] = json.load(open(job / "sweep.json"))["members"]
    assert len(docs["pairs"]) == 2 and len(built) == 2
    for a, b in zip(docs["pairs"], docs["sorted"]):
        assert a["metrics"] == b["metrics"] and a["metrics"]["gauc_groups"] == 2 and 0.0 < a["metrics"]["auc_exact"] < 1.0


# ---- the real library, without a device ---------------------------------------------------------------------------------
def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    err = lambda: lib.mi_last_error().decode()
    N = 10
    z, y, g = torch.zeros(3, N), torch.ones(N, dtype=torch.uint8), torch.zeros(N, dtype=torch.int32)
    counts = torch.full((3, 4, 2), 7, dtype=torch.int64)
    nbytes = lib.mi_auc_sorted_workspace_bytes(N, 4)
    assert nbytes >= 16 * N and lib.mi_auc_sorted_workspace_bytes(N, 1) > 0 and lib.mi_auc_sorted_workspace_bytes(2 ** 31 - 1, 1) > 2 ** 35
    ws = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8)

    def refused(status, match, stride=N, M=3, S=4, n=N, size=nbytes, **args):
        a = dict(z=z, y=y, g=g, counts=counts, ws=ws)
        a.update(args)
        rc = lib.mi_auc_sorted_counts(_lib.ptr(a["z"]), stride, M, _lib.ptr(a["y"]), _lib.ptr(a["g"]), S, n, _lib.ptr(a["counts"]),
                                      _lib.ptr(a["ws"]), size, None)
        assert rc == status and match in err(), (rc, err())
    for name in ("z", "y", "counts", "ws"):
        refused(-1, "auc_sorted_counts: logits / labels / counts / workspace", **{name: None})
    refused(-1, "auc_sorted_counts: N=0 examples (1 to 2147483647)", n=0, stride=0)
    refused(-1, "auc_sorted_counts: N=-3 examples", n=-3)
    refused(-1, "auc_sorted_counts: N=2147483648 examples (1 to 2147483647)", n=2 ** 31, stride=2 ** 31)
    refused(-1, "auc_sorted_counts: 0 groups (at least 1)", S=0)
    refused(-1, "auc_sorted_counts: -2 groups (at least 1)", S=-2)
    refused(-1, "auc_sorted_counts: groups is NULL with 4 groups", g=None)
    refused(-1, "auc_sorted_counts: 0 members (1 to 1024)", M=0)
    refused(-1, "auc_sorted_counts: 1025 members (1 to 1024)", M=1025)
    refused(-1, "auc_sorted_counts: member_stride=9 below N=10", stride=9)
    refused(-4, "auc_sorted_counts: workspace of %d bytes, %d needed" % (nbytes - 1, nbytes), size=nbytes - 1)
    refused(-4, "auc_sorted_counts: workspace of 0 bytes", size=0)
    refused(-1, "auc_sorted_counts: workspace (16-byte aligned)", ws=ws[8:])
    assert bool((counts == 7).all()) and bool((ws == 0xA5).all())
    for bad in ((0, 1), (-1, 1), (2 ** 31, 1), (N, 0), (N, -1)):
        assert lib.mi_auc_sorted_workspace_bytes(*bad) == 0, bad
    assert lib.mi_abi_version() == 21 == _lib.ABI_VERSION


def test_header_binding_library_and_stand_in_agree_on_the_new_entries(lib):
    decls = _header_decls()
    for name, nargs in (("mi_auc_sorted_workspace_bytes", 2), ("mi_auc_sorted_counts", 11)):
        assert decls[name] == nargs == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    params = list(inspect.signature(SortedAucKernels.mi_auc_sorted_counts).parameters.values())[1:]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params) and len(params) == len(_lib.SIGNATURES["mi_auc_sorted_counts"][1]) - 1
