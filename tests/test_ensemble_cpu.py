"""CPU: the host side of serving an ensemble — EnsemblePredictor (its refusals, from_exports / from_sweep, the three modes,
its buffers) and the two CLIs' new flags.  mi_predict_group_plan / mi_predict_group are stood in by a numpy restatement of
their contract in include/mi355x_rec.h (tests.cpu_kernels.NumpyKernels: member i's logit is that engine's predict_logits on
the CPU, the mean is formed in fp32 in member order); the real kernel is tested in test_hip_ensemble.py.  The binding is
checked against the real library."""
import copy
import csv
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from mi355x_rec.engine import DeepFM
from mi355x_rec.predictor import EnsemblePredictor, FusedGroup, Predictor
from tests.cases import _sweep_args
from tests.cpu_kernels import NumpyKernels, cpu_kernels  # noqa: F401  (a fixture)
from tests.util import _fake_sweep, _header_decls, _requests, _train_deep_fm_export, max_err_scaled
from trainers import ml_100k, predict

F32 = np.float32


@pytest.fixture(scope="module")
def exports(tmp_path_factory):
    """two small trained deep_fm exports that differ in embedding size and layers (trained once for the module)"""
    root = str(tmp_path_factory.mktemp("ens"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine, "HipKernels", NumpyKernels)
        return [_train_deep_fm_export(root, "a", ["--embedding-size", "4", "--hidden-units", "8", "8"]),
                _train_deep_fm_export(root, "b", ["--embedding-size", "8", "--hidden-units", "8"])]


def _members(exports, **kw):
    ps = [Predictor.from_export(d, device="cpu", **kw) for d in exports]
    NumpyKernels.register([p.engine for p in ps])
    return ps


def test_modes_agree_and_the_mean_is_fp32_in_member_order(cpu_kernels, exports):
    ps = _members(exports)
    feats = _requests()
    solo = [p(feats)["logits"][:, 0] for p in ps]
    out = {}
    for mode in ("fused", "layered", "auto"):
        ens = EnsemblePredictor(ps, mode=mode)
        out[mode] = ens(feats, return_members=True)
        got = out[mode]
        assert set(got) == {"logits", "logistic", "probabilities", "class_ids", "classes", "member_logits"}
        assert got["logits"].shape == (30, 1) and got["probabilities"].shape == (30, 2) and got["class_ids"].dtype == np.int64
        assert got["member_logits"].shape == (2, 30) and got["member_logits"].dtype == np.float32
        want = ((got["member_logits"][0] + got["member_logits"][1]) / F32(2)).astype(F32)
        assert np.array_equal(got["logits"][:, 0], want)
        assert np.array_equal(got["class_ids"][:, 0], (got["logistic"][:, 0] > 0.5).astype(np.int64))
        for i in range(2):
            assert max_err_scaled(got["member_logits"][i], solo[i]) < 1e-5
        assert "member_logits" not in ens(feats)
    assert max_err_scaled(out["fused"]["logits"], out["layered"]["logits"]) < 1e-5
    # one member: the member itself (a division by 1 is exact)
    one = EnsemblePredictor(ps[:1], mode="fused")(feats)
    assert max_err_scaled(one["logits"][:, 0], solo[0]) < 1e-5
    assert EnsemblePredictor(ps, mode="fused").predict_ids(np.zeros((0, ps[0].engine.F), np.int32))["logits"].shape == (0, 1)


def test_refusals_name_the_difference(cpu_kernels, exports):
    ps = _members(exports)
    with pytest.raises(ValueError, match="no members"):
        EnsemblePredictor([])
    with pytest.raises(ValueError, match="mode"):
        EnsemblePredictor(ps, mode="eager")
    # columns: a bucket count
    sig = copy.deepcopy(ps[1].signature)
    col = sig["model"]["categorical_columns"][2]
    col["num_buckets"] += 1
    with pytest.raises(ValueError, match=r"member 1 differs from member 0 in categorical column 2 \(%r\): num_buckets" % col["name"]):
        EnsemblePredictor([ps[0], Predictor(sig, ps[1].plan, ps[1].engine)])
    # columns: one fewer
    sig = copy.deepcopy(ps[1].signature)
    sig["model"]["categorical_columns"].pop()
    with pytest.raises(ValueError, match="member 1 has %d categorical columns, member 0 has %d" % (ps[0].engine.F - 1, ps[0].engine.F)):
        EnsemblePredictor([ps[0], Predictor(sig, ps[1].plan, ps[1].engine)])
    # receivers
    sig = copy.deepcopy(ps[1].signature)
    key = sorted(sig["receiver_tensors"])[0]
    sig["receiver_tensors"][key] = "int64"
    with pytest.raises(ValueError, match="member 1 differs from member 0 in receiver %r" % key):
        EnsemblePredictor([ps[0], Predictor(sig, ps[1].plan, ps[1].engine)])
    # devices
    far = copy.copy(ps[1].engine)
    far.device = torch.device("cuda:1")
    with pytest.raises(ValueError, match="member 1 is on device cuda:1, member 0 on cpu"):
        EnsemblePredictor([ps[0], Predictor(ps[1].signature, ps[1].plan, far)])
    # members that differ in embedding size and layers are what an ensemble is for
    assert ps[0].engine.E != ps[1].engine.E
    EnsemblePredictor(ps)


def test_fused_mode_refuses_a_member_outside_the_kernels_scope_and_auto_follows_the_members(cpu_kernels, exports):
    ps = _members(exports)
    lead = ps[0].engine
    big = DeepFM(lead.vocab_sizes, embedding_size=4, hidden_units=[1024], device="cpu")
    wide = Predictor(ps[0].signature, ps[0].plan, big)
    with pytest.raises(ValueError, match="member 1: the model has a hidden layer of 1024 units"):
        EnsemblePredictor([ps[0], wide], mode="fused")
    with pytest.raises(ValueError, match="member 1: the model has a hidden layer of 1024 units"):
        FusedGroup([lead, big])
    ens = EnsemblePredictor([ps[0], wide], mode="auto")                  # auto: allowed, and never fused
    assert not ens.use_fused(1) and EnsemblePredictor(ps, mode="auto").use_fused(32)
    assert not EnsemblePredictor(ps, mode="auto").use_fused(8192)        # the members' own batch threshold
    assert not EnsemblePredictor(ps, mode="layered").use_fused(1) and EnsemblePredictor(ps, mode="fused").use_fused(8192)
    lay = _members(exports[1:], mode="layered")
    assert not EnsemblePredictor([ps[0], lay[0]], mode="auto").use_fused(32)
    # auto on such a pair runs every member by its own path and no group launch
    k = ps[0].engine.k
    k.calls.clear()
    EnsemblePredictor([ps[0], lay[0]], mode="auto")(_requests(5))
    assert "mi_predict_group" not in k.calls and k.calls.get("mi_predict_fused", 0) == 1


def test_the_plan_is_built_once_buffers_are_kept_per_batch_size_and_ids_are_transformed_once(cpu_kernels, exports, monkeypatch):
    ps = _members(exports)
    ens = EnsemblePredictor(ps, mode="fused")
    k = ens.k
    k.calls.clear()
    transforms = []
    for p in ps:
        real = p.plan.transform
        monkeypatch.setattr(p.plan, "transform", lambda cols, real=real: transforms.append(1) or real(cols))
    a = ens(_requests(30))
    bufs30 = ens._bufs[30]
    ens(_requests(30, seed=3))
    ens(_requests(7))
    b = ens(_requests(30))
    assert len(transforms) == 4                                          # once per call, not once per member
    assert k.calls.get("mi_predict_group_plan", 0) == 1 and k.calls.get("mi_predict_group", 0) == 4
    assert "mi_predict_fused" not in k.calls and all("mi_predict_fused" not in p.engine.k.calls for p in ps)
    assert ens._bufs[30] is bufs30 and sorted(ens._bufs) == [7, 30]
    assert not bool(bufs30["tickets"].any()) and bufs30["tickets"].numel() == 1
    assert np.array_equal(a["logits"], b["logits"]) and a["logits"] is not b["logits"]     # host copies, not views of the buffer


def test_from_sweep_takes_the_first_rows_in_order(cpu_kernels, exports, tmp_path):
    job = _fake_sweep(str(tmp_path), exports)
    ens = EnsemblePredictor.from_sweep(job, top=2, device="cpu")
    assert ens.sweep_members == [1, 0] and [p.engine.E for p in ens.members] == [8, 4]
    assert [os.path.dirname(d) for d in ens.export_dirs] == [exports[1], exports[0]]
    assert EnsemblePredictor.from_sweep(job, top=1, device="cpu").sweep_members == [1]
    for top in (0, -1, 3):
        with pytest.raises(ValueError, match="top=%d: the sweep in .* has 2 members" % top):
            EnsemblePredictor.from_sweep(job, top=top, device="cpu")
    with pytest.raises(FileNotFoundError, match="no sweep.json"):
        EnsemblePredictor.from_sweep(str(tmp_path / "nothing"), top=1, device="cpu")
    NumpyKernels.register([p.engine for p in ens.members])
    got = ens(_requests(9), return_members=True)
    solo = [Predictor.from_export(exports[m], device="cpu", mode="layered")(_requests(9))["logits"][:, 0] for m in (1, 0)]
    for i in range(2):
        assert max_err_scaled(got["member_logits"][i], solo[i]) < 1e-5


def test_predict_cli_top(cpu_kernels, exports, tmp_path, monkeypatch):
    a = predict.make_parser().parse_args(["--job-dir", "x", "--input", "y"])
    assert a.top is None                                                 # without --top nothing changes
    assert predict.make_parser().parse_args(["--job-dir", "x", "--input", "y", "--top", "3"]).top == 3
    with pytest.raises(SystemExit, match="no sweep.json"):
        predict.main(["--job-dir", os.path.dirname(os.path.dirname(exports[0])), "--input", "synthetic:5:1", "--top", "1",
                      "--device", "cpu"])
    job = _fake_sweep(str(tmp_path), exports)
    real = EnsemblePredictor.from_sweep.__func__

    def registered(cls, *a, **kw):
        ens = real(cls, *a, **kw)
        NumpyKernels.register([p.engine for p in ens.members])
        return ens
    monkeypatch.setattr(EnsemblePredictor, "from_sweep", classmethod(registered))
    out = predict.main(["--job-dir", job, "--input", "synthetic:23:5", "--top", "2", "--device", "cpu", "--batch-size", "10"])
    rows = list(csv.DictReader(open(out)))
    assert out == os.path.join(job, "predict", "predictions.csv") and len(rows) == 23
    cols, _ = ml_100k._read_csv("synthetic:23:5")
    ens = EnsemblePredictor.from_sweep(job, top=2, device="cpu")
    want = ens({k: v for k, v in cols.items() if k in ens.receivers})["logits"][:, 0]
    assert np.array_equal(np.asarray([float(r["logit"]) for r in rows], F32), want)


def test_sweep_ensemble_flag(cpu_kernels, tmp_path, capsys, monkeypatch):
    from trainers import sweep
    assert sweep.make_parser().parse_args([]).ensemble == 0
    real = EnsemblePredictor.from_sweep.__func__

    def registered(cls, *a, **kw):
        ens = real(cls, *a, **kw)
        NumpyKernels.register([p.engine for p in ens.members])
        return ens
    monkeypatch.setattr(EnsemblePredictor, "from_sweep", classmethod(registered))
    grid = ["--learning-rate", "0.001", "0.01", "--seeds", "2"]
    job = tmp_path / "off"
    sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "6", "--ensemble", "0", *grid))
    assert "ensemble" not in json.load(open(job / "sweep.json")) and "INFO: ensemble of" not in capsys.readouterr().out
    job = tmp_path / "on"
    sweep.train_and_evaluate(_sweep_args(job, "--train-steps", "6", "--ensemble", "3", *grid))
    doc = json.load(open(job / "sweep.json"))
    assert doc["ensemble"]["members"] == [r["member"] for r in doc["members"][:3]]
    keys = {"accuracy", "accuracy_baseline", "auc", "auc_precision_recall", "average_loss", "label/mean", "prediction/mean",
            "precision", "recall", "loss"}
    assert set(doc["ensemble"]["metrics"]) == keys and all(np.isfinite(v) for v in doc["ensemble"]["metrics"].values())
    assert doc["ensemble"]["metrics"]["label/mean"] == pytest.approx(doc["members"][0]["metrics"]["label/mean"])
    out = capsys.readouterr().out
    assert "INFO: ensemble of the 3 best members" in out and "auc = " in out and "the best single member (member %d)" % doc["members"][0]["member"] in out
    with pytest.raises(ValueError, match="--ensemble 5: the sweep has 4 members"):
        sweep.train_and_evaluate(_sweep_args(tmp_path / "bad", "--train-steps", "2", "--ensemble", "5", *grid))


def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    """what the real library decides on the host, with no GPU: the member count, a plan it did not write"""
    import ctypes as C
    members = (_lib.ServeMember * 1)()
    plan = _lib.ServeGroupPlan()
    err = lambda: lib.mi_last_error().decode()
    assert lib.mi_predict_group_plan_bytes(0) == 0 and lib.mi_predict_group_plan_bytes(3) == 3 * lib.mi_predict_group_plan_bytes(1)
    assert lib.mi_predict_group_plan(members, 0, 3, 0, None, None, C.byref(plan), None) == -1 and "0 members (at least 1)" in err()
    assert lib.mi_predict_group_plan(members, 257, 3, 0, None, None, C.byref(plan), None) == -2 and "257 members (at most 256" in err()
    assert plan.magic == 0 and plan.device_table is None
    # a zeroed plan, a NULL plan
    assert lib.mi_predict_group(C.byref(plan), 1, None, None, 4, None, None, None, None, None, None, None) == -1
    assert "not written by mi_predict_group_plan" in err()
    assert lib.mi_predict_group(None, 1, None, None, 4, None, None, None, None, None, None, None) == -1


def test_header_binding_and_library_agree_on_the_new_entries(lib):
    decls = _header_decls()
    for name, nargs in (("mi_predict_group_plan_bytes", 1), ("mi_predict_group_plan", 8), ("mi_predict_group", 12)):
        assert decls[name] == nargs == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    assert lib.mi_abi_version() == 21
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_rec.h")).read()
    assert "#define MI_PREDICT_GROUP_MAX_MEMBERS %d" % _lib.PREDICT_GROUP_MAX_MEMBERS in src
