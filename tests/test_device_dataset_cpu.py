"""CPU: the dataset that lives on the device (mi355x_rec/dataset.py) with the numpy stand-in for mi_batch_gather
(tests.batch_kernels) — its index streams, batches and raw features against the plain get_input_fn's, the order of its
evaluation batches, what it refuses, and what the real library refuses on the host before any launch."""
import inspect
import types

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, dataset, feature_column as fc
from mi355x_rec.dataset import DeviceBatch, DeviceDataset, materialise_group
from mi355x_rec.feature_column import FieldPlan
from tests.batch_kernels import BatchKernels, batch_kernels  # noqa: F401  (the fixture)
from tests.util import _header_decls
from trainers import _cli, deep_fm, ml_100k

SHAPES = [(1000, 96), (5000, 64)]        # 16 B > n: no draw, the whole pass is one shuffled buffer; pending crosses every pass


def _plan(mode="off"):
    """the MovieLens columns and one numeric feature, so that x is on the path too"""
    plan = FieldPlan(ml_100k.get_feature_columns()["linear"], [fc.numeric_column("timestamp")])
    plan.set_device_mode(mode)
    return plan


def _engine():
    return types.SimpleNamespace(device=torch.device("cpu"), k=BatchKernels(), shard=None)


@pytest.fixture
def rows_column(monkeypatch):
    """every file read gains a column `row` = the example's number and a timestamp that differs per example: a plain batch
    then tells which examples it holds"""
    reads = []
    orig = ml_100k._read_csv

    def read(path):
        cols, n = orig(path)
        cols["row"] = np.arange(n, dtype=np.int64)
        cols["timestamp"] = (np.arange(n) * 7 % 1013).astype(np.int32)
        reads.append(path)
        return cols, n
    monkeypatch.setattr(ml_100k, "_read_csv", read)
    return reads


def _pairs(n, B, count, mode="train"):
    """`count` batches of the plain input_fn and of the dataset's, same seed"""
    path = "synthetic:%d:3" % n
    plain = ml_100k.get_input_fn(path, mode, batch_size=B, seed=11)()
    ondev = ml_100k.get_input_fn(path, mode, batch_size=B, seed=11, device_dataset=True)()
    out = []
    for _ in range(count):
        p, d = next(plain, None), next(ondev, None)
        if p is None or d is None:
            assert p is None and d is None
            break
        out.append((p, d))
    return out


@pytest.mark.parametrize("n,B", SHAPES)
def test_index_streams_equal_the_plain_input_fns_over_three_passes(rows_column, n, B):
    pairs = _pairs(n, B, 3 * n // B + 1)
    assert len(pairs) == 3 * n // B + 1
    streams = set()
    for (pf, pl), (df, dl) in pairs:
        assert isinstance(df, DeviceBatch) and df.hi - df.lo == B == len(pl)
        assert np.array_equal(df.rows(), pf["row"]) and np.array_equal(dl, pl) and dl.dtype == bool
        streams.add(id(df.stream))
    assert len(streams) == 4 and n % B                              # a stream per pass; a batch straddles every pass boundary
    rows = np.concatenate([pf["row"] for (pf, _), _ in pairs])
    for p in range(3):                                              # every pass holds every example once: pending crossed over
        assert sorted(rows[p * n:(p + 1) * n].tolist()) == list(range(n))


@pytest.mark.parametrize("mode", ["off", "on"])
@pytest.mark.parametrize("n,B", SHAPES)
def test_every_batch_equals_the_plain_batchs_transform(rows_column, n, B, mode):
    plan, eng = _plan(mode), _engine()
    ref = _plan("off")
    count = (n // B + 2) if mode == "off" else 4                  # a whole pass and over its boundary
    for (pf, pl), (df, dl) in _pairs(n, B, count):
        (ids, x, y), status = df.materialise(plan, eng)
        status.raise_if_bad()
        want_ids, want_x = ref.transform(pf)
        assert ids.dtype == torch.int32 and x.dtype == torch.float32 and y.dtype == torch.uint8
        assert np.array_equal(ids.numpy(), want_ids) and np.array_equal(x.numpy(), want_x)
        assert np.array_equal(y.numpy(), pl.astype(np.uint8))
    ds = df.dataset
    assert ds.binds == 1 and tuple(ds.ids_all.shape) == (n, 26) and tuple(ds.x_all.shape) == (n, 1) and tuple(ds.y_all.shape) == (n,)
    assert eng.k.calls["mi_batch_gather"] == count                 # one call a batch


def test_raw_features_of_a_handle_are_the_plain_batchs(rows_column):
    for (pf, _), (df, _) in _pairs(1000, 96, 12):
        assert set(df) == set(pf) and len(df) == len(pf) and "user_id" in df and "no_such" not in df
        for key in ("user_id", "zipcode", "gender", "war"):
            assert np.array_equal(df[key], pf[key]) and df[key].dtype == pf[key].dtype
        with pytest.raises(KeyError):
            df["no_such"]


def test_a_group_is_formed_at_once_and_the_batches_are_its_rows(rows_column):
    """Estimator._grouped's group: one launch for consecutive batches of a pass, one more over a pass boundary"""
    n, B = 1000, 96
    plan, eng = _plan(), _engine()
    pairs = _pairs(n, B, 14)                                        # 10 whole batches a pass: batches 8..13 cross into pass 2
    for lo, hi, launches in ((0, 6, 1), (8, 14, 2)):
        handles = [df for _, (df, _) in pairs[lo:hi]]
        before = eng.k.calls.get("mi_batch_gather", 0)
        (ids, x, y), status = materialise_group(handles, plan, eng)
        status.raise_if_bad()
        assert eng.k.calls["mi_batch_gather"] - before == launches
        want = [plan.transform(pf) for (pf, _), _ in pairs[lo:hi]]
        assert np.array_equal(ids.numpy(), np.concatenate([w[0] for w in want]))
        assert np.array_equal(x.numpy(), np.concatenate([w[1] for w in want]))
        assert np.array_equal(y.numpy(), np.concatenate([pl for (_, pl), _ in pairs[lo:hi]]).astype(np.uint8))


def test_evaluation_batches_come_in_order_with_a_short_last_one(rows_column):
    plan, eng = _plan(), _engine()
    pairs = _pairs(150, 32, 9, mode="eval")
    assert [len(dl) for _, (_, dl) in pairs] == [32, 32, 32, 32, 22]
    for i, ((pf, pl), (df, dl)) in enumerate(pairs):
        assert df.stream is None and (df.lo, df.hi) == (32 * i, min(150, 32 * i + 32))
        (ids, x, y), status = df.materialise(plan, eng)
        assert status is None and np.array_equal(ids.numpy(), plan.transform(pf)[0]) and np.array_equal(dl, pl)
        assert np.array_equal(y.numpy(), pl.astype(np.uint8)) and np.array_equal(df["user_id"], pf["user_id"])
        # views of the resident arrays: no launch, no copy
        assert ids.data_ptr() == df.dataset.ids_all[df.lo:].data_ptr() and y.data_ptr() == df.dataset.y_all[df.lo:].data_ptr()
    assert "mi_batch_gather" not in eng.k.calls


def test_a_second_input_fn_call_reads_and_binds_nothing_again(rows_column):
    plan, eng = _plan(), _engine()
    input_fn = ml_100k.get_input_fn("synthetic:150:2", "eval", batch_size=64, device_dataset=True)
    assert rows_column == [] and input_fn.dataset() is None        # nothing is read before the first call
    for _ in range(3):
        for df, _ in input_fn():
            df.materialise(plan, eng)
    assert rows_column == ["synthetic:150:2"] and input_fn.dataset().binds == 1


def test_a_shard_and_a_dataset_that_does_not_fit_are_refused(monkeypatch, capsys):
    cols, n = ml_100k.synthetic_columns(300, 1)
    label = cols.pop("rating") >= 5
    ds = DeviceDataset(cols, label, n)
    plan = FieldPlan(ml_100k.get_feature_columns()["linear"])
    sharded = types.SimpleNamespace(device=torch.device("cpu"), k=BatchKernels(), shard=object())
    with pytest.raises(ValueError, match="device_dataset: one GPU only"):
        ds.bind(plan, sharded)
    assert ds.binds == 0 and ds.ids_all is None
    need = 300 * (4 * 26 + 1)
    monkeypatch.setattr(dataset, "_free_bytes", lambda device: need - 1)
    with pytest.raises(ValueError, match="device_dataset: the dataset needs %d bytes" % need):
        ds.bind(plan, _engine())
    assert ds.binds == 0 and ds.ids_all is None
    monkeypatch.setattr(dataset, "_free_bytes", lambda device: need)
    assert ds.bind(plan, _engine()).binds == 1
    with pytest.raises(ValueError, match="device_dataset: 3 examples and 2 labels"):
        DeviceDataset({"a": np.arange(3)}, np.zeros(2, bool), 3)
    # the CLI refuses the switch by name before any work, the model_fn too
    monkeypatch.setattr(_cli, "init_distributed", lambda args: (1, 2, "cpu", object()))
    args = _cli.make_parser("linear").parse_args(["--device-dataset", "on", "--synthetic", "100"])
    with pytest.raises(SystemExit, match="--device-dataset on: one GPU only"):
        _cli.run(args, lambda columns, config: pytest.fail("no estimator is built"))
    with pytest.raises(ValueError, match="device_dataset=on: one GPU only"):
        deep_fm.model_fn({}, None, "_build", {"categorical_columns": ml_100k.get_feature_columns()["linear"], "device": "cpu",
                                             "device_dataset": "on", "_shard": object()})
    with pytest.raises(ValueError, match="device_dataset must be 'off' or 'on'"):
        deep_fm.model_fn({}, None, "_build", {"categorical_columns": ml_100k.get_feature_columns()["linear"], "device": "cpu",
                                             "device_dataset": "auto"})


def test_bad_values_are_refused_at_bind_as_the_host_transform_refuses_them():
    cols, n = ml_100k.synthetic_columns(200, 1)
    label = cols.pop("rating") >= 5
    cols["war"] = cols["war"].copy()
    cols["war"][[57, 130]] = 5                                      # an identity column of 2 buckets and no default
    ref = FieldPlan(ml_100k.get_feature_columns()["linear"])
    with pytest.raises(ValueError) as host:
        ref.transform(cols)
    for mode in ("off", "on"):
        plan = FieldPlan(ml_100k.get_feature_columns()["linear"])
        plan.set_device_mode(mode)
        with pytest.raises(ValueError) as bound:
            DeviceDataset(cols, label, n).bind(plan, _engine())
        assert str(bound.value) == str(host.value)


def test_a_bad_index_raises_naming_the_first_bad_position():
    cols, n = ml_100k.synthetic_columns(100, 1)
    label = cols.pop("rating") >= 5
    ds = DeviceDataset(cols, label, n).bind(FieldPlan(ml_100k.get_feature_columns()["linear"]), _engine())
    stream = dataset._Pass(np.array([3, 100, 5, -1, 99, 0], np.int64))
    (ids, x, y), status = ds.gather([(stream, 1, 6)], "batch")
    assert x is None and ids[0].tolist() == [0] * 26 and ids[2].tolist() == [0] * 26 and y[0] == 0 and y[2] == 0
    assert torch.equal(ids[1], ds.ids_all[5]) and torch.equal(ids[3], ds.ids_all[99])
    with pytest.raises(ValueError, match="device_dataset: 2 of the batch's indices name no resident row; the first is at position 0"):
        status.raise_if_bad()


# ---- the switch through the trainers, kernels stood in by numpy --------------------------------------------------------
def test_device_dataset_on_trains_and_evaluates_to_the_same_numbers_on_a_cpu_device(tmp_path, monkeypatch, capsys, batch_kernels):
    fixed = lambda path, mode="train", batch_size=32, seed=None, **kw: ml_100k.get_input_fn(path, mode, batch_size=batch_size, seed=5, **kw)
    monkeypatch.setattr(_cli, "get_input_fn", fixed)
    opt = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")
    logs, finals = [], []
    for flag, transform in (("off", "off"), ("on", "off"), ("on", "on")):
        argv = ["--synthetic", "400", "--job-dir", str(tmp_path / (flag + transform)), "--train-steps", "30", "--batch-size", "16",
                "--device", "cpu", "--hidden-units", "8", "--device-dataset", flag, "--device-transform", transform, "--gauc-by", "user_id"]
        est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(argv))
        assert est.params["device_dataset"] == flag and est.global_step == 30
        calls = est._engine().k.calls
        assert ("mi_batch_gather" in calls) == (flag == "on")
        if flag == "on":
            assert calls["mi_batch_gather"] == 6                  # ONE group of 128 batches of 16: 2,048 rows, six passes of 400
        finals.append(est._engine().export_numpy())
        logs.append([l for l in capsys.readouterr().out.splitlines() if ("loss" in l.lower() or "Saving dict" in l) and "global_step/sec" not in l])
    assert logs[0] and any("gauc = " in l for l in logs[0]) and logs[0] == logs[1] == logs[2]
    for other in finals[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(finals[0]["emb"] + finals[0]["lin_w"], other["emb"] + other["lin_w"]))


def test_the_parsers_new_flag_and_its_default():
    for model, extra in (("deep_fm", ("hidden_units",)), ("linear", ()), ("deep", ("hidden_units",)), ("linear_deep", ("hidden_units",))):
        p = _cli.make_parser(model, extra)
        assert p.parse_args([]).device_dataset == "off" and p.parse_args(["--device-dataset", "on"]).device_dataset == "on"
        with pytest.raises(SystemExit):
            p.parse_args(["--device-dataset", "auto"])
    assert inspect.signature(ml_100k.get_input_fn).parameters["device_dataset"].default is False


# ---- the real library, without a device ---------------------------------------------------------------------------------
def test_the_library_refuses_on_the_host_before_it_touches_a_device(lib):
    err = lambda: lib.mi_last_error().decode()
    ids_all, x_all, y_all = torch.zeros(10, 4, dtype=torch.int32), torch.zeros(10, 2), torch.zeros(10, dtype=torch.uint8)
    order, status = torch.zeros(5, dtype=torch.int32), torch.full((2,), 7, dtype=torch.int32)
    ids, x, y = torch.full((5, 3), 7, dtype=torch.int32), torch.full((5, 2), 7.0), torch.full((5,), 7, dtype=torch.uint8)

    def refused(match, ld_ids=4, ld_x=2, N=10, B=5, F=3, n_num=2, **args):
        a = dict(ids_all=ids_all, x_all=x_all, y_all=y_all, order=order, ids=ids, x=x, y=y, status=status)
        a.update(args)
        rc = lib.mi_batch_gather(_lib.ptr(a["ids_all"]), ld_ids, _lib.ptr(a["x_all"]), ld_x, _lib.ptr(a["y_all"]), N, _lib.ptr(a["order"]),
                                 B, F, n_num, _lib.ptr(a["ids"]), _lib.ptr(a["x"]), _lib.ptr(a["y"]), _lib.ptr(a["status"]), None)
        assert rc == -1 and match in err(), (rc, err())
    for name in ("ids_all", "order", "ids", "status"):
        refused("batch_gather: null " + name, **{name: None})
    for bad in (0, -1, 2 ** 31):
        refused("batch_gather: N=%d" % bad, N=bad)
        refused("batch_gather: B=%d" % bad, B=bad)
    for bad in (0, -1, 65):
        refused("batch_gather: F=%d" % bad, F=bad, ld_ids=100)
    refused("batch_gather: ld_ids=2 < F=3", ld_ids=2)
    refused("batch_gather: n_num=-1", n_num=-1)
    refused("batch_gather: null x_all with n_num=2", x_all=None)
    refused("batch_gather: null x with n_num=2", x=None)
    refused("batch_gather: ld_x=1 < n_num=2", ld_x=1)
    refused("batch_gather: y is null and y_all is not", y=None)
    refused("batch_gather: y_all is null and y is not", y_all=None)
    assert bool((ids == 7).all()) and bool((x == 7).all()) and bool((y == 7).all()) and bool((status == 7).all())
    assert lib.mi_abi_version() == 21 == _lib.ABI_VERSION


def test_the_wrapper_checks_shapes_and_types_before_the_entry():
    k = BatchKernels()
    ids_all, y_all = torch.zeros(10, 4, dtype=torch.int32), torch.zeros(10, dtype=torch.uint8)
    order, status = torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    ids, y = torch.zeros(5, 4, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="order is torch.int64, not torch.int32"):
        dataset.batch_gather(k, ids_all, None, y_all, order.long(), ids, None, y, status)
    with pytest.raises(ValueError, match="come in pairs"):
        dataset.batch_gather(k, ids_all, None, y_all, order, ids, None, None, status)
    with pytest.raises(ValueError, match="order is int32 \\[B\\]"):
        dataset.batch_gather(k, ids_all, None, y_all, order[:4], ids, None, y, status)
    with pytest.raises(ValueError, match="ids_all is \\[N, >= F\\]"):
        dataset.batch_gather(k, ids_all[:, :3], None, y_all, order, ids, None, y, status)
    assert "mi_batch_gather" not in k.calls
    dataset.batch_gather(k, ids_all, None, None, order, ids, None, None, status)       # no labels: both NULL
    assert k.calls["mi_batch_gather"] == 1


def test_header_binding_library_and_stand_in_agree_on_the_new_entry(lib):
    assert _header_decls()["mi_batch_gather"] == 15 == len(_lib.SIGNATURES["mi_batch_gather"][1]) and hasattr(lib, "mi_batch_gather")
    params = list(inspect.signature(BatchKernels.mi_batch_gather).parameters.values())[1:]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params) and len(params) == 14
