"""CPU: the device transform's host side — the lowering of a FieldPlan to mi_ids_transform's descriptor table, the refused
columns, the one blob-and-offsets encoder, the status contract and the switches — with the table run by the host entries
(what DeviceTransform does on a CPU device).  Everything is equality with FieldPlan.transform."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, feature_column as fc
from mi355x_rec.device_transform import DeviceTransform, vocabulary_table
from mi355x_rec.feature_column import FieldPlan, encode_strings
from trainers import _cli, deep_fm, ml_100k, predict, recommend, sweep


def _ml100k():
    cols, _ = ml_100k.synthetic_columns(257, seed=3)
    return FieldPlan(ml_100k.get_feature_columns()["linear"]), cols


def test_descriptor_table_of_the_ml_100k_plan():
    plan, _ = _ml100k()
    dt = plan.device_transform("cpu")
    assert isinstance(dt, DeviceTransform) and dt.refused == [] and dt.runs == [[0, 26]]
    table = dt.table()
    assert [d["name"] for d in table] == [c.name for c in plan.categorical] and [d["field"] for d in table] == list(range(26))
    by = {d["name"]: d for d in table}
    assert by["user_id"] == {"field": by["user_id"]["field"], "name": "user_id", "key": "user_id", "family": "hash_bucket",
                             "num_buckets": 1000, "n_table": 0, "num_oov": 0, "default": -1}
    assert (by["age_bucketized"]["family"], by["age_bucketized"]["key"], by["age_bucketized"]["n_table"],
            by["age_bucketized"]["num_buckets"]) == ("bucketized", "age", 6, 7)
    assert (by["gender"]["family"], by["gender"]["n_table"], by["gender"]["num_oov"], by["gender"]["num_buckets"]) == (
        "vocabulary_list", 2, 1, 3)
    assert all(by[g]["family"] == "identity" and by[g]["num_buckets"] == 2 and by[g]["default"] == -1 for g in ml_100k.GENRE)
    # the batch decides the kinds of hash_bucket and identity columns: int32 columns here, strings for occupation / zipcode
    _, cols = _ml100k()
    descr, _, B = dt.descriptors(cols, 0, 26)
    kinds = {c.name: descr[f].kind for f, c in enumerate(plan.categorical)}
    assert B == 257 and kinds["user_id"] == _lib.IDS_HASH_I32 and kinds["zipcode"] == _lib.IDS_HASH_BYTES
    assert kinds["gender"] == _lib.IDS_VOCAB_BYTES and kinds["age_bucketized"] == _lib.IDS_BUCKETIZE_F32
    assert kinds["war"] == _lib.IDS_IDENTITY_I32
    cols["user_id"] = cols["user_id"].astype(np.int64)
    assert dt.descriptors(cols, 0, 26)[0][[c.name for c in plan.categorical].index("user_id")].kind == _lib.IDS_HASH_I64


def test_vocabulary_table_layout(lib):
    vocab = ["pear", "apple", "fig"]
    raw = vocabulary_table(vocab)
    n = 3
    fp = raw[:8 * n].view(np.uint64)
    start = raw[8 * n:8 * n + 8 * (n + 1)].view(np.int64)
    index = raw[8 * n + 8 * (n + 1):8 * n + 8 * (n + 1) + 4 * (n + 1)].view(np.int32)       # (n odd: 4 bytes of padding)
    text = raw[8 * n + 8 * (n + 1) + 4 * (n + 1):].tobytes()
    assert np.all(fp[1:] > fp[:-1]) and sorted(index[:n]) == [0, 1, 2] and index[n] == 0
    for j in range(n):
        word = text[start[j]:start[j + 1]]
        assert word == vocab[index[j]].encode() and fp[j] == lib.mi_fingerprint64(word, len(word))


def test_refused_columns_and_their_reasons(capsys):
    cols = [fc.categorical_column_with_vocabulary_list("a", [1, 2, 3], num_oov_buckets=1),
            fc.categorical_column_with_vocabulary_list("b", ["x", "y", "x"], num_oov_buckets=1),
            fc.categorical_column_with_hash_bucket("c", 10, np.float32),
            fc.categorical_column_with_hash_bucket("d", 10),
            fc.categorical_column_with_identity("e", 4)]
    plan = FieldPlan(cols)
    dt = plan.device_transform("cpu")
    assert dt.refused == [(0, "a", "vocabulary with entries that are not strings"), (1, "b", "vocabulary with duplicate entries"),
                          (2, "c", "hash_bucket of dtype float32: neither integers nor strings")]
    assert dt.runs == [[3, 5]]
    feats = {"a": [1, 7, 3, 2], "b": ["x", "y", "q", "x"], "c": [0.5, 1.5, 0.5, 2.0], "d": ["u", "v", "", "u"], "e": [0, 3, 1, 2]}
    ids, x = dt.transform(feats)                              # the refused columns: transformed on the host and merged
    assert x is None and torch.equal(ids, torch.from_numpy(plan.transform(feats)[0]))
    plan.on_device("cpu")
    plan.on_device("cpu")
    out = capsys.readouterr().out
    assert out.count("stays on the host transform") == 3 and "column 'b' stays on the host transform: vocabulary with duplicate" in out


@pytest.mark.parametrize("values", [
    ["a", "bc", "", "def", "a"], ["é", "日本", "x", ""], ["nul\x00", "x", "\x00"], [b"raw", b"\xff\x00", b""],
    np.array([b"ab", b"c", b""], dtype="S"), np.array(["u", "vw"], dtype="U"), [1.5, "x", None, 7]])
def test_encoder_against_the_per_element_definition(values):
    blob, offs = encode_strings(values)
    want = [v if isinstance(v, bytes) else str(v).encode("utf-8") for v in values]
    assert offs.dtype == np.int64 and offs[0] == 0 and len(offs) == len(want) + 1
    assert [bytes(blob[offs[i]:offs[i + 1]]) for i in range(len(want))] == want


def test_cpu_execution_of_the_table_equals_the_host_transform():
    plan, cols = _ml100k()
    dt = plan.device_transform("cpu")
    ids, x = dt.transform(cols)
    assert x is None and ids.dtype == torch.int32 and torch.equal(ids, torch.from_numpy(plan.transform(cols)[0]))
    # a ready (bytes, offsets) pair, tensors in place, numeric columns by a plain cast, and an out buffer with canaries
    plan2 = FieldPlan([fc.categorical_column_with_hash_bucket("s", 97), fc.categorical_column_with_identity("i", 9, default_value=8),
                       fc.categorical_column_with_vocabulary_list("v", ["a", "bb"], default_value=1)],
                      [fc.numeric_column("n")])
    words = ["x" * k for k in range(70)] + ["bb", "a", "b"]
    feats = {"s": words, "i": np.arange(-3, 70), "v": words[::-1], "n": np.arange(73) * 0.5}
    blob, offs = encode_strings(words)
    dev = {"s": (torch.frombuffer(bytearray(blob), dtype=torch.uint8), torch.from_numpy(offs)), "i": torch.arange(-3, 70),
           "v": words[::-1], "n": torch.arange(73) * 0.5}
    ref_ids, ref_x = plan2.transform(feats)
    out = torch.full((75, 5), -7, dtype=torch.int32)
    ids, x = plan2.device_transform("cpu").transform(dev, out=out)
    assert torch.equal(ids, torch.from_numpy(ref_ids)) and torch.equal(x, torch.from_numpy(ref_x))
    assert ids.data_ptr() == out.data_ptr() and bool((out[73:] == -7).all()) and bool((out[:, 3:] == -7).all())


def test_value_error_texts_and_the_status_contract():
    plan = FieldPlan([fc.categorical_column_with_vocabulary_list("g", ["a", "bb", "ccc"]),
                      fc.categorical_column_with_identity("i", 5), fc.categorical_column_with_identity("j", 5, default_value=9)])
    dt = plan.device_transform("cpu")
    ok = {"g": ["a", "bb", "a", "ccc"], "i": [1, 2, 3, 4], "j": [0, 1, 2, 3]}
    for bad in (dict(ok, g=["a", "zz", "bb", "y"]), dict(ok, i=[1, 2, 7, -4]), dict(ok, j=[0, 1, 2, 5])):
        with pytest.raises(ValueError) as host:
            plan.transform(bad)
        with pytest.raises(ValueError) as device:
            dt.transform(bad)
        assert str(device.value) == str(host.value)
        ids, x, status = dt.transform(bad, check=False)          # nothing raised: the caller looks when it uses the batch
        with pytest.raises(ValueError) as later:
            status.raise_if_bad()
        assert str(later.value) == str(host.value)
        assert bool((ids >= 0).all()) and bool((ids < torch.tensor(plan.vocab_sizes)).all())
    ids, x, status = dt.transform(dict(ok, g=["q", "a", "r", "bb"], i=[1, 9, 9, 1]), check=False)
    assert status.bad() == [(0, 2, 0), (1, 2, 1)] and ids[:, 0].tolist() == [0, 0, 0, 1] and ids[:, 1].tolist() == [1, 0, 0, 1]
    assert dt.transform(ok, check=False)[2].bad() == []
    # reversed offsets: a bad value, never an id
    p2 = FieldPlan([fc.categorical_column_with_hash_bucket("s", 11)])
    pair = (np.frombuffer(b"abcdef", np.uint8), np.array([0, 4, 2, 6], np.int64))
    ids, _, status = p2.device_transform("cpu").transform({"s": pair}, check=False)
    assert status.bad() == [(0, 1, 1)] and ids[1, 0] == 0
    with pytest.raises(ValueError, match="column 's': offsets not monotone at 1"):
        status.raise_if_bad()
    with pytest.raises(ValueError, match="device_transform must be 'off' or 'on'"):
        plan.set_device_mode("auto")


def test_device_transform_on_trains_to_the_same_losses_on_a_cpu_device(tmp_path, monkeypatch, capsys):
    from mi355x_rec import engine
    from tests.cpu_kernels import NumpyKernels
    monkeypatch.setattr(engine, "HipKernels", NumpyKernels)
    fixed = lambda path, mode="train", batch_size=32, seed=None: ml_100k.get_input_fn(path, mode, batch_size=batch_size, seed=5)
    monkeypatch.setattr(_cli, "get_input_fn", fixed)
    opt = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")
    logs, finals = [], []
    for flag in ("off", "on"):
        argv = ["--synthetic", "400", "--job-dir", str(tmp_path / flag), "--train-steps", "20", "--batch-size", "16", "--device", "cpu",
                "--hidden-units", "8", "--device-transform", flag]
        est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(argv))
        assert est.params["_store"]["plan"].device_mode == flag
        finals.append(est._engine().export_numpy())
        logs.append([l for l in capsys.readouterr().out.splitlines() if "loss" in l.lower() and "global_step/sec" not in l])
    assert logs[0] and logs[0] == logs[1]
    a, b = finals
    assert all(np.array_equal(u, v) for u, v in zip(a["emb"] + a["lin_w"], b["emb"] + b["lin_w"]))


def test_the_parsers_new_flag_and_its_default():
    for model, extra in (("deep_fm", ("hidden_units",)), ("linear", ()), ("deep", ("hidden_units",)), ("linear_deep", ("hidden_units",))):
        p = _cli.make_parser(model, extra)
        assert p.parse_args([]).device_transform == "off" and p.parse_args(["--device-transform", "on"]).device_transform == "on"
        with pytest.raises(SystemExit):
            p.parse_args(["--device-transform", "auto"])
    a = predict.make_parser().parse_args(["--job-dir", "j", "--input", "i"])
    assert a.device_transform == "off"
    assert predict.make_parser().parse_args(["--job-dir", "j", "--input", "i", "--device-transform", "on"]).device_transform == "on"
    assert recommend.parse_args(["--model", "deep_fm"]).device_transform == "off"
    assert recommend.parse_args(["--model", "linear", "--device-transform", "on"]).device_transform == "on"
    assert sweep.make_parser().parse_args([]).device_transform == "off"
    assert sweep.make_parser().parse_args(["--device-transform", "on"]).device_transform == "on"


def test_refused_columns_with_bad_values_never_store_an_id_outside_the_range():
    """two columns that stay on the host transform, both with bad values in one batch: every stored id is a row of its
    column, with and without check, and the error is the host's — the first bad column in field order, device or host"""
    cols = [fc.categorical_column_with_identity("a", 4, default_value=9),                 # device column, field 0
            fc.categorical_column_with_vocabulary_list("b", [1, 2, 3]),                   # refused (not strings): default -1
            fc.categorical_column_with_vocabulary_list("c", ["x", "y", "x"]),             # refused (duplicates): default -1
            fc.categorical_column_with_vocabulary_list("d", [5, 6], default_value=7)]     # refused: default 7 >= 2
    plan = FieldPlan(cols)
    dt = plan.device_transform("cpu")
    assert [f for f, _, _ in dt.refused] == [1, 2, 3]
    nb = torch.tensor(plan.vocab_sizes)
    bad_host = {"a": [0, 1, 2, 3], "b": [1, 8, 2, 9], "c": ["x", "q", "y", "r"], "d": [5, 6, 0, 5]}
    ids, x, status = dt.transform(bad_host, check=False)
    assert bool((ids >= 0).all()) and bool((ids < nb).all())
    assert ids[:, 1].tolist() == [0, 0, 1, 0] and ids[:, 2].tolist() == [2, 0, 1, 0] and ids[:, 3].tolist() == [0, 1, 0, 0]
    assert sorted(status.host_errors) == [1, 2, 3]
    for feats in (bad_host, dict(bad_host, a=[0, 7, 2, 3]), dict(bad_host, a=[0, 7, 2, 3], b=[1, 2, 3, 1])):
        with pytest.raises(ValueError) as host:
            plan.transform(feats)
        with pytest.raises(ValueError) as now:
            dt.transform(feats)
        ids, x, status = dt.transform(feats, check=False)
        with pytest.raises(ValueError) as later:
            status.raise_if_bad()
        assert str(now.value) == str(host.value) == str(later.value)
        assert bool((ids >= 0).all()) and bool((ids < nb).all())


def test_host_offsets_past_the_bytes_are_refused_and_plain_tuples_are_columns():
    plan = FieldPlan([fc.categorical_column_with_hash_bucket("s", 11), fc.categorical_column_with_identity("i", 9)])
    dt = plan.device_transform("cpu")
    blob = np.frombuffer(b"abcdef", np.uint8)
    with pytest.raises(ValueError, match="an offset of 100, past the 6 bytes"):
        dt.transform({"s": (blob, np.array([0, 100, 2, 6], np.int64)), "i": [1, 2, 3]})
    with pytest.raises(ValueError, match="an offset of 7, past the 6 bytes"):
        dt.transform({"s": (b"abcdef", torch.tensor([0, 2, 4, 7])), "i": [1, 2, 3]})
    # a Python tuple of two values is a column of B = 2, as for FieldPlan.transform — not a (bytes, offsets) pair
    for feats in ({"s": ("a", "b"), "i": (3, 5)}, {"s": (3, 5), "i": (0, 8)}, {"s": (b"a", b"bc"), "i": (1, 1)}):
        ids, _ = dt.transform(feats)
        assert torch.equal(ids, torch.from_numpy(plan.transform(feats)[0])), feats
