"""GPU: the categorical id transforms on the device — mi_ids_transform and mi_fingerprint64_device (csrc/ids.hip) through
the bound entries, DeviceTransform, and the switches of the trainers and predictors.

Integer work held to EQUALITY with the host definitions (mi_fingerprint64, mi_hash_bucket_*, mi_bucketize_f32,
VocabularyListColumn / IdentityColumn / FieldPlan.transform): there is no tolerance anywhere in this file."""
import os
import re

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, feature_column as fc
from mi355x_rec.device_transform import vocabulary_table
from mi355x_rec.engine import HipKernels
from mi355x_rec.feature_column import FieldPlan, encode_strings
from mi355x_rec.predictor import EnsemblePredictor, Predictor
from tests.util import dev
from trainers import ml_100k, recommend as rec_cli

pytestmark = pytest.mark.gpu

BUCKETS = (1, 2, 3, 1000, 10 ** 6 + 3, 2 ** 31 - 1)
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def k():
    return HipKernels()


def _blob(strings):
    offs = np.zeros(len(strings) + 1, np.int64)
    np.cumsum([len(s) for s in strings], out=offs[1:])
    raw = b"".join(strings)
    return np.frombuffer(raw if raw else b"\0", np.uint8).copy(), offs


def _column(kind, values, num_buckets, offsets=None, table=None, table_host=None, n_table=0, num_oov=0, default=-1):
    c = _lib.IdsColumn()
    c.kind, c.num_buckets, c.n_table, c.num_oov, c.default_value = kind, num_buckets, n_table, num_oov, default
    _lib.set_ptrs(c, values=values, offsets=offsets, table=table, table_host=table_host)
    return c


def _run(k, columns, B, ld=None, rows=None):
    """ids [rows, ld] (canaries -7 outside [B, F]) and status [F, 2] of one mi_ids_transform launch, as numpy"""
    F = len(columns)
    ld, rows = ld or F, rows or B
    arr = (_lib.IdsColumn * F)(*columns)
    ids = torch.full((rows, ld), -7, dtype=torch.int32, device="cuda")
    status = torch.zeros(F, 2, dtype=torch.int32, device="cuda")
    k.mi_ids_transform(arr, F, B, ids, ld, status)
    return ids.cpu().numpy(), status.cpu().numpy()


def _random_strings(rng, lengths):
    out = []
    for n in lengths:
        s = rng.integers(0, 256, n, dtype=np.uint8)
        if n > 2:
            s[rng.integers(0, n)] = 0                      # a NUL inside
            s[rng.integers(0, n)] = 0x80 + int(rng.integers(0, 128))
        out.append(s.tobytes())
    return out


# every length 0 .. 200, then empty strings next to each other, then a few long ones (several rounds of the 64-byte loop)
LENGTHS = list(range(201)) + [0, 0, 0, 5, 0, 0] + [255, 256, 257, 1000] + [(7 * i) % 131 for i in range(50)]
assert len(LENGTHS) >= 257


@pytest.fixture(scope="module")
def strings():
    return _random_strings(np.random.default_rng(11), LENGTHS)


def test_fingerprints_equal_the_host_fingerprint(lib, k, strings):
    want = np.array([lib.mi_fingerprint64(s, len(s)) for s in strings], np.uint64)
    for n in (1, 63, 64, 65, 257, len(strings)):
        blob, offs = _blob(strings[:n])
        assert len(offs) == n + 1
        out = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        out[n] = -7
        k.mi_fingerprint64_device(dev(blob), dev(offs), n, out)
        got = out.cpu().numpy()
        assert got[n] == -7 and np.array_equal(got[:n].view(np.uint64), want[:n]), n
    # the strings from the far end too: other alignments of every length
    blob, offs = _blob(strings[::-1])
    out = torch.zeros(len(strings), dtype=torch.int64, device="cuda")
    k.mi_fingerprint64_device(dev(blob), dev(offs), len(strings), out)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want[::-1])


def _integer_values():
    v = [0, -(2 ** 63), 2 ** 63 - 1, -(2 ** 31), 2 ** 31 - 1]
    for e in range(19):
        for d in (-1, 0, 1):
            v += [10 ** e + d, -(10 ** e + d)]
    rng = np.random.default_rng(5)
    raw = rng.integers(-(2 ** 63), 2 ** 63 - 1, 4096, dtype=np.int64) >> rng.integers(0, 64, 4096)
    return np.concatenate([np.array(v, np.int64), raw])


def test_integer_hash_bucket_equals_the_host_entry(lib, k):
    v64 = _integer_values()
    v32 = np.concatenate([v64[(v64 >= -(2 ** 31)) & (v64 <= INT32_MAX)], np.array([-(2 ** 31), INT32_MAX])]).astype(np.int32)
    for vals, kind in ((v64, _lib.IDS_HASH_I64), (v32, _lib.IDS_HASH_I32)):
        B = len(vals)
        d = dev(vals)
        got, status = _run(k, [_column(kind, d, nb) for nb in BUCKETS], B)
        a = np.ascontiguousarray(vals, np.int64)
        for f, nb in enumerate(BUCKETS):
            want = np.empty(B, np.int32)
            _lib.check(lib.mi_hash_bucket_i64(a.ctypes.data, B, nb, want.ctypes.data), "mi_hash_bucket_i64")
            assert np.array_equal(got[:, f], want), (kind, nb)
        assert not status.any()


def test_sixty_four_columns_in_one_launch(lib, k):
    """F = MI_IDS_MAX_COLUMNS: the whole column table in the kernel's arguments, every column with its own values, kind and
    bucket count, the last one read as carefully as the first"""
    F, B = _lib.IDS_MAX_COLUMNS, 300
    rng = np.random.default_rng(64)
    vals = [rng.integers(-(10 ** 12), 10 ** 12, B, dtype=np.int64) if f % 2 == 0 else rng.integers(-(2 ** 31), 2 ** 31 - 1, B).astype(np.int32)
            for f in range(F)]
    nbs = [int(rng.integers(1, 2 ** 31 - 1)) if f % 3 else f + 1 for f in range(F)]
    d = [dev(v) for v in vals]
    cols = [_column(_lib.IDS_HASH_I64 if f % 2 == 0 else _lib.IDS_HASH_I32, d[f], nbs[f]) for f in range(F)]
    got, status = _run(k, cols, B, ld=F + 1, rows=B + 1)
    for f in range(F):
        a = np.ascontiguousarray(vals[f], np.int64)
        want = np.empty(B, np.int32)
        _lib.check(lib.mi_hash_bucket_i64(a.ctypes.data, B, nbs[f], want.ctypes.data), "mi_hash_bucket_i64")
        assert np.array_equal(got[:B, f], want), f
    assert not status.any() and (got[B:] == -7).all() and (got[:, F] == -7).all()


def test_string_hash_bucket_equals_the_host_entry(lib, k, strings):
    blob, offs = _blob(strings)
    B = len(strings)
    b, o = dev(blob), dev(offs)
    got, status = _run(k, [_column(_lib.IDS_HASH_BYTES, b, nb, offsets=o) for nb in BUCKETS], B)
    for f, nb in enumerate(BUCKETS):
        want = np.empty(B, np.int32)
        _lib.check(lib.mi_hash_bucket_bytes(blob.ctypes.data, offs.ctypes.data, B, nb, want.ctypes.data), "mi_hash_bucket_bytes")
        assert np.array_equal(got[:, f], want), nb
    assert not status.any()


@pytest.mark.parametrize("nb", [1, 33])
def test_bucketize_equals_the_host_entry(lib, k, nb):
    rng = np.random.default_rng(nb)
    bd = np.sort(rng.standard_normal(nb).astype(np.float32) * 50)
    assert np.all(bd[1:] > bd[:-1])
    x = np.concatenate([bd, np.nextafter(bd, np.float32(-np.inf)), np.nextafter(bd, np.float32(np.inf)),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32), rng.standard_normal(300).astype(np.float32) * 60])
    x = x.astype(np.float32)
    B = len(x)
    x_d, bd_d = dev(x), dev(bd)                              # (named: the descriptor holds addresses, not references)
    got, status = _run(k, [_column(_lib.IDS_BUCKETIZE_F32, x_d, nb + 1, table=bd_d, table_host=bd, n_table=nb)], B)
    want = np.empty(B, np.int32)
    _lib.check(lib.mi_bucketize_f32(x.ctypes.data, B, bd.ctypes.data, nb, want.ctypes.data), "mi_bucketize_f32")
    assert np.array_equal(got[:, 0], want) and not status.any()
    assert got[np.isnan(x), 0].tolist() == [0]


VOCAB = ["F", "M", "other", "a-much-longer-entry-of-the-vocabulary", "éé", "oth", "x" * 70, "12345678", "123456789"]


def _vocab_values():
    vals = list(VOCAB) + [v[:-1] for v in VOCAB] + [v + "!" for v in VOCAB] + ["", "f", "m", "x" * 69, "x" * 71, "x" * 64]
    rng = np.random.default_rng(2)
    return [vals[i] for i in rng.permutation(len(vals))] + vals


@pytest.mark.parametrize("num_oov,default", [(1, -1), (3, -1), (0, 2)])
def test_vocabulary_equals_the_host_column(k, num_oov, default):
    col = fc.categorical_column_with_vocabulary_list("v", VOCAB, default_value=default, num_oov_buckets=num_oov)
    vals = _vocab_values()
    want = col.transform({"v": vals})
    blob, offs = encode_strings(vals)
    b_d, o_d, table = dev(np.frombuffer(blob, np.uint8).copy()), dev(offs), dev(vocabulary_table(VOCAB))
    got, status = _run(k, [_column(_lib.IDS_VOCAB_BYTES, b_d, col.num_buckets, offsets=o_d, table=table, n_table=len(VOCAB),
                                   num_oov=num_oov, default=default)], len(vals))
    assert np.array_equal(got[:, 0], want) and not status.any()
    assert set(want[:len(VOCAB) * 3 + 6]) >= set(range(len(VOCAB)))            # (members were looked up, not only misses)


def test_vocabulary_default_minus_one_is_counted_and_stores_row_zero(k):
    col = fc.categorical_column_with_vocabulary_list("v", VOCAB)
    vals = ["M", "M", "F"] + _vocab_values()
    host = col.transform({"v": vals})
    blob, offs = encode_strings(vals)
    b_d, o_d, table = dev(np.frombuffer(blob, np.uint8).copy()), dev(offs), dev(vocabulary_table(VOCAB))
    got, status = _run(k, [_column(_lib.IDS_VOCAB_BYTES, b_d, col.num_buckets, offsets=o_d, table=table, n_table=len(VOCAB))], len(vals))
    miss = host < 0
    assert miss.any() and np.array_equal(got[:, 0], np.where(miss, 0, host))
    assert status[0, 0] == miss.sum() and INT32_MAX - status[0, 1] == np.flatnonzero(miss)[0] > 2


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_identity_equals_the_host_column(k, dtype):
    n = 11
    vals = np.array([0, 1, n - 1, n, n + 1, -1, -5, 10 ** 6, 3, INT32_MAX, -(2 ** 31)] + ([2 ** 40, -(2 ** 40)] if dtype == np.int64 else []), dtype)
    kind = _lib.IDS_IDENTITY_I64 if dtype == np.int64 else _lib.IDS_IDENTITY_I32
    d = dev(vals)
    got, status = _run(k, [_column(kind, d, n, default=4), _column(kind, d, n)], len(vals))
    want = fc.categorical_column_with_identity("i", n, default_value=4).transform({"i": vals})
    assert np.array_equal(got[:, 0], want) and status[0].tolist() == [0, 0]
    bad = (vals < 0) | (vals >= n)
    assert np.array_equal(got[:, 1], np.where(bad, 0, vals)) and status[1, 0] == bad.sum()
    assert INT32_MAX - status[1, 1] == np.flatnonzero(bad)[0] == 3


@pytest.fixture(scope="module")
def ml100k():
    cols, _ = ml_100k.synthetic_columns(257, seed=3)
    plan = FieldPlan(ml_100k.get_feature_columns()["linear"])
    return plan, cols, torch.from_numpy(plan.transform(cols)[0])


def test_the_whole_ml_100k_plan_from_numpy_columns_and_from_device_tensors(ml100k, k):
    plan, cols, want = ml100k
    dt = plan.device_transform("cuda", k)
    assert dt.refused == [] and dt.runs == [[0, 26]]
    ids, x = dt.transform(cols)
    assert x is None and ids.dtype == torch.int32 and ids.is_cuda and torch.equal(ids.cpu(), want)
    on_dev = {}
    for key, v in cols.items():
        if v.dtype.kind in "iu":
            on_dev[key] = torch.from_numpy(v).cuda()
        else:
            blob, offs = encode_strings(v)
            on_dev[key] = (torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(), torch.from_numpy(offs).cuda())
    F = 26
    out = torch.full((257 + 4, F + 3), -7, dtype=torch.int32, device="cuda")
    ids2, _ = dt.transform(on_dev, out=out)
    host = out.cpu()
    assert ids2.data_ptr() == out.data_ptr() and torch.equal(host[:257, :F], want)
    assert bool((host[257:] == -7).all()) and bool((host[:, F:] == -7).all())
    again = torch.full_like(out, -7)
    dt.transform(on_dev, out=again)
    assert torch.equal(again.cpu(), host)                       # the same bits on a second call


def test_garbage_never_stores_an_id_outside_the_fields_range(k):
    rng = np.random.default_rng(9)
    B = 1000
    junk = rng.integers(-(2 ** 63), 2 ** 63 - 1, B, dtype=np.int64)
    junk[::7] = rng.integers(0, 50, len(junk[::7]))
    blob = rng.integers(0, 256, 4096, dtype=np.uint8)
    offs = np.sort(rng.integers(0, 4096, B + 1)).astype(np.int64)[::-1].copy()          # reversed: descending
    offs[500:520] = offs[500]                                                            # (a stretch of empty strings is fine)
    table = dev(vocabulary_table(VOCAB))
    d, b, o = dev(junk), dev(blob), dev(offs)
    cols = [_column(_lib.IDS_IDENTITY_I64, d, 50), _column(_lib.IDS_IDENTITY_I64, d, 50, default=77),
            _column(_lib.IDS_HASH_BYTES, b, 13, offsets=o), _column(_lib.IDS_VOCAB_BYTES, b, len(VOCAB) + 2, offsets=o, table=table,
                                                                    n_table=len(VOCAB), num_oov=2)]
    got, status = _run(k, cols, B, ld=6, rows=B + 2)
    nb = np.array([50, 50, 13, len(VOCAB) + 2])
    assert (got[:B, :4] >= 0).all() and (got[:B, :4] < nb).all() and (got[B:] == -7).all() and (got[:, 4:] == -7).all()
    bad_id = (junk < 0) | (junk >= 50)
    bad_off = offs[1:] < offs[:-1]
    assert status[:, 0].tolist() == [bad_id.sum(), bad_id.sum(), bad_off.sum(), bad_off.sum()]
    assert (INT32_MAX - status[:, 1]).tolist() == [np.flatnonzero(bad_id)[0]] * 2 + [np.flatnonzero(bad_off)[0]] * 2
    assert np.array_equal(got[:B, 0], np.where(bad_id, 0, junk)) and (got[:B, 2][bad_off] == 0).all()
    again, status2 = _run(k, cols, B, ld=6, rows=B + 2)
    assert np.array_equal(again, got) and np.array_equal(status2, status)


def test_refusals_leave_ids_and_status_untouched(lib):
    B = 8
    vals = torch.arange(B, dtype=torch.int64, device="cuda")
    fl = torch.arange(B, dtype=torch.float32, device="cuda")
    offs = torch.arange(B + 1, dtype=torch.int64, device="cuda")
    raw = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    status = torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    bd_ok, bd_bad = np.array([1.0, 2.0, 3.0], np.float32), np.array([1.0, 3.0, 3.0], np.float32)
    bd_dev = dev(bd_ok)
    table = dev(vocabulary_table(VOCAB))
    good = _column(_lib.IDS_HASH_I64, vals, 10)
    stream = _lib.cur_stream()

    def refused(cols, F=None, B_=B, ids_=ids, status_=status, ld=2, text=""):
        arr = (_lib.IdsColumn * max(len(cols), 1))(*cols) if cols is not None else None
        rc = lib.mi_ids_transform(arr, len(cols) if F is None else F, B_, None if ids_ is None else ids_.data_ptr(), ld,
                                  None if status_ is None else status_.data_ptr(), stream)
        msg = lib.mi_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg, text)

    refused(None, F=1, text="null")
    refused([good], ids_=None, text="null")
    refused([good], status_=None, text="null")
    refused([good], F=0, text="F=0")
    refused([good] * 65, text="F=65")
    refused([good], B_=0, text="B=0")
    refused([good], B_=2 ** 31, text="B=")
    refused([good, good], ld=1, text="ld=1")
    refused([good, _column(7, vals, 10)], text="column 1: unknown kind 7")
    refused([good, _column(-1, vals, 10)], text="column 1: unknown kind")
    refused([_column(_lib.IDS_HASH_I64, None, 10), good], text="column 0: null values")
    refused([good, _column(_lib.IDS_HASH_BYTES, raw, 10)], text="column 1: null offsets")
    refused([good, _column(_lib.IDS_HASH_I64, vals, 0)], text="column 1: num_buckets=0")
    refused([good, _column(_lib.IDS_IDENTITY_I32, vals, -3)], text="column 1: num_buckets=-3")
    refused([good, _column(_lib.IDS_BUCKETIZE_F32, fl, 4, table=bd_dev, table_host=bd_bad, n_table=3)],
            text="column 1: boundaries must be strictly increasing")
    refused([good, _column(_lib.IDS_BUCKETIZE_F32, fl, 4, table=bd_dev, n_table=3)], text="column 1: null boundaries")
    refused([good, _column(_lib.IDS_BUCKETIZE_F32, fl, 3, table=bd_dev, table_host=bd_ok, n_table=3)], text="column 1: 3 boundaries")
    refused([good, _column(_lib.IDS_VOCAB_BYTES, raw, 20, offsets=offs, n_table=len(VOCAB))], text="column 1: no vocabulary table")
    refused([good, _column(_lib.IDS_VOCAB_BYTES, raw, len(VOCAB), offsets=offs, table=table, n_table=len(VOCAB), num_oov=1)],
            text="column 1: %d entries + 1 oov buckets" % len(VOCAB))
    assert lib.mi_fingerprint64_device(raw.data_ptr(), offs.data_ptr(), 0, ids.data_ptr(), stream) == -1
    assert lib.mi_fingerprint64_device(raw.data_ptr(), None, 4, ids.data_ptr(), stream) == -1
    assert lib.mi_fingerprint64_device(raw.data_ptr(), offs.data_ptr(), 4, None, stream) == -1
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((status == -7).all())


def test_check_false_leaves_the_host_free_and_raises_the_same_message_later(k):
    plan = FieldPlan([fc.categorical_column_with_vocabulary_list("g", ["a", "bb", "ccc"]),
                      fc.categorical_column_with_identity("i", 5)])
    dt = plan.device_transform("cuda", k)
    ok = {"g": ["a", "bb", "a", "ccc"], "i": [1, 2, 3, 4]}
    for bad in (dict(ok, g=["a", "zz", "bb", "y"]), dict(ok, i=torch.tensor([1, 2, 7, -4], device="cuda"))):
        host_feats = {key: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for key, v in bad.items()}
        with pytest.raises(ValueError) as host:
            plan.transform(host_feats)
        with pytest.raises(ValueError) as now:
            dt.transform(bad)
        ids, x, status = dt.transform(bad, check=False)                  # returns without looking at the status
        assert status.event is not None
        more, _, fine = dt.transform(ok, check=False)                    # ... and the host queues the next batch
        with pytest.raises(ValueError) as later:
            status.raise_if_bad()
        assert str(now.value) == str(host.value) == str(later.value)
        fine.raise_if_bad()
        assert bool((ids.cpu() >= 0).all()) and bool((ids.cpu() < torch.tensor(plan.vocab_sizes)).all())
        assert torch.equal(more.cpu(), torch.from_numpy(plan.transform(ok)[0]))


# ---- end to end: the trainers' flag, the predictors' argument, recommend ------------------------------------------------------
def _loss_lines(text):
    return [re.sub(r" \([0-9.]+ global_step/sec\)", "", l) for l in text.splitlines() if "loss" in l]


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """two deep_fm runs with the flag off (E = 4 and 8: the members of an ensemble) and the first one again with it on; in
    this process, the input pipeline's shuffle seeded alike (a process of its own draws a fresh seed per run)"""
    import contextlib
    import io
    from trainers import _cli, deep_fm
    root = tmp_path_factory.mktemp("device_transform")
    fixed = lambda path, mode="train", batch_size=32, seed=None: ml_100k.get_input_fn(path, mode, batch_size=batch_size, seed=5)
    opt = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_cli, "get_input_fn", fixed)
        for name, E, flag in (("a", "4", "off"), ("b", "8", "off"), ("a_on", "4", "on")):
            job = str(root / name)
            argv = ["--synthetic", "400", "--job-dir", job, "--train-steps", "20", "--embedding-size", E, "--device-transform", flag]
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(argv))
            assert est.params["_store"]["plan"].device_mode == flag
            runs[name] = (job, log.getvalue())
    return runs


def _requests(spec):
    cols, _ = ml_100k._read_csv(spec)
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    return {key: v for key, v in cols.items() if key in recv}


def test_trainer_with_the_flag_on_logs_the_bits_of_offs_losses(jobs):
    (job_off, out_off), (job_on, out_on) = jobs["a"], jobs["a_on"]
    assert _loss_lines(out_off) and _loss_lines(out_off) == _loss_lines(out_on)
    newest = lambda job: Predictor.from_export(os.path.join(job, "export", "exporter")).export_dir
    a = torch.load(os.path.join(newest(job_off), "variables.pt"), weights_only=True, map_location="cpu")
    b = torch.load(os.path.join(newest(job_on), "variables.pt"), weights_only=True, map_location="cpu")
    for key in ("table", "lin_w", "dense"):
        assert torch.equal(a[key], b[key]), key


def test_predictors_give_equal_outputs_on_and_off(jobs):
    dirs = [os.path.join(jobs[n][0], "export", "exporter") for n in ("a", "b")]
    for spec in ("synthetic:70:3", "synthetic:1:4"):
        feats = _requests(spec)
        for mode in ("fused", "layered"):
            off = Predictor.from_export(dirs[0], mode=mode)(feats)
            on = Predictor.from_export(dirs[0], mode=mode, device_transform="on")(feats)
            assert sorted(on) == sorted(off) and all(np.array_equal(on[key], off[key]) for key in off), (spec, mode)
            e_off = EnsemblePredictor.from_exports(dirs, mode=mode, member_mode=mode)(feats, return_members=True)
            e_on = EnsemblePredictor.from_exports(dirs, mode=mode, member_mode=mode, device_transform="on")(feats, return_members=True)
            assert sorted(e_on) == sorted(e_off) and all(np.array_equal(e_on[key], e_off[key]) for key in e_off), (spec, mode)


def test_recommend_gives_equal_indices_and_logits_on_and_off(jobs):
    d = os.path.join(jobs["a"][0], "export", "exporter")
    train, _ = ml_100k._read_csv("synthetic:300:1")
    test, _ = ml_100k._read_csv("synthetic:60:2")
    users, qf, items, cf = rec_cli.tables(train, test)
    off = Predictor.from_export(d).recommend(qf, cf, 5)
    on_p = Predictor.from_export(d, device_transform="on")
    on = on_p.recommend(qf, cf, 5)
    assert np.array_equal(on["indices"], off["indices"]) and np.array_equal(on["logits"], off["logits"])
    targets = rec_cli.positive_targets(users, items, test)
    assert np.array_equal(on_p.rank_targets(qf, cf, targets), Predictor.from_export(d).rank_targets(qf, cf, targets))
