"""-m gpu: the dataset that lives on the device — mi_batch_gather (csrc/batch.hip) through the entry itself, then
DeviceDataset under Estimator.train / evaluate and the trainers' --device-dataset switch.

Everything is copied integers, floats and bytes: held to EQUALITY with numpy fancy indexing and with the plain input
pipeline's runs; there is no tolerance anywhere in this file."""
import types

import numpy as np
import pytest
import torch

from mi355x_rec import dataset
from mi355x_rec.dataset import DeviceDataset
from mi355x_rec.engine import DeepFM, HipKernels
from mi355x_rec.estimator import Estimator, RunConfig
from mi355x_rec.feature_column import FieldPlan
from tests.util import _run_module, dev
from trainers import deep_fm, ml_100k

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
GUARD = 67                        # elements of guard band on either side of every output
ID_GUARD, X_GUARD, Y_GUARD = -7, -7.5, 0xA5


@pytest.fixture(scope="module")
def k():
    return HipKernels()


def _banded(n, fill, dtype):
    """a device buffer of GUARD + n + GUARD elements of `fill`, and its middle"""
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _gather(k, res, order, B, F, n_num, labels):
    """one launch into banded outputs: (ids, x, y, status) as numpy, and the whole buffers (bands included) as tensors"""
    ids_all, ld_ids, x_all, ld_x, y_all, N = res
    ids_buf, ids = _banded(B * F, ID_GUARD, torch.int32)
    x_buf, x = _banded(B * n_num, X_GUARD, torch.float32)
    y_buf, y = _banded(B, Y_GUARD, torch.uint8)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    k.mi_batch_gather(ids_all, ld_ids, x_all if n_num else None, ld_x, y_all if labels else None, N, order, B, F, n_num, ids,
                      x if n_num else None, y if labels else None, status)
    bufs = (ids_buf, x_buf, y_buf)
    for buf, fill in zip(bufs, (ID_GUARD, X_GUARD, Y_GUARD)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())          # nothing outside the outputs
    return (ids.cpu().numpy().reshape(B, F), x.cpu().numpy().reshape(B, n_num), y.cpu().numpy(), status.cpu().numpy()), bufs


@pytest.mark.parametrize("F", [1, 26, 27])
def test_batch_gather_equals_numpy_fancy_indexing(k, F):
    rng = np.random.default_rng(F)
    launches = 0
    for ld_ids in (F, F + 3):
        for N in (1, 1000):
            for n_num in (0, 1, 3):
                ld_x = n_num + (ld_ids - F)
                ids_np = rng.integers(0, 2 ** 31 - 1, (N, ld_ids)).astype(np.int32)
                x_np = rng.standard_normal((N, max(ld_x, 1))).astype(np.float32)
                y_np = rng.integers(0, 2, N).astype(np.uint8)
                res = (dev(ids_np), ld_ids, dev(x_np), ld_x, dev(y_np), N)
                for B in (1, 63, 64, 65, 4097):
                    o = rng.integers(0, N, B).astype(np.int32)
                    o[0], o[-1] = N - 1, 0                                    # the last and the first row, in this order
                    if B > 4:
                        o[2] = o[1]                                           # a repeated index
                    order = dev(np.concatenate([np.full(3, -99, np.int32), o]))[3:]      # the pointer offset by an odd count
                    for labels in (True, False):
                        (ids, x, y, status), bufs = _gather(k, res, order, B, F, n_num, labels)
                        assert np.array_equal(ids, ids_np[o][:, :F]), (ld_ids, N, n_num, B)
                        assert np.array_equal(x, x_np[o][:, :n_num]), (ld_ids, N, n_num, B)
                        assert np.array_equal(y, y_np[o] if labels else np.full(B, Y_GUARD, np.uint8)), (ld_ids, N, n_num, B)
                        assert status.tolist() == [0, 0]
                        _, again = _gather(k, res, order, B, F, n_num, labels)
                        assert all(torch.equal(a, b) for a, b in zip(bufs, again))          # equal bits on a second call
                        launches += 2
    assert launches == 2 * 2 * 2 * 3 * 5 * 2


def test_bad_indices_store_zero_rows_and_tell_the_status(k):
    """-1, N and N + 1 only, and the resident arrays inside a larger allocation of sentinels: a missing bound check would
    show the sentinel (it would not read foreign memory)"""
    rng = np.random.default_rng(3)
    N, F, n_num, B, pad = 50, 26, 3, 130, 2
    ids_big = torch.full((N + 2 * pad, F), 12345, dtype=torch.int32, device="cuda")
    x_big = torch.full((N + 2 * pad, n_num), 123.5, dtype=torch.float32, device="cuda")
    y_big = torch.full((N + 2 * pad,), 77, dtype=torch.uint8, device="cuda")
    ids_np = rng.integers(1, 1000, (N, F)).astype(np.int32)
    x_np = (rng.standard_normal((N, n_num)) + 3).astype(np.float32)
    y_np = rng.integers(0, 2, N).astype(np.uint8)
    ids_big[pad:pad + N], x_big[pad:pad + N], y_big[pad:pad + N] = dev(ids_np), dev(x_np), dev(y_np)
    res = (ids_big[pad:pad + N], F, x_big[pad:pad + N], n_num, y_big[pad:pad + N], N)
    o = rng.integers(0, N, B).astype(np.int32)
    bad = {70: -1, 5: N, 129: N + 1, 64: -1, 63: N}                         # in several tiles, on both sides of a tile's edge
    for b, v in bad.items():
        o[b] = v
    (ids, x, y, status), _ = _gather(k, res, dev(o), B, F, n_num, True)
    ok = np.array([b not in bad for b in range(B)])
    safe = np.where(ok, o, 0)
    assert np.array_equal(ids, np.where(ok[:, None], ids_np[safe], 0))
    assert np.array_equal(x, np.where(ok[:, None], x_np[safe], np.float32(0))) and not np.signbit(x[~ok]).any()
    assert np.array_equal(y, np.where(ok, y_np[safe], 0))
    assert status[0] == len(bad) and INT32_MAX - status[1] == 5
    # through the dataset: a ValueError that names the first bad position
    cols, n = ml_100k.synthetic_columns(100, 1)
    label = cols.pop("rating") >= 5
    eng = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), k=HipKernels(), shard=None)
    ds = DeviceDataset(cols, label, n).bind(FieldPlan(ml_100k.get_feature_columns()["linear"]), eng)
    (ids, _, y), st = ds.gather([(dataset._Pass(np.array([3, 100, 5, -1, 99], np.int64)), 0, 5)], "batch")
    assert ids[1].tolist() == [0] * 26 and int(y[3]) == 0 and torch.equal(ids[4], ds.ids_all[99])
    with pytest.raises(ValueError, match="2 of the batch's indices name no resident row; the first is at position 1"):
        st.raise_if_bad()


def test_bind_leaves_the_host_transforms_ids_on_the_device_in_both_modes_and_in_chunks(monkeypatch):
    cols, n = ml_100k.synthetic_columns(1000, 4)
    label = cols.pop("rating") >= 5
    eng = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), k=HipKernels(), shard=None)
    want = FieldPlan(ml_100k.get_feature_columns()["linear"]).transform(cols)[0]
    for mode, chunk in (("off", None), ("on", None), ("on", 300)):
        plan = FieldPlan(ml_100k.get_feature_columns()["linear"])
        plan.set_device_mode(mode)
        if chunk:
            monkeypatch.setattr(DeviceDataset, "_chunk_rows", lambda self, room: chunk)
        ds = DeviceDataset(cols, label, n).bind(plan, eng)
        assert ds.ids_all.dtype == torch.int32 and np.array_equal(ds.ids_all.cpu().numpy(), want) and ds.x_all is None
        assert np.array_equal(ds.y_all.cpu().numpy(), label.astype(np.uint8))
    free = torch.cuda.mem_get_info(eng.device)[0]
    monkeypatch.setattr(dataset, "_free_bytes", lambda device: 1000)
    with pytest.raises(ValueError, match="the dataset needs 105000 bytes"):
        DeviceDataset(cols, label, n).bind(plan, eng)
    assert free > 105000


# ---- under the Estimator ------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[key], b[key]) for key in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


def _train(tmp_path, tag, n, B, steps, on, **params):
    """Estimator.train over n synthetic examples: (the loss of every step, the engine's state at the end, the estimator)"""
    losses = []

    def model_fn(features, labels, mode, p):
        spec = deep_fm.model_fn(features, labels, mode, p)
        if mode == "train":
            losses.append(torch.as_tensor(spec.loss).detach().clone())
        return spec
    p = {"categorical_columns": ml_100k.get_feature_columns(8)["linear"], "embedding_size": 8, "hidden_units": [16, 16],
         "dropout": 0.1, "device_dataset": "on" if on else "off"}
    p.update(params)
    est = Estimator(model_fn, model_dir=str(tmp_path / tag), config=RunConfig(device="cuda"), params=p)
    est.train(ml_100k.get_input_fn("synthetic:%d:1" % n, batch_size=B, seed=5, device_dataset=on), steps=steps)
    assert est.global_step == steps and len(losses) == steps
    return torch.stack([l.reshape(()) for l in losses]).cpu(), est._engine().state_dict(), est


def test_training_with_lookahead_is_bit_equal_and_the_engine_sees_announced_batches(tmp_path, monkeypatch):
    """B = 4,096 on n = 10,000: two batches a pass and `pending` over every boundary; the next batch's ids are formed a step
    early and announced to the engine"""
    taken = []
    orig = DeepFM._take_presorted
    monkeypatch.setattr(DeepFM, "_take_presorted", lambda self, ids: (lambda ps: (taken.append(ps is not None), ps)[1])(orig(self, ids)))
    runs = []
    for on in (False, True):
        taken.clear()
        losses, state, _ = _train(tmp_path, "la%d" % on, 10000, 4096, 8, on)
        runs.append((losses, state, sum(taken)))
    (l0, s0, hits0), (l1, s1, hits1) = runs
    print("announced batches taken: plain %d, dataset %d" % (hits0, hits1))
    assert hits1 >= 4 and hits0 >= 4, (hits0, hits1)
    assert torch.equal(l0, l1), (l0, l1)
    assert _same(s0, s1)


@pytest.mark.parametrize("params", [{"hip_graph": "auto"}, {"fused_step": "on"}], ids=["hip_graph_auto", "fused_step_on"])
def test_training_small_batches_is_bit_equal(tmp_path, params):
    """B = 32 on n = 1,000 for 70 steps: two groups of 64 batches, each over two pass boundaries"""
    (l0, s0, _), (l1, s1, est) = (_train(tmp_path, "g%d" % on, 1000, 32, 70, on, **params) for on in (False, True))
    assert torch.equal(l0, l1), (l0, l1)
    assert _same(s0, s1)
    assert est._engine().step == 70


def test_evaluation_is_equal_and_reads_the_test_file_once(tmp_path, monkeypatch):
    reads = []
    orig = ml_100k._read_csv
    monkeypatch.setattr(ml_100k, "_read_csv", lambda path: (reads.append(path), orig(path))[1])
    _, _, est = _train(tmp_path, "ev", 1000, 32, 20, False, exact_auc=True, gauc_by="user_id")
    reads.clear()
    plain = ml_100k.get_input_fn("synthetic:1000:2", "eval", batch_size=64)
    ondev = ml_100k.get_input_fn("synthetic:1000:2", "eval", batch_size=64, device_dataset=True)
    want = [est.evaluate(plain) for _ in range(2)]
    assert reads == ["synthetic:1000:2"] * 2
    reads.clear()
    got = [est.evaluate(ondev) for _ in range(2)]
    assert reads == ["synthetic:1000:2"] and ondev.dataset().binds == 1          # read and transformed once for both
    assert want[0] == want[1] == got[0] == got[1], (want[0], got[0])
    assert {"auc", "auc_exact", "auc_exact_pairs", "gauc", "gauc_groups", "average_loss"} <= set(got[0])
    first = next(est.predict(ondev))
    assert first["probabilities"].shape == (2,)


def test_the_cli_runs_with_the_switch_on(tmp_path):
    r = _run_module("trainers.deep_fm", ["--synthetic", "2000", "--device-dataset", "on", "--train-steps", "40",
                                         "--job-dir", str(tmp_path / "job")])
    assert "Saving dict for global step 40" in r.stdout and "auc = " in r.stdout and "average_loss = " in r.stdout
