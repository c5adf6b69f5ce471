"""A dataset that lives on the device: ``DeviceDataset`` transforms ALL of its examples once (``bind``), keeps the id
matrix, the numeric features and the labels there, and forms every training batch on the device from the shuffle's index
stream in one launch (``mi_batch_gather``, include/mi355x_rec.h, csrc/batch.hip).  Evaluation and prediction batches are
ordered and contiguous: views of the resident arrays, no launch.

What the plain input pipeline does per batch — fancy-index every raw column, encode the strings, transform the ids, copy
them — happens here once per dataset; a step copies nothing but (once a pass) the pass's index stream.  The id transforms
are stateless, so the batches are those of the plain pipeline bit for bit (tests/test_device_dataset_cpu.py).

``input_fn()`` of a dataset yields ``(DeviceBatch, labels)``: the plan and the engine do not exist when the first batches
are drawn, so a batch is a lazy handle that ``model.run_batch`` materialises (``DeviceBatch.materialise``).  The handle is
also a mapping of the batch's RAW features, fetched from the host columns on demand.  One GPU only."""
import collections.abc

import numpy as np
import torch

from . import _lib

_INT32_MAX = 2 ** 31 - 1
TRAIN = "train"                   # estimator.ModeKeys.TRAIN (the estimator imports this module)


def shuffle_passes(n, batch_size, seed=None):
    """The index streams of tf.data's ``.shuffle(16 * batch_size).repeat().batch(batch_size)`` over n examples, one int64
    array per pass, forever: the pass's shuffled order behind the `pending` examples the previous pass left over (fewer
    than a batch).  Batch b of a pass is stream[b * batch_size : (b + 1) * batch_size]; what is left after the last whole
    batch is the next pass's `pending`.  The plain input_fn (trainers/ml_100k.get_input_fn) and DeviceDataset both draw
    their batches from this generator."""
    rng = np.random.default_rng(seed)
    cap = 16 * batch_size
    pending = np.empty(0, np.int64)
    while True:                                        # .repeat()
        # .shuffle(cap): a buffer of cap elements; every further element i draws a slot j uniformly, the slot's
        # occupant goes out, i takes its place; at the end of the pass the buffer goes out in random order.
        # The draws of a pass come from the generator in one call, the swap chain — element i's successor is the
        # next element that draws i's slot — is followed per SLOT in numpy: out[k] = the occupant of slot j[k]
        # before draw k = the element of the latest earlier draw with the same slot (or the slot's first occupant).
        m = max(n - cap, 0)
        j = rng.integers(cap, size=m) if m else np.empty(0, np.int64)
        order = np.argsort(j, kind="stable")           # draws grouped by slot, in time order inside a group
        js = j[order]
        prev = np.empty(m, np.int64)                   # for every draw: who sits in its slot
        first = np.ones(m, bool)
        first[1:] = js[1:] != js[:-1]
        prev[order] = np.where(first, js, np.concatenate([[0], order[:-1]]) + cap)   # slot's first occupant = element js
        out = prev                                     # (element ids: the first cap elements are 0..cap-1, draw k places element cap + k)
        buf = np.arange(min(n, cap), dtype=np.int64)
        if m:
            last = np.ones(m, bool)
            last[:-1] = js[1:] != js[:-1]
            buf[js[last]] = order[last] + cap          # what sits in a drawn slot after the pass
        rng.shuffle(buf)
        stream = np.concatenate([pending, out, buf])
        yield stream
        pending = stream[len(stream) // batch_size * batch_size:]


def batch_gather(kernels, ids_all, x_all, y_all, order, ids, x, y, status):
    """One mi_batch_gather call on tensors: rows order[0 .. B) of ids_all [N, >= F] (x_all [N, >= n_num] or None, y_all
    [N] or None) into the dense ids [B, F] (x [B, n_num], y [B]); status int32 [2], zeroed by the caller.  The shapes are
    checked here, the values by the entry; `order` is usually a view into a pass's stream."""
    B, F = ids.shape
    N = ids_all.shape[0]
    n_num = 0 if x is None else x.shape[1]
    if (x is None) != (x_all is None) or (y is None) != (y_all is None):
        raise ValueError("batch_gather: x_all / x and y_all / y come in pairs")
    for name, t, dtype in (("ids_all", ids_all, torch.int32), ("ids", ids, torch.int32), ("x_all", x_all, torch.float32),
                           ("x", x, torch.float32), ("y_all", y_all, torch.uint8), ("y", y, torch.uint8),
                           ("order", order, torch.int32), ("status", status, torch.int32)):
        if t is not None and t.dtype != dtype:
            raise ValueError("batch_gather: %s is %s, not %s" % (name, t.dtype, dtype))
    if ids_all.dim() != 2 or ids_all.shape[1] < F or ids_all.stride(1) != 1 or not ids.is_contiguous():
        raise ValueError("batch_gather: ids_all is [N, >= F] with contiguous rows, ids dense [B, F]")
    if x is not None and (x_all.dim() != 2 or x_all.shape[0] != N or x_all.shape[1] < n_num or x_all.stride(1) != 1
                          or tuple(x.shape) != (B, n_num) or not x.is_contiguous()):
        raise ValueError("batch_gather: x_all is [N, >= n_num] with contiguous rows, x dense [B, n_num]")
    if y is not None and (tuple(y_all.shape) != (N,) or tuple(y.shape) != (B,) or not y_all.is_contiguous() or not y.is_contiguous()):
        raise ValueError("batch_gather: y_all is [N], y is [B]")
    if tuple(order.shape) != (B,) or not order.is_contiguous() or status.numel() != 2:
        raise ValueError("batch_gather: order is int32 [B], status int32 [2]")
    ld_ids = ids_all.stride(0) if N > 1 else ids_all.shape[1]
    ld_x = 0 if x is None else (x_all.stride(0) if N > 1 else x_all.shape[1])
    kernels.mi_batch_gather(ids_all, ld_ids, x_all if n_num else None, ld_x, y_all, N, order, B, F, n_num, ids,
                            x if n_num else None, y, status)


def _free_bytes(device):
    """free device memory in bytes, or None where nobody counts it (a CPU device)"""
    if device.type != "cuda":
        return None
    return torch.cuda.mem_get_info(device)[0]


class GatherStatus:
    """The status of one mi_batch_gather call, copied to pinned host memory behind the launch: raise_if_bad() waits for that
    copy alone (nothing queued later) and names the first bad position."""

    def __init__(self, status, event, what):
        self.status, self.event, self.what = status, event, what

    def raise_if_bad(self):
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        count, first = int(self.status[0]), _INT32_MAX - int(self.status[1])
        if count > 0:
            raise ValueError("device_dataset: %d of the %s's indices name no resident row; the first is at position %d" %
                             (count, self.what, first))


class _Pass:
    """One pass's index stream: on the host as the shuffle made it, on the device (int32, copied once) when first used"""

    def __init__(self, stream):
        self.stream = stream
        self.device = None

    def on(self, device):
        if self.device is None:
            self.device = torch.from_numpy(self.stream.astype(np.int32)).to(device)
        return self.device


class DeviceBatch(collections.abc.Mapping):
    """One batch of a DeviceDataset: rows lo..hi of a pass's index stream (training) or of the dataset itself (evaluation,
    prediction: `stream` is None).  As a mapping: the batch's raw features, name -> host values."""

    def __init__(self, dataset, stream, lo, hi):
        self.dataset, self.stream, self.lo, self.hi = dataset, stream, lo, hi

    def rows(self):
        """the examples of the batch, as an index into the dataset's host columns (a slice for an ordered batch)"""
        return slice(self.lo, self.hi) if self.stream is None else self.stream.stream[self.lo:self.hi]

    def __getitem__(self, key):
        return self.dataset.columns[key][self.rows()]

    def __contains__(self, key):
        return key in self.dataset.columns

    def __iter__(self):
        return iter(self.dataset.columns)

    def __len__(self):
        return len(self.dataset.columns)

    def labels(self):
        return self.dataset.labels[self.rows()]

    def materialise(self, plan, engine):
        """((ids, x, y), status) on the engine's device: views for an ordered batch (status None), one mi_batch_gather for
        a shuffled one (status: a GatherStatus, nothing waited for)."""
        ds = self.dataset.bind(plan, engine)
        if self.stream is None:
            return (ds.ids_all[self.lo:self.hi], None if ds.x_all is None else ds.x_all[self.lo:self.hi],
                    ds.y_all[self.lo:self.hi]), None
        return ds.gather([(self.stream, self.lo, self.hi)], "batch")


def materialise_group(handles, plan, engine):
    """A group of consecutive training batches (Estimator._grouped) formed at once: ((ids, x, y), status) of all their rows,
    the batches are row ranges of it in order.  One launch — one more where the group runs over the end of a pass."""
    runs = []
    for h in handles:
        if runs and runs[-1][0] is h.stream and runs[-1][2] == h.lo:
            runs[-1][2] = h.hi
        else:
            runs.append([h.stream, h.lo, h.hi])
    return handles[0].dataset.bind(plan, engine).gather(runs, "group of batches")


class DeviceDataset:
    def __init__(self, columns, labels, n):
        """columns: name -> [n] raw host values (what trainers/ml_100k._read_csv returns, without the label column);
        labels: [n] bool."""
        self.columns, self.n = columns, int(n)
        self.labels = np.asarray(labels).reshape(-1)
        if self.n < 1 or len(self.labels) != self.n:
            raise ValueError("device_dataset: %d examples and %d labels" % (self.n, len(self.labels)))
        self.plan = self.engine = self.ids_all = self.x_all = self.y_all = None
        self.binds = 0

    # -- once: everything to the device ------------------------------------------------------------------------------
    def resident_bytes(self, plan):
        return self.n * (4 * len(plan.categorical) + 4 * len(plan.numeric) + 1)

    def bind(self, plan, engine):
        """Transform all n examples with `plan` and leave ids_all int32 [n, F], x_all float32 [n, n_num] (or None) and
        y_all uint8 [n] on the engine's device.  Runs once: binding again to the same plan and engine does nothing."""
        if self.plan is plan and self.engine is engine:
            return self
        if getattr(engine, "shard", None) is not None:
            raise ValueError("device_dataset: one GPU only — a row-sharded engine (RowShard) takes the plain input pipeline")
        if self.n > _INT32_MAX:
            raise ValueError("device_dataset: %d examples (at most 2^31 - 1)" % self.n)
        dev = engine.device
        F, n_num = len(plan.categorical), len(plan.numeric)
        if not 1 <= F <= _lib.IDS_MAX_COLUMNS:
            raise ValueError("device_dataset: %d categorical columns (1 to %d)" % (F, _lib.IDS_MAX_COLUMNS))
        need, free = self.resident_bytes(plan), _free_bytes(dev)
        if free is not None and need > free:
            raise ValueError("device_dataset: the dataset needs %d bytes on %s (%d examples: ids of %d columns, %d numeric "
                             "features, labels) and %d are free" % (need, dev, self.n, F, n_num, free))
        ids_all = torch.empty(self.n, F, dtype=torch.int32, device=dev)
        x_all = torch.empty(self.n, n_num, dtype=torch.float32, device=dev) if n_num else None
        if plan.device_mode == "on":
            # the raw columns go to the device a chunk at a time (as many rows as fit beside the resident arrays)
            dt = plan.on_device(dev, engine.k)
            rows = self._chunk_rows(None if free is None else free - need)
            try:
                for lo in range(0, self.n, rows):
                    hi = min(self.n, lo + rows)
                    _, x = dt.transform({k: v[lo:hi] for k, v in self.columns.items()}, out=ids_all[lo:hi])
                    if x is not None:
                        x_all[lo:hi] = x
            except ValueError:
                plan.transform(self.columns)        # a bad value: FieldPlan.transform's own error for the whole dataset
                raise
        else:
            ids_np, x_np = plan.transform(self.columns)
            ids_all.copy_(torch.from_numpy(ids_np))
            if x_np is not None:
                x_all.copy_(torch.from_numpy(x_np))
        self.y_all = torch.from_numpy(np.ascontiguousarray(self.labels).astype(np.uint8)).to(dev)
        self.ids_all, self.x_all = ids_all, x_all
        self.plan, self.engine, self.k = plan, engine, engine.k
        self.binds += 1
        return self

    def _chunk_rows(self, room):
        """rows of raw columns to copy at once: what fits into half of `room` bytes (None: everything), at most 2^22"""
        per_row = 0
        for v in self.columns.values():
            v = np.asarray(v)
            if v.dtype.kind in "OUS":               # strings: their bytes (sampled) and an int64 offset
                head = v[:1024]
                per_row += 8 + int(np.mean([len(str(s)) for s in head])) + 1 if len(head) else 8
            else:
                per_row += 8
        rows = 1 << 22
        if room is not None:
            rows = min(rows, max(room // 2 // max(per_row, 1), 1024))
        return int(min(rows, self.n))

    # -- per step: one launch ----------------------------------------------------------------------------------------
    def gather(self, runs, what):
        """runs: [(pass, lo, hi)], consecutive stretches of index streams.  ((ids, x, y), GatherStatus) of their rows, one
        after another: one mi_batch_gather per run into one set of dense outputs."""
        dev = self.ids_all.device
        rows = sum(hi - lo for _, lo, hi in runs)
        F = self.ids_all.shape[1]
        ids = torch.empty(rows, F, dtype=torch.int32, device=dev)
        x = torch.empty(rows, self.x_all.shape[1], dtype=torch.float32, device=dev) if self.x_all is not None else None
        y = torch.empty(rows, dtype=torch.uint8, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        at = 0
        for p, lo, hi in runs:
            to = at + hi - lo
            batch_gather(self.k, self.ids_all, self.x_all, self.y_all, p.on(dev)[lo:hi], ids[at:to],
                         None if x is None else x[at:to], y[at:to], status)
            at = to
        event = None
        if dev.type == "cuda":
            host = torch.empty(2, dtype=torch.int32, pin_memory=True)
            host.copy_(status, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            status = host
        return (ids, x, y), GatherStatus(status, event, what)

    # -- the batches -------------------------------------------------------------------------------------------------
    def batches(self, mode, batch_size, seed=None):
        """(DeviceBatch, labels [B] bool) — TRAIN: shuffled with a 16 * batch_size buffer, forever; otherwise one ordered
        pass, the last batch may be short: trainers/ml_100k.get_input_fn's batches."""
        if mode != TRAIN:
            for s in range(0, self.n, batch_size):
                b = DeviceBatch(self, None, s, min(self.n, s + batch_size))
                yield b, b.labels()
            return
        for stream in shuffle_passes(self.n, batch_size, seed):
            p = _Pass(stream)
            for s in range(0, len(stream) - batch_size + 1, batch_size):
                b = DeviceBatch(self, p, s, s + batch_size)
                yield b, b.labels()


def dataset_input_fn(load, mode, batch_size, seed=None):
    """input_fn() over the DeviceDataset that load() makes — load() runs at the first call only: the dataset, and what it
    has bound to the device, is kept across calls (an evaluation reads and transforms its file once per run, not once per
    evaluation)."""
    kept = []

    def input_fn():
        if not kept:
            kept.append(load())
        return kept[0].batches(mode, batch_size, seed)
    input_fn.dataset = lambda: kept[0] if kept else None
    return input_fn
