"""The categorical id transforms on the device: ``FieldPlan.device_transform(device)`` lowers a plan's columns — the
column constructors of the reference's ``trainers/ml_100k.py:19-35`` — ONCE to the descriptor table of
``mi_ids_transform`` (include/mi355x_rec.h, csrc/ids.hip); ``DeviceTransform.transform`` then takes a batch's RAW columns
to the device (nothing is hashed on the host) and turns them into the id matrix in one launch.  On a CPU device the same
table is run by the host entries (``mi_hash_bucket_*``, ``mi_bucketize_f32``, ``mi_fingerprint64``).

Bad values (an id no table row stands for) never reach the id matrix: the kernel stores row 0 and counts them per column
in ``status``; the status is copied to pinned host memory behind the launch and looked at either at once
(``check=True``) or when the caller uses the batch (``check=False`` -> ``TransformStatus.raise_if_bad()``)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .feature_column import (BucketizedColumn, HashBucketColumn, IdentityColumn, VocabularyListColumn, bad_id_message,
                             encode_strings)

_INT32_MAX = 2 ** 31 - 1


def vocabulary_table(vocab):
    """The vocabulary table of mi_ids_column_t as one uint8 array: uint64 fingerprint[n] ascending, int64 start[n + 1],
    int32 index[n] (+ 4 bytes of padding when n is odd), then the entries' utf-8 in the fingerprints' order."""
    lib = _lib.load()
    enc = [v.encode("utf-8") for v in vocab]
    fps = [lib.mi_fingerprint64(b, len(b)) for b in enc]
    order = sorted(range(len(enc)), key=lambda j: (fps[j], enc[j]))
    n = len(enc)
    fp = np.array([fps[j] for j in order], np.uint64)
    start = np.zeros(n + 1, np.int64)
    np.cumsum([len(enc[j]) for j in order], out=start[1:])
    index = np.zeros(n + (n & 1), np.int32)
    index[:n] = order
    text = np.frombuffer(b"".join(enc[j] for j in order), np.uint8)
    return np.concatenate([fp.view(np.uint8), start.view(np.uint8), index.view(np.uint8), text])


def _is_pair(v):
    """is a feature value a ready (bytes, offsets) pair?  A 2-tuple whose first element is bytes, a bytearray, a uint8
    array or a uint8 tensor and whose second is an array, a tensor or a list — any other tuple is a column of two values."""
    if not (isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], (np.ndarray, torch.Tensor, list))):
        return False
    b = v[0]
    return (isinstance(b, (bytes, bytearray)) or (isinstance(b, np.ndarray) and b.dtype == np.uint8)
            or (isinstance(b, torch.Tensor) and b.dtype == torch.uint8))


def _host_tensor(a, dtype):
    """a numpy array as a CPU tensor of `dtype` (a read-only array, such as the view of a bytes object, is copied)"""
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a if a.flags.writeable else a.copy())


class _Lowered:
    """One categorical column of the plan as mi_ids_transform takes it: everything of its descriptor but the batch's
    values (and, for hash_bucket and identity, whether they arrive as int32, int64 or strings)."""

    def __init__(self, field, column, device):
        c = self.column = column
        self.field = field
        self.table = self.table_np = None
        self.n_table = self.num_oov = 0
        self.default = -1
        if isinstance(c, HashBucketColumn):
            self.family = "hash_bucket"
            dt = c.dtype
            if not (dt in (str, bytes, object, None) or np.issubdtype(np.dtype(dt), np.integer)):
                raise _Refused("hash_bucket of dtype %s: neither integers nor strings" % np.dtype(dt).name)
        elif isinstance(c, BucketizedColumn):
            self.family = "bucketized"
            self.table_np = np.ascontiguousarray(c.boundaries, np.float32)
            self.n_table = len(self.table_np)
        elif isinstance(c, VocabularyListColumn):
            self.family = "vocabulary_list"
            if not all(isinstance(v, str) for v in c.vocab):
                raise _Refused("vocabulary with entries that are not strings")
            if len(set(c.vocab)) != len(c.vocab):
                raise _Refused("vocabulary with duplicate entries")
            self.table_np = vocabulary_table(c.vocab)
            self.n_table, self.num_oov, self.default = len(c.vocab), c.num_oov, c.default_value
        elif isinstance(c, IdentityColumn):
            self.family = "identity"
            self.default = -1 if c.default_value is None else int(c.default_value)
        else:
            raise _Refused("a %s has no device form" % type(c).__name__)
        if not -2 ** 31 <= self.default <= _INT32_MAX:
            raise _Refused("default_value %d is no int32" % self.default)
        if self.table_np is not None:
            self.table = torch.from_numpy(self.table_np).to(device)

    def describe(self):
        c = self.column
        return {"field": self.field, "name": c.name, "key": c.key, "family": self.family, "num_buckets": int(c.num_buckets),
                "n_table": self.n_table, "num_oov": self.num_oov, "default": self.default}


class _Refused(Exception):
    pass


class TransformStatus:
    """The status of one DeviceTransform.transform call: raise_if_bad() waits for the status copy queued behind the launch
    (not for anything queued later) and raises what FieldPlan.transform raises for the first bad example of the first bad
    column in field order, whether the device or the host transformed that column."""

    def __init__(self, owner, features, status, event, host_errors=None):
        self.owner, self.features, self.status, self.event = owner, features, status, event
        self.host_errors = host_errors or {}          # field -> the ValueError of a column that stayed on the host transform

    def bad(self):
        """[(field, count of bad values, lowest bad example)] of the columns that had any"""
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        st = self.status.numpy() if isinstance(self.status, torch.Tensor) else self.status
        return [(f, int(st[f, 0]), _INT32_MAX - int(st[f, 1])) for f in range(st.shape[0]) if st[f, 0] > 0]

    def raise_if_bad(self):
        first = {f: i for f, _, i in self.bad()}
        for f in sorted(set(first) | set(self.host_errors)):          # the first bad column in field order, as on the host
            raise self.host_errors[f] if f in self.host_errors else ValueError(self.owner.message(f, first[f], self.features))


class DeviceTransform:
    def __init__(self, plan, device, kernels=None):
        self.plan = plan
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.F = len(plan.categorical)
        self.lowered = {}             # field -> _Lowered
        self.refused = []             # [(field, column name, reason)]: these columns stay on the host transform
        for f, c in enumerate(plan.categorical):
            try:
                self.lowered[f] = _Lowered(f, c, self.device)
            except _Refused as e:
                self.refused.append((f, c.name, str(e)))
        # maximal runs of consecutive device fields, at most MI_IDS_MAX_COLUMNS each: one launch a run (one for a whole
        # plan the device takes)
        self.runs = []
        for f in sorted(self.lowered):
            if self.runs and self.runs[-1][1] == f and f - self.runs[-1][0] < _lib.IDS_MAX_COLUMNS:
                self.runs[-1][1] = f + 1
            else:
                self.runs.append([f, f + 1])
        self.on_gpu = self.device.type == "cuda"
        self.k = kernels
        if self.on_gpu and self.k is None:
            from .engine import HipKernels
            self.k = HipKernels()

    def table(self):
        """The static part of the descriptor table, one dict per device column in field order."""
        return [self.lowered[f].describe() for f in sorted(self.lowered)]

    # -- one column's values as the descriptor takes them ---------------------------------------------------------------
    def _to_device(self, a):
        return _host_tensor(a, a.dtype).to(self.device, non_blocking=True)

    def _strings(self, v):
        """(bytes uint8, offsets int64 [B + 1]) on the device from a ready pair on either side or a column of strings"""
        if _is_pair(v):
            b, o = v
            if isinstance(b, (bytes, bytearray)):
                b = np.frombuffer(b, np.uint8)
            b = b if isinstance(b, torch.Tensor) else _host_tensor(b, np.uint8)
            o = o if isinstance(o, torch.Tensor) else _host_tensor(o, np.int64)
            if b.dtype != torch.uint8 or o.dtype != torch.int64:
                raise ValueError("a (bytes, offsets) pair is (uint8, int64)")
            if o.device.type == "cpu" and o.numel() and int(o.max()) > b.numel():     # (offsets on the device: the caller's word)
                raise ValueError("an offset of %d, past the %d bytes" % (int(o.max()), b.numel()))
            return b.to(self.device, non_blocking=True).contiguous(), o.to(self.device, non_blocking=True).contiguous()
        blob, offs = encode_strings(v)
        return self._to_device(np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)), self._to_device(offs)

    def _ints(self, v):
        """int32 / int64 values on the device, as they are: a device tensor in place, a host column copied raw"""
        if isinstance(v, torch.Tensor):
            t = v.reshape(-1)
            if t.dtype not in (torch.int32, torch.int64):
                t = t.to(torch.int64)
            return t.to(self.device, non_blocking=True).contiguous()
        a = np.asarray(v).reshape(-1)
        if a.dtype not in (np.int32, np.int64):
            a = a.astype(np.int64)
        return self._to_device(a)

    def _column(self, lw, features):
        """(kind, values, offsets) of one device column for this batch"""
        c = lw.column
        v = features[c.key]
        if lw.family == "bucketized":
            if isinstance(v, torch.Tensor):
                t = v.reshape(-1).to(self.device, non_blocking=True).to(torch.float32).contiguous()
            else:
                t = self._to_device(np.asarray(v, np.float32).reshape(-1))
            return _lib.IDS_BUCKETIZE_F32, t, None
        if lw.family == "vocabulary_list":
            b, o = self._strings(v)
            return _lib.IDS_VOCAB_BYTES, b, o
        if lw.family == "identity":
            t = self._ints(v)
            return (_lib.IDS_IDENTITY_I32 if t.dtype == torch.int32 else _lib.IDS_IDENTITY_I64), t, None
        # hash_bucket: integers hash their decimal text, everything else its utf-8 — decided by the values, as on the host
        is_int = (v.dtype in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) if isinstance(v, torch.Tensor)
                  else (not _is_pair(v) and np.asarray(v).dtype.kind in "iu"))
        if is_int:
            t = self._ints(v)
            return (_lib.IDS_HASH_I32 if t.dtype == torch.int32 else _lib.IDS_HASH_I64), t, None
        if isinstance(v, torch.Tensor):
            raise ValueError("column %r: a hash_bucket column takes integers or strings, not a %s tensor" % (c.name, v.dtype))
        b, o = self._strings(v)
        return _lib.IDS_HASH_BYTES, b, o

    def descriptors(self, features, f0, f1):
        """The mi_ids_column_t array of fields f0..f1-1 for this batch, the tensors it points at, and B"""
        cols = (_lib.IdsColumn * (f1 - f0))()
        keep, B = [], None
        for j, f in enumerate(range(f0, f1)):
            lw = self.lowered[f]
            kind, vals, offs = self._column(lw, features)
            n = (offs.numel() - 1) if offs is not None else vals.numel()
            if B is None:
                B = n
            elif n != B:
                raise ValueError("column %r has %d values, the batch has %d" % (lw.column.name, n, B))
            d = cols[j]
            d.kind, d.num_buckets, d.n_table, d.num_oov, d.default_value = kind, lw.column.num_buckets, lw.n_table, lw.num_oov, lw.default
            d.values, d.offsets = vals.data_ptr(), (offs.data_ptr() if offs is not None else None)
            d.table = lw.table.data_ptr() if lw.table is not None else None
            d.table_host = lw.table_np.ctypes.data if lw.family == "bucketized" else None
            keep.append((vals, offs))
        return cols, keep, B

    # -- the transform ------------------------------------------------------------------------------------------------
    def transform(self, features, out=None, check=True):
        """features: dict key -> B raw values (a device tensor is used in place; a numpy or Python column is copied raw;
        strings also as a ready (uint8 bytes, int64 offsets [B + 1]) pair).  Returns (ids int32 [B, F], x float32
        [B, n_d] or None) on the device — with check=False (ids, x, TransformStatus): nothing has been waited for.
        out: an int32 [>= B, >= F] tensor on the device, rows contiguous, whose first B rows and F columns receive the ids."""
        runs = [self.descriptors(features, f0, f1) + (f0,) for f0, f1 in self.runs]
        host_cols, host_errors = {}, {}
        for f, _, _ in self.refused:                       # (the host transform of the columns the device plan refused)
            c = self.plan.categorical[f]
            v = np.asarray(c.transform(features)).reshape(-1)
            bad = (v < 0) | (v >= c.num_buckets)
            if bad.any():                                  # as the kernel does: row 0 is stored, the status tells
                host_errors[f] = ValueError(bad_id_message(c, v[bad][0]))
                v = np.where(bad, 0, v)
            host_cols[f] = v.astype(np.int32)
        B = runs[0][2] if runs else (len(next(iter(host_cols.values()))) if host_cols else self.plan._batch_size(features))
        if B < 1:
            raise ValueError("an empty batch")
        if out is None:
            out = torch.empty(B, self.F, dtype=torch.int32, device=self.device)
        elif (out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] < B or out.shape[1] < self.F or out.stride(1) != 1
              or out.device != self.device):
            raise ValueError("out: an int32 [>= %d, >= %d] tensor on %s with contiguous rows" % (B, self.F, self.device))
        ld = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], self.F)
        status = torch.zeros(max(self.F, 1), 2, dtype=torch.int32, device=self.device)
        for cols, keep, n, f0 in runs:
            if n != B:
                raise ValueError("columns of %d and of %d values in one batch" % (n, B))
            if self.on_gpu:
                self.k.mi_ids_transform(cols, len(cols), B, out[:, f0:], ld, status[f0:])
            else:
                _run_on_host(cols, keep, B, out, f0, status)
        for f, v in host_cols.items():
            out[:B, f] = torch.from_numpy(v).to(self.device, non_blocking=True)
        x = None
        if self.plan.numeric:
            x = torch.stack([self._numeric(c, features) for c in self.plan.numeric], 1)
        event = None
        if self.on_gpu:
            host = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(status, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            status = host
        st = TransformStatus(self, features, status, event, host_errors)
        ids = out[:B, :self.F]
        if check:
            st.raise_if_bad()
            return ids, x
        return ids, x, st

    def _numeric(self, c, features):
        v = features[c.key]
        if isinstance(v, torch.Tensor):
            return v.reshape(-1).to(self.device, non_blocking=True).to(torch.float32)
        return self._to_device(np.asarray(v, np.float32).reshape(-1))

    def message(self, f, i, features):
        """The ValueError text for example i of field f, whose value is bad — FieldPlan.transform's for the same batch"""
        lw = self.lowered[f]
        c = lw.column
        if lw.family == "identity" and c.default_value is None:
            v = features[c.key]
            v = v.reshape(-1)[i].item() if isinstance(v, torch.Tensor) else np.asarray(v).reshape(-1)[i]
            return "column %s: value %d outside [0, %d)" % (c.key, int(v), c.num_buckets)
        if lw.family in ("identity", "vocabulary_list") and not self._offsets_bad(lw, features, i):
            return bad_id_message(c, lw.default)
        return "column %r: offsets not monotone at %d" % (c.name, i)

    def _offsets_bad(self, lw, features, i):
        v = features[lw.column.key]
        if not _is_pair(v):
            return False
        o = v[1]
        lo, hi = int(o[i]), int(o[i + 1])
        return lo < 0 or hi < lo


def _run_on_host(cols, keep, B, out, f0, status):
    """A CPU device: the descriptor table run by the host entries, with the kernel's treatment of bad values."""
    lib = _lib.load()
    for j, d in enumerate(cols):
        vals, offs = keep[j]
        ids = np.empty(B, np.int64)
        if d.kind in (_lib.IDS_HASH_I64, _lib.IDS_HASH_I32):
            a = np.ascontiguousarray(vals.numpy(), np.int64)
            o32 = np.empty(B, np.int32)
            _lib.check(lib.mi_hash_bucket_i64(a.ctypes.data, B, d.num_buckets, o32.ctypes.data), "mi_hash_bucket_i64")
            ids[:] = o32
        elif d.kind == _lib.IDS_BUCKETIZE_F32:
            o32 = np.empty(B, np.int32)
            _lib.check(lib.mi_bucketize_f32(vals.data_ptr(), B, d.table_host, d.n_table, o32.ctypes.data), "mi_bucketize_f32")
            ids[:] = o32
        elif d.kind in (_lib.IDS_IDENTITY_I64, _lib.IDS_IDENTITY_I32):
            v = vals.numpy().astype(np.int64)
            ids[:] = np.where((v >= 0) & (v < d.num_buckets), v, d.default_value)
        else:
            blob, o = vals.numpy().tobytes(), offs.numpy()
            ok = (o[:-1] >= 0) & (o[1:] >= o[:-1])
            vocab = _HostVocabulary(d) if d.kind == _lib.IDS_VOCAB_BYTES else None
            for i in range(B):
                if not ok[i]:
                    ids[i] = -1
                    continue
                s = blob[o[i]:o[i + 1]]
                h = lib.mi_fingerprint64(s, len(s))
                ids[i] = h % d.num_buckets if vocab is None else vocab.lookup(s, h)
        bad = (ids < 0) | (ids >= d.num_buckets)
        if bad.any():
            status[f0 + j, 0] += int(bad.sum())
            status[f0 + j, 1] = max(int(status[f0 + j, 1]), _INT32_MAX - int(np.flatnonzero(bad)[0]))
            ids[bad] = 0
        out[:B, f0 + j] = torch.from_numpy(ids.astype(np.int32))


class _HostVocabulary:
    """The vocabulary table of a descriptor, read back as the kernel reads it"""

    def __init__(self, d):
        n = self.n = d.n_table
        self.num_oov, self.default = d.num_oov, d.default_value
        head = 8 * n + 8 * (n + 1) + 4 * (n + (n & 1))
        raw = (C.c_uint8 * head).from_address(d.table)
        self.fp = np.frombuffer(raw, np.uint64, n)
        self.start = np.frombuffer(raw, np.int64, n + 1, 8 * n)
        self.index = np.frombuffer(raw, np.int32, n, 8 * n + 8 * (n + 1))
        self.text = bytes((C.c_uint8 * int(self.start[n])).from_address(d.table + head))

    def lookup(self, s, h):
        j = int(np.searchsorted(self.fp, np.uint64(h), "left"))
        while j < self.n and int(self.fp[j]) == h:
            if self.text[self.start[j]:self.start[j + 1]] == s:
                return int(self.index[j])
            j += 1
        return self.n + h % self.num_oov if self.num_oov > 0 else self.default
