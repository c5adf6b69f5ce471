"""numpy stand-ins for the device entry points of libmi355x_rec.so — TEST INFRASTRUCTURE ONLY.
(The wide part's strided state views arrive as strided numpy views: lin_stride needs no handling here.)

The CPU (gloo, world_size 2) tests hand an instance to ``DeepFM(_kernels=...)`` so that the REAL
host orchestration (engine.py) and the REAL multi-rank exchange plumbing (parallel.py) run without a
GPU.  Every method restates the contract documented in include/mi355x_rec.h on CPU torch tensors
(in place, through ``.numpy()`` views), using the oracle's update rules for the optimizers.  Nothing
under recommender-tensorflow_amd/ imports this file.

The fused entries (serve, one-launch step, population step and evaluation, ensemble, pair top-K and its group form) are
restated from the header on their own, so that a test built on one does not compare the code under test with itself: none
of them calls the numpy of a layered entry, and none takes a selection, a head or a metric from the package.  Where the
header defines an entry by another one, the stand-in says so in as many words: a member of a population or of a pair group
is the solo fused stand-in, a member of an ensemble is its engine's layered forward on the CPU.
`calls` counts the entries fetched from an instance; a stand-in that needs another one fetches it uncounted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from oracle import deepfm as O
from oracle import optimizers as OO
from tests.util import MASK64, dropout_mask, host_topk

_NAMES = {0: "Adam", 1: "Adagrad", 2: "Ftrl", 3: "RMSProp", 4: "SGD"}
_ACT = {0: lambda v: v, 1: lambda v: np.maximum(v, 0), 2: lambda v: 1 / (1 + np.exp(-v)), 3: np.tanh}
_CT = {np.float32: C.c_float, np.int32: C.c_int32, np.int64: C.c_int64}
F32 = np.float32


def _np(t):
    return None if t is None else t.numpy()


def _at(ptr, n, dtype, stride=1, width=None):
    """the host memory at `ptr` as a tensor: n elements `stride` apart, or n rows of `width`"""
    if not ptr:
        return None
    span = (n - 1) * stride + (width or 1)
    flat = torch.from_numpy(np.ctypeslib.as_array((_CT[dtype] * span).from_address(ptr)))
    return flat.as_strided((n, width), (stride, 1)) if width else flat.as_strided((n,), (stride,))


def _publish(vec, values):
    """an abs-max vector (a tensor, or the address in a mi_gemm_amax_t; may be NULL) raised to max |values|: the header's
    contract — the largest of its MI_AMAX_SLOTS entries is the value, the caller zeroes it"""
    vec = _at(vec, _lib.AMAX_SLOTS, F32) if isinstance(vec, int) else vec
    if vec is not None and np.size(values):
        vec[0] = max(float(vec[0]), float(np.abs(values).max()))


def thresholds():
    """tf.metrics.auc's 200 thresholds as mi_eval_accumulate holds them (fp32 of the fp64 values)"""
    th = np.arange(200, dtype=np.float64) / 199.0
    th[0], th[-1] = 0.0 - 1e-7, 1.0 + 1e-7
    return th.astype(F32)


def sigmoid32(z):
    """mi_sigmoid_stable restated in numpy fp32: e = exp(-|z|); 1 / (1 + e) for z >= 0, e / (1 + e) below"""
    z = np.asarray(z, F32)
    e = np.exp(-np.abs(z)).astype(F32)
    return np.where(z >= 0, F32(1) / (F32(1) + e), e / (F32(1) + e)).astype(F32)


def counters(z, y):
    """mi_eval_accumulate restated: (hist [2, 201], counts [8], sums [3]) of fp32 logits z and labels y"""
    z = np.asarray(z, F32)
    y = np.asarray(y).astype(np.int64)
    p = sigmoid32(z)
    k = np.searchsorted(thresholds(), p, side="left")                    # #{j : th[j] < p}
    hist = np.zeros((2, 201), np.int64)
    np.add.at(hist, (y, k), 1)
    cls = (p > F32(0.5)).astype(np.int64)
    counts = np.array([len(z), y.sum(), cls.sum(), (cls == y).sum(), (cls & y).sum(), (cls & (1 - y)).sum(),
                       ((1 - cls) & y).sum(), 0], np.int64)
    zd = z.astype(np.float64)
    sums = np.array([(np.maximum(zd, 0) - zd * y + np.log1p(np.exp(-np.abs(zd)))).sum(), p.astype(np.float64).sum(), y.sum()])
    return hist, counts, sums


def _select(scores, k, excl_off, excl_idx, top_score, top_idx):
    """the header's selection rule (tests.util.host_topk) on the CSR exclusions, into the entry's outputs"""
    off, idx = _np(excl_off), _np(excl_idx)
    rows = [[] if off is None else idx[off[u]:off[u + 1]].tolist() for u in range(scores.shape[0])]
    top_score.numpy()[:], top_idx.numpy()[:] = host_topk(scores, k, rows)


def _hyper(hp):
    return OO.Hyper(_NAMES[hp.kind], lr=np.float32(hp.lr), beta1=np.float32(hp.beta1), beta2=np.float32(hp.beta2),
                    epsilon=np.float32(hp.epsilon), decay=np.float32(hp.decay), momentum=np.float32(hp.momentum),
                    lr_power=-0.5, l1=np.float32(hp.l1), l2=np.float32(hp.l2))


class NumpyKernels:
    timers = None
    MAGIC = 0x6d69               # of a plan mi_train_group_plan wrote
    GROUP_MAGIC = 0x7072         # of a plan mi_predict_group_plan wrote
    ENGINES = {}                 # register(): the engines a ServeMember's `dense` pointer is recognised by

    def __init__(self):
        self.calls = {}
        self.plans = {}

    def __getattribute__(self, name):
        value = object.__getattribute__(self, name)
        if name.startswith("mi_"):
            calls = object.__getattribute__(self, "calls")
            calls[name] = calls.get(name, 0) + 1
        return value

    def query(self, name, *args):
        return 64 * args[0] if name == "mi_train_group_plan_bytes" else 256

    @classmethod
    def register(cls, engines):
        for e in engines:
            cls.ENGINES[e.dense.data_ptr()] = e

    # ---- ids / routing -----------------------------------------------------------------
    def mi_global_rows(self, ids, field_off, B, F, rows):
        _np(rows)[:] = (_np(ids).astype(np.int64) + _np(field_off)[None, :]).reshape(-1)

    def mi_shard_keys(self, rows, n, world, entries_per_chunk, rows_per_rank, self_rank, keys):
        r = _np(rows)[:n].astype(np.int64)
        chunk = (np.arange(n) // entries_per_chunk) if entries_per_chunk > 0 else 0
        o = r % world
        if self_rank >= 0:
            o = np.where(o == self_rank, world - 1, np.where(o > self_rank, o - 1, o))
        _np(keys)[:n] = (chunk * world + o) * rows_per_rank + r // world

    def mi_route_requests(self, uniq, num_uniq, n_max, rows_per_rank, n_groups, send_rows, counts):
        U = int(_np(num_uniq)[0])
        key = _np(uniq)[:U].astype(np.int64)
        _np(send_rows)[:U] = key % rows_per_rank
        _np(counts)[:n_groups] = np.bincount(key // rows_per_rank, minlength=n_groups)

    def mi_segment_slots(self, seg, sorted_entry, num_uniq, n, slot):
        U = int(_np(num_uniq)[0])
        sg, se = _np(seg), _np(sorted_entry)
        for u in range(U):
            _np(slot)[se[sg[u]:sg[u + 1]]] = u

    def mi_entry_grads_segsum(self, rows, seg, sorted_entry, u_begin, u_count, d_concat, ldd, sumv, dlf, dll, b0, F, E,
                              out_rows, out_lin, out_row0=0, rows_stride=0, out_stride=0):
        sg, se = _np(seg), _np(sorted_entry)
        for u in range(u_begin, u_begin + u_count):
            g = np.zeros(E, np.float32)
            gl = np.float32(0)
            for e in se[sg[u]:sg[u + 1]]:
                b, f = int(e) // F - b0, int(e) % F
                if out_rows is not None:
                    v = np.zeros(E, np.float32)
                    if d_concat is not None:
                        v = v + _np(d_concat)[b, f * E:(f + 1) * E]
                    if dlf is not None:
                        v = v + _np(dlf)[b] * (_np(sumv)[b] - _np(rows)[u])
                    g = g + v
                if out_lin is not None:
                    gl = gl + _np(dll)[b]
            if out_rows is not None:
                _np(out_rows)[u - out_row0] = g
            if out_lin is not None:
                _np(out_lin)[u - out_row0] = gl

    def mi_axpy(self, y, x, n, alpha):
        _np(y)[:n] += np.float32(alpha) * _np(x)[:n]

    def mi_gather_u32(self, src, idx, n, out):
        _np(out)[:n] = _np(src)[_np(idx)[:n]]

    def mi_sort_unique_rows(self, rows, n, total, sorted_entry, uniq, seg, num_uniq, ws, wsb):
        r = _np(rows)[:n]
        order = np.argsort(r, kind="stable").astype(np.int32)
        sr = r[order]
        starts = np.flatnonzero(np.r_[True, sr[1:] != sr[:-1]]).astype(np.int32)
        U = len(starts)
        _np(sorted_entry)[:n] = order
        if uniq is None:
            return
        _np(uniq)[:U] = sr[starts]
        _np(seg)[:U] = starts
        _np(seg)[U] = n
        _np(num_uniq)[0] = U

    def mi_sort_unique_rows_slots(self, rows, n, total, sorted_entry, uniq, seg, num_uniq, slot, ws, wsb):
        self.mi_sort_unique_rows(rows, n, total, sorted_entry, uniq, seg, num_uniq, ws, wsb)
        self.mi_segment_slots(seg, sorted_entry, num_uniq, n, slot)

    # ---- embedding side ------------------------------------------------------------------
    def mi_embed_fm_linear_fwd(self, table, lin_w, field_off, ids, B, F, E, concat, ld, sumv, fm, lin, amax=None, ls=1, ts=0):
        rows = _np(ids).astype(np.int64) + _np(field_off)[None, :]
        if table is not None:
            v = _np(table)[rows]                               # [B,F,E]
            if concat is not None:
                _np(concat)[:, :F * E] = v.reshape(B, F * E)
            _publish(amax, v)
            s = v.sum(1)
            if sumv is not None:
                _np(sumv)[:] = s
            if fm is not None:
                _np(fm)[:] = np.float32(0.5) * (s * s - (v * v).sum(1)).sum(1)
        if lin is not None:
            _np(lin)[:] = _np(lin_w)[rows].sum(1)

    def mi_gather_rows(self, table, lin_w, rows, n, E, out_rows, out_lin, ls=1, ts=0, out_stride=0):
        r = _np(rows)[:n]
        if table is not None:
            _np(out_rows)[:n] = _np(table)[r]
        if lin_w is not None and out_lin is not None:
            _np(out_lin)[:n] = _np(lin_w)[r]

    def mi_numeric_embed_fwd(self, x, V, w_num, B, nd, E, concat, ld, col0, sumv, fm, lin):
        xv, Vv = _np(x), _np(V)
        r = xv[:, :, None] * Vv[None, :, :]
        _np(concat)[:, col0:col0 + nd * E] = r.reshape(B, nd * E)
        if sumv is not None:
            sc = _np(sumv).copy()
            st = sc + r.sum(1)
            _np(sumv)[:] = st
            if fm is not None:
                _np(fm)[:] += np.float32(0.5) * ((st * st - sc * sc) - (r * r).sum(1)).sum(1)
        if lin is not None and w_num is not None:
            _np(lin)[:] += xv @ _np(w_num)

    def mi_numeric_raw_fwd(self, x, w_num, B, nd, concat, ld, col0, ncols, lin):
        xv = _np(x)
        if concat is not None:
            cc = _np(concat)
            cc[:, col0:col0 + ncols] = 0
            cc[:, col0:col0 + nd] = xv
        if lin is not None and w_num is not None:
            acc = _np(lin).copy()
            for j in range(nd):
                acc = acc + xv[:, j] * _np(w_num)[j]
            _np(lin)[:] = acc

    def mi_numeric_raw_bwd(self, x, dll, B, nd, dw, ws, wsb):
        _np(dw)[:nd] = (_np(dll)[:, None] * _np(x)).sum(0)

    def mi_embed_fm_linear_bwd(self, d_concat, lddc, concat, ldc, rows, sumv, dlf, dll, pos, B, F, E, d_rows, d_lin):
        p = np.arange(B * F) if pos is None else _np(pos).reshape(-1)[:B * F].astype(np.int64)
        if d_rows is not None:
            g = np.zeros((B, F, E), np.float32)
            if d_concat is not None:
                g += _np(d_concat)[:, :F * E].reshape(B, F, E)
            if dlf is not None:
                v = _np(rows)[p].reshape(B, F, E) if rows is not None else _np(concat)[:, :F * E].reshape(B, F, E)
                g += _np(dlf)[:, None, None] * (_np(sumv)[:, None, :] - v)
            _np(d_rows)[p] = g.reshape(B * F, E)
        if d_lin is not None:
            _np(d_lin)[p] = np.repeat(_np(dll), F)

    def mi_numeric_embed_bwd(self, x, d_concat, lddc, concat, ldc, col0, sumv, dlf, dll, B, nd, E, dV, dw, ws, wsb):
        g = np.zeros((B, nd, E), np.float32)
        if d_concat is not None:
            g += _np(d_concat)[:, col0:col0 + nd * E].reshape(B, nd, E)
        if dlf is not None:
            v = _np(concat)[:, col0:col0 + nd * E].reshape(B, nd, E)
            g += _np(dlf)[:, None, None] * (_np(sumv)[:, None, :] - v)
        _np(dV)[:nd * E] = np.einsum("bj,bje->je", _np(x), g).reshape(-1)
        if dw is not None:
            _np(dw)[:nd] = (_np(dll)[:, None] * _np(x)).sum(0) if dll is not None else 0

    # ---- MLP ----------------------------------------------------------------------------------
    def mi_absmax(self, x, n, out):
        _publish(out, _np(x).reshape(-1)[:n])      # (the vectors only steer the HIP kernels' fp16 scales; tests read them)

    def mi_dense_fwd(self, X, ldx, W, bias, Y, ldy, M, N, K, relu, keep, seed, amax=None):
        y = _np(X)[:, :K] @ _np(W) + _np(bias)
        y = {0: lambda v: v, 1: lambda v: np.maximum(v, 0), 2: lambda v: 1 / (1 + np.exp(-v)), 3: np.tanh}[int(relu)](y).astype(np.float32)
        if keep < 1.0:
            y = (y / np.float32(keep)) * dropout_mask(seed, M, N, keep)
        _np(Y)[:, :N] = y
        _publish(amax.out if amax is not None else None, y)

    def mi_dense_bwd_data(self, dY, lddy, W, Xact, ldxa, dX, lddx, M, N, K, keep, act=1, amax=None):
        dy = _np(dY).reshape(M, -1)[:, :N]
        g = dy @ _np(W).T
        if Xact is not None:
            xa = _np(Xact)[:, :K]
            if act == 1:
                g = (g * (xa > 0)) / np.float32(keep)
            else:
                y = xa * np.float32(keep)
                d = {0: np.ones_like(y), 2: y * (1 - y), 3: 1 - y * y}[int(act)]
                g = np.where((keep < 1) & (xa == 0), 0, (g / np.float32(keep)) * d).astype(np.float32)
        _np(dX)[:, :K] = g
        _publish(amax.out if amax is not None else None, g)

    def mi_dense_bwd_weight(self, X, ldx, dY, lddy, dW, db, M, N, K, ws, wsb, amax=None):
        dy = _np(dY).reshape(M, -1)[:, :N]
        _np(dW)[:] = _np(X)[:, :K].T @ dy
        if db is not None:
            _np(db)[:N] = dy.sum(0)

    def mi_sigmoid_ce_head(self, lin, lin_bias, fm, dnn, labels, B, scale, logits, loss, dlogit, dsum, ws, wsb):
        x = np.zeros(B, np.float32)
        if lin is not None:                                   # (a NULL lin_bias is a zero bias)
            x = x + (_np(lin) + (_np(lin_bias)[0] if lin_bias is not None else np.float32(0)))
        if fm is not None:
            x = x + _np(fm)
        if dnn is not None:
            x = x + _np(dnn)
        _np(logits)[:] = x
        if labels is not None:
            y = _np(labels).astype(np.float32)
            per = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
            if loss is not None:
                _np(loss)[0] = (per * np.float32(scale)).sum(dtype=np.float32)
            if dlogit is not None:
                e = np.exp(-np.abs(x))
                sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(np.float32)
                d = (sig - y) * np.float32(scale)
                _np(dlogit)[:] = d
                if dsum is not None:
                    _np(dsum)[0] = d.sum(dtype=np.float32)

    # ---- optimizers ---------------------------------------------------------------------------
    def mi_dense_apply(self, param, s0, s1, grad, n, hp):
        h = _hyper(hp)
        z = np.zeros(n, np.float32)
        OO.dense_apply(h, _np(param)[:n], _np(s0)[:n] if s0 is not None else z, _np(s1)[:n] if s1 is not None else z,
                       _np(grad)[:n], np.float32(hp.lr_t))

    def mi_catchup_gap_keys(self, uniq, num_uniq, last_step, n_max, step_to, keys, ls=1):
        U = int(_np(num_uniq)[0])
        k = np.full(n_max, 63, np.int32)
        ls = _np(last_step)[_np(uniq)[:U]]
        k[:U] = np.where((ls > 0) & (ls < step_to), np.minimum(step_to - ls, 62), 0)
        _np(keys)[:n_max] = k

    def mi_catchup_rows_by_gap(self, uniq, num_uniq, last_step, n_max, step_to, ls, rows_out, ws, ws_bytes):
        keys = torch.empty(n_max, dtype=torch.int32)
        self.mi_catchup_gap_keys(uniq, num_uniq, last_step, n_max, step_to, keys, ls)
        _np(rows_out)[:n_max] = _np(uniq)[:n_max][np.argsort(_np(keys), kind="stable")]

    def mi_sparse_catchup(self, table, tm, tv, lin_w, lm, lv, last_step, uniq, num_uniq, n_max, E, step_to, lr_table,
                          b1, b2, eps, flags=0, ls=1, ts=0):
        defer = bool(flags & 1) and uniq is not None          # (flag 2, the bounded-error replay: the exact sweep stands in)
        rows = np.arange(n_max) if uniq is None else _np(uniq)[:int(_np(num_uniq)[0])]
        ls = _np(last_step)
        lr = _np(lr_table)
        b1, b2, eps = np.float32(b1), np.float32(b2), np.float32(eps)
        for r in rows:
            if ls[r] >= step_to:
                continue
            if ls[r] > 0:
                for w, m, v in ((table, tm, tv), (lin_w, lm, lv)):
                    if w is None:
                        continue
                    W, M, V = _np(w), _np(m), _np(v)
                    mr, vr = M[r].copy(), V[r].copy()
                    for s in range(ls[r] + 1, step_to + 1):
                        mr = mr * b1
                        vr = vr * b2
                        W[r] = W[r] - (lr[s] * mr) / (np.sqrt(vr) + eps)
                    if not defer:
                        M[r], V[r] = mr, vr
            if not defer and not (flags & 4):
                ls[r] = step_to

    def mi_sparse_apply(self, table, t0, t1, lin_w, l0, l1, last_step, uniq, seg, sorted_entry, num_uniq, n_max,
                        d_rows, d_lin, E, step, hp, ls=1, ts=0, grad_stride=0):
        h = _hyper(hp)
        U = int(_np(num_uniq)[0])
        rows = _np(uniq)[:U].astype(np.int64)
        sg, se = _np(seg), _np(sorted_entry)
        from mi355x_rec.engine import OptimizerSpec  # noqa: F401
        for w, a, b, g, width in ((table, t0, t1, d_rows, E), (lin_w, l0, l1, d_lin, 1)):
            if w is None:
                continue
            W = _np(w).reshape(-1, width)
            A = _np(a).reshape(-1, width) if a is not None else np.zeros_like(W)
            Bm = _np(b).reshape(-1, width) if b is not None else np.zeros_like(W)
            G = _np(g).reshape(-1, width)
            gsum = np.zeros((U, width), np.float32)
            for u in range(U):
                for kk in range(sg[u], sg[u + 1]):
                    gsum[u] += G[se[kk]]
            wv, av, bv = W[rows], A[rows], Bm[rows]
            if h.name == "Adam":
                b1, b2, eps = np.float32(h.beta1), np.float32(h.beta2), np.float32(h.epsilon)
                if last_step is not None:                       # deferred decay of the steps the row sat out
                    ls = _np(last_step)[rows]
                    missed = np.where(ls > 0, np.maximum(0, step - 1 - ls), 0)
                    for j in range(int(missed.max()) if len(missed) else 0):
                        on = (missed > j)[:, None]
                        av = np.where(on, av * b1, av)
                        bv = np.where(on, bv * b2, bv)
                av = av * b1 + gsum * (np.float32(1) - b1)
                bv = bv * b2 + (gsum * gsum) * (np.float32(1) - b2)
                wv = wv - (np.float32(hp.lr_t) * av) / (np.sqrt(bv) + eps)
            else:
                OO.dense_apply(h, wv, av, bv, gsum, None)
            W[rows] = wv
            if a is not None:
                A[rows] = av
            if b is not None:
                Bm[rows] = bv
        if last_step is not None:
            _np(last_step)[rows] = step

    # ---- gathered / fused single-GPU forms --------------------------------------------------------
    def _concat(self, table, field_off, ids, F, E):
        rows = _np(ids).astype(np.int64) + _np(field_off)[None, :]
        return _np(table)[rows].reshape(len(rows), F * E)

    def mi_dense_fwd_gathered(self, table, field_off, ids, F, E, W, bias, Y, ldy, M, N, relu, keep, seed, amax=None, ts=0):
        X = torch.from_numpy(self._concat(table, field_off, ids, F, E))
        self.mi_dense_fwd(X, F * E, W, bias, Y, ldy, M, N, F * E, relu, keep, seed, amax)

    def mi_dense_bwd_weight_gathered(self, table, field_off, ids, F, E, dY, lddy, dW, db, M, N, ws, wsb, amax=None, ts=0):
        X = torch.from_numpy(self._concat(table, field_off, ids, F, E))
        self.mi_dense_bwd_weight(X, F * E, dY, lddy, dW, db, M, N, F * E, ws, wsb)

    def mi_sparse_apply_fused(self, table, t0, t1, lin_w, l0, l1, last_step, uniq, seg, sorted_entry, num_uniq,
                              n_max, d_concat, ldd, sumv, dlf, dll, F, E, step, hp, ls=1, ts=0):
        n = int(_np(seg)[int(_np(num_uniq)[0])])
        e = np.arange(n)
        b, f = e // F, e % F
        d_rows = d_lin = None
        if table is not None:
            g = np.zeros((n, E), np.float32)
            if d_concat is not None:
                g += _np(d_concat)[:, :F * E].reshape(-1, F, E)[b, f]
            if dlf is not None:
                # w = the row as it is before this update
                U = int(_np(num_uniq)[0])
                row_of = np.empty(n, np.int64)
                sg, se = _np(seg), _np(sorted_entry)
                for u in range(U):
                    row_of[se[sg[u]:sg[u + 1]]] = _np(uniq)[u]
                g += _np(dlf)[b][:, None] * (_np(sumv)[b] - _np(table)[row_of])
            d_rows = torch.from_numpy(g)
        if lin_w is not None:
            d_lin = torch.from_numpy(_np(dll)[b].astype(np.float32))
        self.mi_sparse_apply(table, t0, t1, lin_w, l0, l1, last_step, uniq, seg, sorted_entry, num_uniq, n_max,
                             d_rows, d_lin, E, step, hp)

    # ---- eval counters --------------------------------------------------------------------------
    def mi_binary_predictions(self, logits, labels, B, logistic, probabilities, class_ids, unreduced_loss):
        from oracle import deepfm as O
        x = _np(logits)[:B]
        sig = O.predictions(x)["logistic"]
        if logistic is not None:
            _np(logistic).reshape(-1)[:B] = sig
        if probabilities is not None:
            _np(probabilities).reshape(-1, 2)[:B] = np.stack([1 - sig, sig], 1)
        if class_ids is not None:
            _np(class_ids).reshape(-1)[:B] = sig > 0.5
        if unreduced_loss is not None:
            _np(unreduced_loss).reshape(-1)[:B] = O.head(x, _np(labels)[:B])[2]

    def mi_layer_stats(self, x, n, out4, ws, wsb):
        v = _np(x).reshape(-1)[:n]
        _np(out4)[:4] = [np.mean(v == 0), v.min(), v.max(), v.mean()]

    def mi_eval_accumulate(self, logits, labels, B, hist, counts, sums):
        from oracle.metrics import auc_thresholds
        x = _np(logits)[:B].astype(np.float32)
        y = _np(labels)[:B].astype(np.int64)
        e = np.exp(-np.abs(x))
        p = np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(np.float32)
        kk = (auc_thresholds()[None, :] < p[:, None]).sum(1)
        np.add.at(_np(hist), y * 201 + kk, 1)
        cls = (p > 0.5).astype(np.int64)
        c = _np(counts)
        c[0] += B; c[1] += y.sum(); c[2] += cls.sum(); c[3] += (cls == y).sum()
        c[4] += (cls & y).sum(); c[5] += (cls & (1 - y)).sum(); c[6] += ((1 - cls) & y).sum()
        xd = x.astype(np.float64)
        s = _np(sums)
        s[0] += (np.maximum(xd, 0) - xd * y + np.log1p(np.exp(-np.abs(xd)))).sum()
        s[1] += p.astype(np.float64).sum(); s[2] += y.sum()

    # ---- serving: one fused launch (fp64, its own forward) ---------------------------------------------------------------
    def mi_predict_fused(self, table, ts, lin_w, ls, field_off, ids, x_num, B, F, E, nd, dense, layer_off, widths, n_layers,
                         act, use_linear, use_fm, use_dnn, raw, lin_bias_off, num_emb_off, lin_num_off, wide, logits,
                         logistic, probabilities, class_ids, ws, wsb):
        f64 = lambda t: t.numpy().astype(np.float64)
        d = f64(dense)
        rows = ids.numpy().astype(np.int64) + field_off.numpy()[None, :] if F else None
        x = f64(x_num) if nd else None
        z = np.zeros(B)
        parts = []
        if (use_fm or use_dnn) and F:
            parts.append(f64(table)[rows])                                   # [B, F, E]
        if nd and not raw and (use_fm or use_dnn):
            parts.append(x[:, :, None] * d[num_emb_off:num_emb_off + nd * E].reshape(nd, E)[None])
        if use_linear:
            lin = np.zeros(B)
            for f in range(F):
                if (wide >> f) & 1:
                    lin += f64(lin_w)[rows[:, f]]
            if nd:
                lin += x @ d[lin_num_off:lin_num_off + nd]
            z += lin + d[lin_bias_off]
        if use_fm:
            m = np.concatenate(parts, 1)
            s = m.sum(1)
            z += 0.5 * (s * s - (m * m).sum(1)).sum(1)
        if use_dnn:
            h = np.concatenate([p.reshape(B, -1) for p in parts] + ([x] if (raw and nd) else []), 1)
            lo, wd = layer_off.numpy(), widths.numpy()
            for i in range(n_layers):
                W = d[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]].reshape(wd[i], wd[i + 1])
                h = h @ W[:h.shape[1]] + d[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]]
                if i + 1 < n_layers:
                    h = _ACT[act](h)
            z += h[:, 0]
        if logits is not None:                                               # (rounded by the store: an fp64 buffer keeps fp64)
            logits.numpy().reshape(-1)[:] = z
        z = z.astype(np.float32)
        sig = O.predictions(z)["logistic"]
        if logistic is not None:
            logistic.numpy().reshape(-1)[:] = sig
        if probabilities is not None:
            probabilities.numpy().reshape(-1, 2)[:] = np.stack([1 - sig, sig], 1)
        if class_ids is not None:
            class_ids.numpy().reshape(-1)[:] = sig > 0.5

    # ---- the one-launch train step (fp32: its own forward, backward, touched-row apply and all-rows sweep) ---------------
    def mi_train_step_fused(self, table, t_m, t_v, ts, lin_w, l_m, l_v, ls, last_step, field_off, R, ids, labels, B, F, E,
                            dense, d_m, d_v, n_dense, layer_off, widths, n_layers, act, use_linear, use_fm, use_dnn,
                            lin_bias_off, keep, seed, scale, step, hp, logits, loss, sweep_blocks, ws, wsb):
        f32 = np.float32
        assert hp.kind == 0 and 1 <= B <= 128 and 1 <= F <= 32 and R <= 1 << 18 and n_layers <= 4
        assert bool((last_step.numpy() == step - 1).all()) or step == 1, "every row must be current"
        keep, scale, lr_t = f32(keep), f32(scale), f32(hp.lr_t)
        b1, b2, eps = f32(hp.beta1), f32(hp.beta2), f32(hp.epsilon)
        d = dense.numpy()
        rows = ids.numpy().astype(np.int64) + field_off.numpy()[None, :]
        emb = bool(use_fm or use_dnn)
        T = table.numpy() if emb else None
        V = T[rows] if emb else None                                  # [B, F, E]
        z = np.zeros(B, f32)
        if use_linear:
            z = z + (lin_w.numpy()[rows].sum(1, dtype=f32) + d[lin_bias_off])
        s = None
        if use_fm:
            s = V.sum(1, dtype=f32)
            z = z + f32(0.5) * (s * s - (V * V).sum(1, dtype=f32)).sum(1, dtype=f32)
        acts, Ws = [], []
        lo, wd = layer_off.numpy(), widths.numpy()
        if use_dnn:
            h = V.reshape(B, F * E)
            for i in range(n_layers):
                W = d[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]].reshape(wd[i], wd[i + 1])
                acts.append(h)
                Ws.append(W.copy())
                h = (h @ W + d[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]]).astype(f32)
                if i + 1 < n_layers:
                    h = _ACT[act](h).astype(f32)
                    if keep < 1:
                        h = (h / keep) * dropout_mask((seed + 7919 * i) & MASK64, B, int(wd[i + 1]), keep)
            z = z + h[:, 0]
        y = labels.numpy().astype(f32)
        logits.numpy()[:] = z
        e = np.exp(-np.abs(z))
        loss.numpy()[0] = ((np.maximum(z, 0) - z * y + np.log1p(e)) * scale).sum(dtype=f32)
        dl = ((np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(f32) - y) * scale).astype(f32)
        # backward
        gd = np.zeros(n_dense, f32)
        d_concat = None
        if use_dnn:
            dy = dl[:, None]
            for i in reversed(range(n_layers)):
                gd[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]] = (acts[i].T @ dy).reshape(-1)
                gd[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]] = dy.sum(0, dtype=f32)
                g = (dy @ Ws[i].T).astype(f32)
                if i:
                    x = acts[i]                                        # the layer's stored output: act(pre) / keep, or 0
                    if act == 1:
                        g = np.where(x > 0, g / keep, 0).astype(f32)
                    else:
                        o = x * keep
                        der = {0: np.ones_like(o), 2: o * (1 - o), 3: 1 - o * o}[act]
                        g = np.where((keep < 1) & (x == 0), 0, (g / keep) * der).astype(f32)
                    dy = g
                else:
                    d_concat = g.reshape(B, F, E)
        if use_linear:
            gd[lin_bias_off] = dl.sum(dtype=f32)
        # touched rows: entries summed in ascending entry order, TF's sparse Adam; every other row: one step of the sweep
        flat = rows.reshape(-1)
        touched = np.zeros(R, bool)
        touched[flat] = True
        G = None
        if emb:
            G = np.zeros((B, F, E), f32)
            if d_concat is not None:
                G = G + d_concat
            if use_fm:
                G = G + dl[:, None, None] * (s[:, None, :] - V)
            G = G.reshape(B * F, E)
        gl = np.repeat(dl, F)
        for w, m, v, grad in ((table, t_m, t_v, G), (lin_w, l_m, l_v, gl)):
            if w is None or grad is None or (w is lin_w and not use_linear):
                continue
            Wn, Mn, Vn = w.numpy(), m.numpy(), v.numpy()
            for r in np.flatnonzero(touched):
                g = np.zeros_like(Wn[r])
                for en in np.flatnonzero(flat == r):
                    g = g + grad[en]
                Mn[r] = Mn[r] * b1 + g * (f32(1) - b1)
                Vn[r] = Vn[r] * b2 + (g * g) * (f32(1) - b2)
                Wn[r] = Wn[r] - (lr_t * Mn[r]) / (np.sqrt(Vn[r]) + eps)
            u = ~touched
            Mn[u] = Mn[u] * b1
            Vn[u] = Vn[u] * b2
            Wn[u] = Wn[u] - (lr_t * Mn[u]) / (np.sqrt(Vn[u]) + eps)
        last_step.numpy()[:] = step
        OO.dense_apply(_hyper(hp), d, d_m.numpy(), d_v.numpy(), gd, lr_t)

    # ---- the population: a member is what mi_train_step_fused does to its buffers, lr_t = lr_table[step] and
    #      seed = seed_base + step * 1000003 (self.plans: what mi_train_group_plan decoded, by plan.device_table) ---------
    def mi_train_group_plan(self, members, M, B, F, field_off, table, nbytes, plan):
        if M < 1:
            raise _lib.MiError("mi_train_group_plan failed (-1): train_group_plan: %d members (at least 1)" % M)
        if M > _lib.FUSED_GROUP_MAX_MEMBERS:
            raise _lib.MiError("mi_train_group_plan failed (-2): train_group_plan: %d members (at most %d in one launch)"
                               % (M, _lib.FUSED_GROUP_MAX_MEMBERS))
        assert nbytes >= 64 * M and len(members) == M
        decoded, owned = [], {}
        for i in range(M):
            m = members[i]
            assert m.hp.kind == 0 and m.lr_table and m.lr_table_len >= 2 and m.workspace and 0 < m.keep_prob <= 1
            for p in (m.table, m.t_m, m.t_v, m.lin_w, m.l_m, m.l_v, m.last_step, m.dense, m.d_m, m.d_v, m.workspace):
                if p and p in owned:
                    raise _lib.MiError("mi_train_group_plan failed (-1): train_group_plan: member %d and member %d share a "
                                       "state or workspace pointer" % (owned[p], i))
                if p:
                    owned[p] = i
            E, R, ts, ls, nl = m.E, m.R, m.table_stride or m.E, m.lin_stride, m.n_layers
            d = dict(table=_at(m.table, R, np.float32, ts, E), t_m=_at(m.t_m, R, np.float32, ts, E),
                     t_v=_at(m.t_v, R, np.float32, ts, E), lin_w=_at(m.lin_w, R, np.float32, ls),
                     l_m=_at(m.l_m, R, np.float32, ls), l_v=_at(m.l_v, R, np.float32, ls),
                     last_step=_at(m.last_step, R, np.int32, ls), dense=_at(m.dense, m.n_dense, np.float32),
                     d_m=_at(m.d_m, m.n_dense, np.float32), d_v=_at(m.d_v, m.n_dense, np.float32),
                     layer_off=_at(m.layer_off, max(2 * nl, 1), np.int64), widths=_at(m.widths, nl + 1, np.int32),
                     lr_table=_at(m.lr_table, m.lr_table_len, np.float32),
                     scalars=(ts, ls, R, E, m.n_dense, nl, m.activation, m.use_linear, m.use_fm, m.use_dnn, m.lin_bias_off,
                              m.keep_prob, m.scale, m.seed_base),
                     hp=(m.hp.kind, m.hp.lr, m.hp.beta1, m.hp.beta2, m.hp.epsilon))
            decoded.append(d)
        key = len(self.plans) + 1
        self.plans[key] = (decoded, field_off, B, F)
        plan.device_table, plan.magic, plan.n_members, plan.B, plan.F = key, self.MAGIC, M, B, F
        plan.max_step = min(m.lr_table_len for m in members) - 1

    def mi_train_group_step(self, plan, M, ids, ids_stride, labels, labels_stride, B, step, logits, loss, sweep_blocks):
        assert plan.magic == self.MAGIC and M == plan.n_members and B == plan.B and 1 <= step <= plan.max_step
        decoded, field_off, _, F = self.plans[plan.device_table]
        assert ids_stride in (0, B * F) and labels_stride in (0, B) and tuple(logits.shape) == (M, B) and tuple(loss.shape) == (M,)
        solo = object.__getattribute__(self, "mi_train_step_fused")          # (not an entry call of the code under test)
        for i, d in enumerate(decoded):
            ts, ls, R, E, nd, nl, act, ul, uf, ud, lbo, keep, scale, seed_base = d["scalars"]
            kind, lr, b1, b2, eps = d["hp"]
            hp = _lib.OptHparams(kind, lr, b1, b2, eps, float(d["lr_table"][step]), 0, 0, 0, 0, 0)
            solo(d["table"], d["t_m"], d["t_v"], ts, d["lin_w"], d["l_m"], d["l_v"], ls, d["last_step"], field_off, R,
                 ids[i] if ids_stride else ids, labels[i] if labels_stride else labels, B, F, E, d["dense"], d["d_m"], d["d_v"],
                 nd, d["layer_off"], d["widths"], nl, act, ul, uf, ud, lbo, keep, (seed_base + step * 1000003) & MASK64, scale,
                 step, hp, logits[i], loss[i:i + 1], sweep_blocks, None, 0)

    # (a tile's logits and batch loss are what mi_train_step_fused reports for that batch with keep_prob = 1, taken on
    # COPIES of the member's buffers; the counters are mi_eval_accumulate's, restated in counters() above)
    def mi_eval_group(self, plan, M, ids, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks):
        assert plan.magic == self.MAGIC and M == plan.n_members and N >= 1 and 0 <= blocks <= 1024
        decoded, field_off, B, F = self.plans[plan.device_table]
        T = -(-N // B)
        assert tuple(ids.shape) == (N, F) and tuple(labels.shape) == (N,) and tuple(batch_loss.shape) == (M, T)
        assert tuple(hist.shape) == (M, 2, 201) and tuple(counts.shape) == (M, 8) and tuple(partials.shape) == (M, T, 3)
        assert logits is None or tuple(logits.shape) == (M, N)
        assert N % B == 0 or tuple(tail_scale.shape) == (M,)
        assert not bool(hist.any()) and not bool(counts.any()), "the caller zeroes hist and counts"
        solo = object.__getattribute__(self, "mi_train_step_fused")          # (not an entry call of the code under test)
        for i, d in enumerate(decoded):
            ts, ls, R, E, nd, nl, act, ul, uf, ud, lbo, keep, scale, seed_base = d["scalars"]
            kind, lr, b1, b2, eps = d["hp"]
            hp = _lib.OptHparams(kind, lr, b1, b2, eps, 0.0, 0, 0, 0, 0, 0)
            for t in range(T):
                lo, hi = t * B, min(N, (t + 1) * B)
                n = hi - lo
                c = {k: (None if d[k] is None else d[k].clone()) for k in ("table", "t_m", "t_v", "lin_w", "l_m", "l_v", "last_step",
                                                                           "dense", "d_m", "d_v")}
                z, lb = torch.zeros(n), torch.zeros(1)
                solo(c["table"], c["t_m"], c["t_v"], ts, c["lin_w"], c["l_m"], c["l_v"], ls, torch.zeros_like(c["last_step"]),
                     field_off, R, ids[lo:hi], labels[lo:hi], n, F, E, c["dense"], c["d_m"], c["d_v"], nd, d["layer_off"],
                     d["widths"], nl, act, ul, uf, ud, lbo, 1.0, 0, float(tail_scale[i]) if n < B else scale, 1, hp, z, lb, 0,
                     None, 0)
                batch_loss[i, t] = lb[0]
                if logits is not None:
                    logits[i, lo:hi] = z
                h, cn, sm = counters(z.numpy(), labels[lo:hi].numpy())
                hist[i] += torch.from_numpy(h)
                counts[i] += torch.from_numpy(cn)
                partials[i, t] = torch.from_numpy(sm)

    # ---- the ensemble: member i's logit is that engine's predict_logits on the CPU (found through register()), the mean
    #      is formed in fp32 in member order -------------------------------------------------------------------------------
    def mi_predict_group_plan(self, members, M, F, nd, field_off, table, plan):
        assert 1 <= M <= _lib.PREDICT_GROUP_MAX_MEMBERS and len(members) == M
        self.group = [self.ENGINES[members[i].dense] for i in range(M)]
        for m, e in zip(members, self.group):
            assert (m.E, m.n_layers, m.activation) == (e.E, len(e.layers), e.act) and e.F == F and e.n_numeric == nd
            assert (m.use_linear, m.use_fm, m.use_dnn, m.numeric_raw) == (int(e.use_linear), int(e.use_mf), int(e.use_dnn),
                                                                           int(e.raw_numeric))
        plan.device_table, plan.magic, plan.n_members, plan.F, plan.n_numeric = table.data_ptr(), self.GROUP_MAGIC, M, F, nd

    def mi_predict_group(self, plan, M, ids, x_num, B, member_logits, tickets, logits, logistic, probabilities, class_ids):
        assert plan.magic == self.GROUP_MAGIC and M == plan.n_members == len(self.group) and B >= 1
        assert tuple(ids.shape) == (B, plan.F) and tuple(member_logits.shape) == (M, B)
        assert tuple(tickets.shape) == ((B + 31) // 32,) and tickets.dtype == torch.int32 and not bool(tickets.any())
        acc = None
        for i, e in enumerate(self.group):
            z = e.predict_logits(ids, x_num).numpy().astype(F32)
            member_logits[i] = torch.from_numpy(z)
            acc = z if acc is None else (acc + z).astype(F32)
        z = (acc / F32(M)).astype(F32)
        sig = O.predictions(z)["logistic"]
        logits.numpy().reshape(-1)[:] = z
        logistic.numpy().reshape(-1)[:] = sig
        probabilities.numpy().reshape(-1, 2)[:] = np.stack([1 - sig, sig], 1)
        class_ids.numpy().reshape(-1)[:] = sig > 0.5

    # ---- pair scoring and top-K (fp64 scores, host sort) ------------------------------------------------------------------
    def mi_pair_topk(self, a_q, s_q, w_q, U, a_c, s_c, w_c, I, H1, E, dense, layer_off, widths, n_layers, act,
                     excl_off, excl_idx, k, top_score, top_idx, scores, ws, wsb):
        f = lambda t: t.numpy().astype(np.float64)
        s = np.zeros((U, I))
        if w_q is not None:
            s += f(w_q)[:, None]
        if w_c is not None:
            s += f(w_c)[None, :]
        if E:
            s += f(s_q) @ f(s_c).T
        if H1:
            h = f(a_q)[:, None, :] + f(a_c)[None, :, :]
            if n_layers:
                h = _ACT[act](h)
            d, lo, wd = dense.numpy().astype(np.float64), layer_off.numpy(), widths.numpy()
            for i in range(n_layers):
                W = d[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]].reshape(wd[i], wd[i + 1])
                h = h @ W + d[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]]
                if i + 1 < n_layers:
                    h = _ACT[act](h)
            s += h[:, :, 0]
        s = s.astype(np.float32)
        if scores is not None:
            scores.numpy()[:] = s
        _select(s, k, excl_off, excl_idx, top_score, top_idx)

    # (member m's score is mi_pair_topk's above, the mean is formed in fp32 in member order)
    def mi_pair_topk_group(self, members, M, U, I, excl_off, excl_idx, k, top_score, top_idx, scores, member_scores, ws, wsb):
        assert 1 <= M <= _lib.PAIR_TOPK_GROUP_MAX_MEMBERS and len(members) == M and 1 <= k <= 256
        solo = object.__getattribute__(self, "mi_pair_topk")                 # (not an entry call of the code under test)
        acc = None
        for i in range(M):
            m = members[i]
            after = [] if m.n_layers == 0 else _at(m.widths, m.n_layers + 1, np.int32).tolist()[1:-1]
            assert m.n_layers < 2 or max(after) < 32, "member %d is outside the VALU scope" % i
            f = lambda p, *shape: None if not p else _at(p, int(np.prod(shape)), np.float32).reshape(*shape)
            lo = _at(m.layer_off, 2 * max(m.n_layers, 1), np.int64)
            wd = _at(m.widths, m.n_layers + 1, np.int32)
            n_dense = 1
            for j in range(m.n_layers):
                n_dense = max(n_dense, int(lo[2 * j]) + int(wd[j]) * int(wd[j + 1]), int(lo[2 * j + 1]) + int(wd[j + 1]))
            z = torch.zeros(U, I)
            s_, i_ = torch.zeros(U, k), torch.zeros(U, k, dtype=torch.int32)
            solo(f(m.a_q, U, m.H1), f(m.s_q, U, m.E), f(m.w_q, U), U, f(m.a_c, I, m.H1), f(m.s_c, I, m.E), f(m.w_c, I), I,
                 m.H1, m.E, f(m.dense, n_dense), lo, wd, m.n_layers, m.activation, None, None, k, s_, i_, z, None, 0)
            z = z.numpy().astype(F32)
            if member_scores is not None:
                member_scores.numpy()[i] = z
            acc = z if acc is None else (acc + z).astype(F32)
        mean = (acc / F32(M)).astype(F32)
        if scores is not None:
            scores.numpy()[:] = mean
        _select(mean, k, excl_off, excl_idx, top_score, top_idx)


def library_sized(lib):
    """the stand-ins with every size query answered by the real library: for the tests of what it refuses on the host"""
    k = NumpyKernels()
    k.query = lambda name, *a: getattr(lib, name)(*a)
    return k


@pytest.fixture
def cpu_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins"""
    monkeypatch.setattr(engine, "HipKernels", NumpyKernels)
