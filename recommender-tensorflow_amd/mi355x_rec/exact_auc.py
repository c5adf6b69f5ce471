"""Exact AUC and per-group AUC (GAUC) of any number of models' logits over one held-out set: the pairs are COUNTED on the
device (mi_auc_plan / mi_auc_pair_counts, include/mi355x_rec.h), one launch for all models, and the two integers per group
become metrics on the host (metrics.auc_from_pair_counts, metrics.gauc_from_counts).

Why, next to the "auc" every evaluation already reports: that one is tf.metrics.auc's trapezoid over 200 thresholds in
probability, whose error depends on the scale of the logits — between the members of a sweep (a grid over learning rates
is a grid over logit scales) it marks the confident member down.  The count has no such error: it is the fraction of
(positive, negative) pairs ranked the right way, ties counting half, exactly.

The count is O(P N-) per model: meant for held-out sets of some ten thousand examples, not for millions."""
import numpy as np
import torch

from . import _lib, engine
from .metrics import exact_auc_from_counts, gauc_from_counts


class _Layout:
    """One evaluation set as mi_auc_plan takes it: order / seg_off / seg_neg from the labels and the examples' segments, the
    plan and the device buffers it points to"""

    def __init__(self, k, labels, seg, n_segments, device, neg_run):
        # segment major, the negatives of a segment first, equal (segment, label) in the set's own order
        order = np.lexsort((labels, seg)).astype(np.int32)
        sizes = np.bincount(seg, minlength=n_segments).astype(np.int64)
        self.n_neg = np.bincount(seg[labels == 0], minlength=n_segments).astype(np.int64)
        self.n_pos = sizes - self.n_neg
        self.S = int(n_segments)
        self.seg_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        self.seg_neg = torch.from_numpy(self.n_neg.copy())
        self.order = torch.from_numpy(order).to(device)
        nbytes = int(k.query("mi_auc_plan_bytes", _lib.ptr(self.seg_off), _lib.ptr(self.seg_neg), self.S, int(neg_run)))
        self.table = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        self.plan = _lib.AucPlan()
        k.mi_auc_plan(self.seg_off, self.seg_neg, self.S, int(neg_run), self.table, self.table.numel(), self.plan)


class ExactAuc:
    """The exact AUC — and, with `groups`, the GAUC — of logits over ONE evaluation set, whose labels and groups are given
    once: the layouts and plans are built here and kept on `device`.

    labels: uint8 [N] of 0 / 1 (a numpy array or a tensor); groups: None, or an integer or string array [N] naming every
    example's group (for a recommender: its user).  The groups are numbered in ascending order of their VALUE (numpy's
    order of the array's dtype: numbers numerically, strings lexicographically); segment s of counts(..., grouped=True) is
    the s-th smallest value, `group_values[s]`.  The one-segment layout of the whole set is always carried.

    NEG_RUN: the negatives one work item takes (mi_auc_plan's neg_run); 0: the library's choice (tests: no count depends
    on it)."""
    NEG_RUN = 0
    MAX_MEMBERS = _lib.AUC_MAX_MEMBERS

    def __init__(self, labels, groups=None, device="cuda", kernels=None):
        y = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if y.ndim != 1 or y.dtype != np.uint8 or len(y) < 1:
            raise ValueError("ExactAuc: labels must be a uint8 [N] array with N >= 1")
        if int(y.max()) > 1:
            raise ValueError("ExactAuc: labels are 0 or 1 (found %d)" % int(y.max()))
        if len(y) >= 2 ** 31:
            raise ValueError("ExactAuc: %d examples (fewer than 2^31)" % len(y))
        self.N = len(y)
        self.device = torch.device(device)
        self.k = kernels if kernels is not None else engine.HipKernels()
        self.whole = _Layout(self.k, y, np.zeros(self.N, np.int64), 1, self.device, self.NEG_RUN)
        self.grouped = self.group_values = None
        if groups is not None:
            g = groups.cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
            if g.shape != (self.N,) or g.dtype.kind not in "iuOUS":
                raise ValueError("ExactAuc: groups must be an integer or string [N] array (N = %d)" % self.N)
            self.group_values, seg = np.unique(g, return_inverse=True)
            self.grouped = _Layout(self.k, y, seg.reshape(-1).astype(np.int64), len(self.group_values), self.device, self.NEG_RUN)
        self._buf = {}             # M -> the zeroed-per-call counts of both layouts, one allocation

    def _logits(self, logits):
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() not in (1, 2) \
                or logits.shape[-1] != self.N or logits.stride(-1) != 1:
            raise ValueError("ExactAuc: logits must be a float32 [M, %d] or [%d] tensor with unit stride along the examples"
                             % (self.N, self.N))
        if logits.device.type != self.device.type:
            raise ValueError("ExactAuc: logits must live on %s" % self.device)
        if logits.dim() == 1:
            return logits, 1, self.N
        M = int(logits.shape[0])
        if M < 1 or M > self.MAX_MEMBERS:
            raise ValueError("ExactAuc: %d models (1 to %d in one launch)" % (M, self.MAX_MEMBERS))
        stride = int(logits.stride(0)) if M > 1 else self.N
        if stride < self.N:
            raise ValueError("ExactAuc: the rows of logits overlap (stride %d, N = %d)" % (stride, self.N))
        return logits, M, stride

    def _count(self, logits):
        """both layouts' counts, zeroed and counted into one allocation: (the whole set's [M, 1, 2], the groups' [M, S, 2]),
        views of it; one launch per layout"""
        z, M, stride = self._logits(logits)
        S = self.grouped.S if self.grouped is not None else 0
        buf = self._buf.get(M)
        if buf is None:
            flat = torch.empty(M * (1 + S) * 2, dtype=torch.int64, device=self.device)
            buf = self._buf[M] = (flat, flat[:M * 2].view(M, 1, 2), flat[M * 2:].view(M, S, 2))
            if len(self._buf) > 4:
                self._buf.pop(next(iter(self._buf)))
        flat, whole, grouped = buf
        flat.zero_()
        self.k.mi_auc_pair_counts(self.whole.plan, z, stride, M, self.whole.order, whole)
        if S:
            self.k.mi_auc_pair_counts(self.grouped.plan, z, stride, M, self.grouped.order, grouped)
        return whole, grouped

    def counts(self, logits, grouped=False):
        """int64 [M, S, 2] on the device (a new tensor): [m, s, 0] the pairs of segment s that model m ranks the right way,
        [m, s, 1] those it ties.  logits: float32 [M, N] or [N] on the device; the row stride may exceed N.
        grouped False: the whole set (S = 1); True: the groups, in `group_values`' order."""
        if grouped and self.grouped is None:
            raise ValueError("ExactAuc: counts(grouped=True) of an ExactAuc without groups")
        whole, by_group = self._count(logits)
        return (by_group if grouped else whole).clone()

    def metrics(self, logits):
        """A list of M dicts: auc_exact, auc_exact_pairs and, with groups, gauc, gauc_groups (metrics.exact_auc_from_counts,
        metrics.gauc_from_counts).  One device-to-host copy."""
        whole, by_group = self._count(logits)
        M = whole.shape[0]
        host = self._buf[M][0].cpu().numpy()
        w, g = host[:M * 2].reshape(M, 1, 2), host[M * 2:].reshape(M, -1, 2)
        out = [exact_auc_from_counts(w[m], self.whole.n_pos[0], self.whole.n_neg[0]) for m in range(M)]
        if self.grouped is not None:
            for d, by in zip(out, gauc_from_counts(g, self.grouped.n_pos, self.grouped.n_neg)):
                d.update(by)
        return out
