"""Exact AUC and per-group AUC (GAUC) of any number of models' logits over one held-out set: the pairs are COUNTED on the
device (mi_auc_plan / mi_auc_pair_counts, include/mi355x_rec.h), one launch for all models, and the two integers per group
become metrics on the host (metrics.auc_from_pair_counts, metrics.gauc_from_counts).

Why, next to the "auc" every evaluation already reports: that one is tf.metrics.auc's trapezoid over 200 thresholds in
probability, whose error depends on the scale of the logits — between the members of a sweep (a grid over learning rates
is a grid over logit scales) it marks the confident member down.  The count has no such error: it is the fraction of
(positive, negative) pairs ranked the right way, ties counting half, exactly.

Two ways to the same integers.  method="pairs" (the default) compares every pair, O(P N-) per model, after the host has laid
the set out once: meant for held-out sets of some ten thousand examples.  method="sorted" sorts every model's examples by
(group, key, label) on the device and counts the tie runs (mi_auc_sorted_counts), O(N log N) and no layout: any size, and
what StreamingExactAuc — an evaluation that meets its data batch by batch (Estimator.evaluate with params["exact_auc"] /
params["gauc_by"], the trainers' --exact-auc / --gauc-by) — ends in."""
import numpy as np
import torch

from . import _lib, engine
from .metrics import exact_auc_from_counts, gauc_from_counts


class _Sizes:
    """The segments' numbers of positives and negatives: what the host formulas need beside the counts"""

    def __init__(self, labels, seg, n_segments):
        sizes = np.bincount(seg, minlength=n_segments).astype(np.int64)
        self.n_neg = np.bincount(seg[labels == 0], minlength=n_segments).astype(np.int64)
        self.n_pos = sizes - self.n_neg
        self.S = int(n_segments)


class _Layout(_Sizes):
    """One evaluation set as mi_auc_plan takes it: order / seg_off / seg_neg from the labels and the examples' segments, the
    plan and the device buffers it points to"""

    def __init__(self, k, labels, seg, n_segments, device, neg_run):
        _Sizes.__init__(self, labels, seg, n_segments)
        # segment major, the negatives of a segment first, equal (segment, label) in the set's own order
        order = np.lexsort((labels, seg)).astype(np.int32)
        sizes = self.n_pos + self.n_neg
        self.seg_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        self.seg_neg = torch.from_numpy(self.n_neg.copy())
        self.order = torch.from_numpy(order).to(device)
        nbytes = int(k.query("mi_auc_plan_bytes", _lib.ptr(self.seg_off), _lib.ptr(self.seg_neg), self.S, int(neg_run)))
        self.table = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        self.plan = _lib.AucPlan()
        k.mi_auc_plan(self.seg_off, self.seg_neg, self.S, int(neg_run), self.table, self.table.numel(), self.plan)


class ExactAuc:
    """The exact AUC — and, with `groups`, the GAUC — of logits over ONE evaluation set, whose labels and groups are given
    once: the layouts and plans (method="pairs") or the labels and the groups' dense numbers (method="sorted") are built
    here and kept on `device`.  Both methods give the same integers, shapes, group_values and metrics; method="auto" takes
    the faster one by the whole set's number of pairs (AUTO_PAIRS).

    labels: uint8 [N] of 0 / 1 (a numpy array or a tensor); groups: None, or an integer or string array [N] naming every
    example's group (for a recommender: its user).  The groups are numbered in ascending order of their VALUE (numpy's
    order of the array's dtype: numbers numerically, strings lexicographically); segment s of counts(..., grouped=True) is
    the s-th smallest value, `group_values[s]`.  The one-segment layout of the whole set is always carried.

    NEG_RUN: the negatives one work item takes (mi_auc_plan's neg_run); 0: the library's choice (tests: no count depends
    on it)."""
    NEG_RUN = 0
    MAX_MEMBERS = _lib.AUC_MAX_MEMBERS
    # method="auto": sort when the whole set has more (positive, negative) pairs than this.  profiles/sorted_auc.md, one
    # member and one group on an MI355X: the pair count is ahead up to 4.66e8 pairs (0.157 against 0.163 ms) and behind from
    # 6.70e8 on (0.199 against 0.163 ms)
    AUTO_PAIRS = 500_000_000

    def __init__(self, labels, groups=None, device="cuda", kernels=None, method="pairs"):
        if method not in ("pairs", "sorted", "auto"):
            raise ValueError("ExactAuc: method must be 'pairs', 'sorted' or 'auto' (got %r)" % (method,))
        y = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if y.ndim != 1 or y.dtype != np.uint8 or len(y) < 1:
            raise ValueError("ExactAuc: labels must be a uint8 [N] array with N >= 1")
        if int(y.max()) > 1:
            raise ValueError("ExactAuc: labels are 0 or 1 (found %d)" % int(y.max()))
        if len(y) >= 2 ** 31:
            raise ValueError("ExactAuc: %d examples (fewer than 2^31)" % len(y))
        self.N = len(y)
        if method == "auto":
            n_pos = int(y.sum())
            method = "sorted" if n_pos * (self.N - n_pos) > self.AUTO_PAIRS else "pairs"
        self.method = method           # what counts: "pairs" or "sorted"
        self.device = torch.device(device)
        self.k = kernels if kernels is not None else engine.HipKernels()
        pairs = method == "pairs"
        zeros = np.zeros(self.N, np.int64)
        self.whole = _Layout(self.k, y, zeros, 1, self.device, self.NEG_RUN) if pairs else _Sizes(y, zeros, 1)
        self.grouped = self.group_values = None
        if groups is not None:
            g = groups.cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
            if g.shape != (self.N,) or g.dtype.kind not in "iuOUS":
                raise ValueError("ExactAuc: groups must be an integer or string [N] array (N = %d)" % self.N)
            self.group_values, seg = np.unique(g, return_inverse=True)
            seg, S = seg.reshape(-1).astype(np.int64), len(self.group_values)
            self.grouped = _Layout(self.k, y, seg, S, self.device, self.NEG_RUN) if pairs else _Sizes(y, seg, S)
        if not pairs:
            # mi_auc_sorted_counts takes the set as it is: the labels, the groups' dense numbers, one workspace for both calls
            self.labels = torch.from_numpy(np.ascontiguousarray(y)).to(self.device)
            self.seg = torch.from_numpy(seg.astype(np.int32)).to(self.device) if groups is not None else None
            S = self.grouped.S if self.grouped is not None else 1
            nbytes = max(int(self.k.query("mi_auc_sorted_workspace_bytes", self.N, n)) for n in {1, S})
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
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
        views of it; one call per layout"""
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
        if self.method == "sorted":
            ws = self.workspace
            self.k.mi_auc_sorted_counts(z, stride, M, self.labels, None, 1, self.N, whole, ws, ws.numel())
            if S:
                self.k.mi_auc_sorted_counts(z, stride, M, self.labels, self.seg, S, self.N, grouped, ws, ws.numel())
            return whole, grouped
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


class StreamingExactAuc:
    """The exact AUC — and, where batches come with groups, the GAUC — of ONE model over an evaluation set that arrives
    batch by batch: add() keeps every batch's logits and labels on the device and its raw group values on the host,
    metrics() joins them, numbers the groups once (ascending value order, as ExactAuc does) and counts with ONE
    mi_auc_sorted_counts call per layout; reset() starts over.  No collective: on N ranks every rank evaluates the same
    batches and counts the same integers."""

    def __init__(self, device="cuda", kernels=None):
        self.device = torch.device(device)
        self.k = kernels
        self.reset()

    def reset(self):
        self._logits, self._labels, self._groups = [], [], []

    def add(self, logits, labels, groups=None):
        """logits: float32 tensor of B logits, labels: B labels (non-zero is positive), both on the device; groups: None, or
        B raw group values (integers or strings) on the host.  Either every batch of a set comes with groups or none does."""
        z = logits.detach().reshape(-1).to(torch.float32)
        y = (labels.detach().reshape(-1) != 0).to(torch.uint8)
        if z.numel() != y.numel() or z.device.type != self.device.type or y.device.type != self.device.type:
            raise ValueError("StreamingExactAuc.add: %d logits and %d labels on %s / %s (one label a logit, both on %s)" % (
                z.numel(), y.numel(), z.device, y.device, self.device))
        if (groups is None) != (not self._groups) and self._logits:
            raise ValueError("StreamingExactAuc.add: every batch of a set comes with groups, or none does")
        if groups is not None:
            g = np.asarray(groups).reshape(-1)
            if len(g) != z.numel() or g.dtype.kind not in "iuOUS":
                raise ValueError("StreamingExactAuc.add: groups must be %d integers or strings" % z.numel())
            self._groups.append(g)
        self._logits.append(z.clone())            # (the engine's logits are a buffer the next batch overwrites)
        self._labels.append(y)

    def metrics(self):
        """{"auc_exact", "auc_exact_pairs"} and, with groups, {"gauc", "gauc_groups"} of everything added since reset()"""
        if not self._logits:
            raise ValueError("StreamingExactAuc.metrics: nothing was added")
        groups = np.concatenate(self._groups) if self._groups else None
        ex = ExactAuc(torch.cat(self._labels), groups, device=self.device, kernels=self.k, method="sorted")
        return ex.metrics(torch.cat(self._logits))[0]
