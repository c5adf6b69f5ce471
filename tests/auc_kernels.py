"""The numpy stand-ins for mi_auc_plan / mi_auc_pair_counts — TEST INFRASTRUCTURE ONLY (tests.cpu_kernels.NumpyKernels plus
those entries).

The entries are restated from include/mi355x_rec.h on their own, and NOT the way the tests' reference counts (a brute force
over all pairs on the bit key): the order of the header is built from float comparisons — a NaN is below every number and
equal to every NaN, numbers compare as floats (so -0 equals +0) — as dense ranks, and the pairs of a segment are counted by
binary search in the segment's sorted negatives."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.cpu_kernels import NumpyKernels


def dense_order(z):
    """int64 ranks with the header's order: 0 for every NaN, 1 + the rank of the value among the distinct numbers"""
    z = np.asarray(z, np.float32)
    out = np.zeros(len(z), np.int64)
    num = ~np.isnan(z)
    if num.any():
        _, inv = np.unique(z[num], return_inverse=True)          # (-0 and +0 are one value: they compare equal)
        out[num] = 1 + inv.reshape(-1)
    return out


class AucKernels(NumpyKernels):
    AUC_MAGIC = 0x617563         # of a plan mi_auc_plan wrote

    def mi_auc_plan(self, seg_off, seg_neg, S, neg_run, table, nbytes, plan):
        off, neg = seg_off.numpy().astype(np.int64), seg_neg.numpy().astype(np.int64)
        assert S >= 1 and len(off) == S + 1 and len(neg) == S and 0 <= neg_run <= 2 ** 24 and nbytes >= 16
        assert off[0] == 0 and (np.diff(off) >= 0).all() and 1 <= off[-1] < 2 ** 31
        assert (neg >= 0).all() and (neg <= np.diff(off)).all()
        run = neg_run or 2048
        pos = np.diff(off) - neg
        both = (neg > 0) & (pos > 0)
        if not hasattr(self, "auc_plans"):
            self.auc_plans = {}
        key = len(self.auc_plans) + 1
        self.auc_plans[key] = (off.copy(), neg.copy())
        plan.device_table, plan.magic, plan.N, plan.n_segments = key, self.AUC_MAGIC, int(off[-1]), S
        plan.n_items = int((-(-pos[both] // 64) * -(-neg[both] // run)).sum())

    def mi_auc_pair_counts(self, plan, logits, member_stride, M, order, counts):
        assert plan.magic == self.AUC_MAGIC and 1 <= M <= _lib.AUC_MAX_MEMBERS and member_stride >= plan.N
        off, neg = self.auc_plans[plan.device_table]
        N, S = plan.N, plan.n_segments
        assert tuple(order.shape) == (N,) and order.dtype == torch.int32 and logits.dtype == torch.float32
        assert tuple(counts.shape) == (M, S, 2) and counts.dtype == torch.int64
        o = order.numpy().astype(np.int64)
        assert sorted(o.tolist()) == list(range(N)), "order is a permutation"
        rows = torch.as_strided(logits, (M, N), (member_stride, 1), logits.storage_offset()).numpy()
        for m in range(M):
            r = dense_order(rows[m])[o]
            for s in range(S):
                n = np.sort(r[off[s]:off[s] + neg[s]])
                p = r[off[s] + neg[s]:off[s + 1]]
                lo, hi = np.searchsorted(n, p, side="left"), np.searchsorted(n, p, side="right")
                counts[m, s, 0] += int(lo.sum())
                counts[m, s, 1] += int((hi - lo).sum())


@pytest.fixture
def auc_kernels(monkeypatch):
    """every engine and every ExactAuc the code under test builds gets the numpy stand-ins, the two AUC entries among them"""
    monkeypatch.setattr(engine, "HipKernels", AucKernels)
