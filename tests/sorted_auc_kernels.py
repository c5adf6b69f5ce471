"""The numpy stand-in for mi_auc_sorted_counts — TEST INFRASTRUCTURE ONLY (tests.auc_kernels.AucKernels plus that entry).

The entry is restated from include/mi355x_rec.h on its own, and NOT the way the tests' reference counts (a brute force over
all pairs on the bit key): the order of the header comes from float comparisons as dense ranks (auc_kernels.dense_order), and
the pairs of a group are counted by binary search in the group's sorted negatives.  It takes what the binding passes: every
SIGNATURES argument but the stream, positionally."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.auc_kernels import AucKernels, dense_order


class SortedAucKernels(AucKernels):
    def mi_auc_sorted_counts(self, logits, member_stride, M, labels, groups, S, N, counts, workspace, workspace_bytes):
        assert 1 <= N < 2 ** 31 and S >= 1 and 1 <= M <= _lib.AUC_MAX_MEMBERS and member_stride >= N
        assert logits.dtype == torch.float32 and labels.dtype == torch.uint8 and tuple(labels.shape) == (N,)
        assert tuple(counts.shape) == (M, S, 2) and counts.dtype == torch.int64
        assert workspace is not None and workspace_bytes >= 1
        assert (groups is None and S == 1) or (groups.dtype == torch.int32 and tuple(groups.shape) == (N,))
        pos = labels.numpy() != 0
        g = np.zeros(N, np.int64) if groups is None else groups.numpy().astype(np.int64)
        rows = torch.as_strided(logits, (M, N), (member_stride, 1), logits.storage_offset()).numpy()
        by_group = np.argsort(g, kind="stable")
        lo_g, hi_g = np.searchsorted(g[by_group], np.arange(S), side="left"), np.searchsorted(g[by_group], np.arange(S), side="right")
        for m in range(M):
            r = dense_order(rows[m])
            for s in np.flatnonzero(hi_g > lo_g):                        # (a group outside [0, S) is never visited)
                who = by_group[lo_g[s]:hi_g[s]]
                n = np.sort(r[who][~pos[who]])
                p = r[who][pos[who]]
                lo, hi = np.searchsorted(n, p, side="left"), np.searchsorted(n, p, side="right")
                counts[m, s, 0] += int(lo.sum())
                counts[m, s, 1] += int((hi - lo).sum())


@pytest.fixture
def sorted_auc_kernels(monkeypatch):
    """every engine, ExactAuc and StreamingExactAuc the code under test builds gets the numpy stand-ins, the sorted AUC
    entry among them"""
    monkeypatch.setattr(engine, "HipKernels", SortedAucKernels)
