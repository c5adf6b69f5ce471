"""The numpy stand-in for mi_batch_gather — TEST INFRASTRUCTURE ONLY (tests.sorted_auc_kernels.SortedAucKernels, which holds
every other stand-in, plus that entry).

The entry is restated from include/mi355x_rec.h on its own, element by element as the header writes it —
ids[b, f] = ids_all[order[b] * ld_ids + f] on the flat storage — and not by the fancy indexing the tests compare with.  A bad
index stores a zero row and label 0, adds 1 to status[0] and takes the maximum of 2^31 - 1 - b into status[1]."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.sorted_auc_kernels import SortedAucKernels

INT32_MAX = 2 ** 31 - 1


def _flat(t):
    """the storage of a CPU tensor from its first element on, as a flat numpy array"""
    n = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    return torch.as_strided(t, (n,), (1,), t.storage_offset()).numpy()


class BatchKernels(SortedAucKernels):
    def mi_batch_gather(self, ids_all, ld_ids, x_all, ld_x, y_all, N, order, B, F, n_num, ids, x, y, status):
        assert ids_all is not None and order is not None and ids is not None and status is not None
        assert 1 <= N <= INT32_MAX and 1 <= B <= INT32_MAX and 1 <= F <= _lib.IDS_MAX_COLUMNS and ld_ids >= F and n_num >= 0
        assert n_num == 0 or (x_all is not None and x is not None and ld_x >= n_num)
        assert (y_all is None) == (y is None)
        assert ids_all.dtype == ids.dtype == order.dtype == status.dtype == torch.int32
        src, dst, o, st = _flat(ids_all), _flat(ids), _flat(order), _flat(status)
        xs, xd = (_flat(x_all), _flat(x)) if n_num else (None, None)
        ys, yd = (_flat(y_all), _flat(y)) if y is not None else (None, None)
        for b in range(B):
            r = int(o[b])
            ok = 0 <= r < N
            if not ok:
                st[0] += 1
                st[1] = max(int(st[1]), INT32_MAX - b)
            for f in range(F):
                dst[b * F + f] = src[r * ld_ids + f] if ok else 0
            for j in range(n_num):
                xd[b * n_num + j] = xs[r * ld_x + j] if ok else 0.0
            if yd is not None:
                yd[b] = ys[r] if ok else 0


@pytest.fixture
def batch_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins, mi_batch_gather among them"""
    monkeypatch.setattr(engine, "HipKernels", BatchKernels)
