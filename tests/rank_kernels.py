"""The numpy stand-ins for mi_pair_target_ranks and mi_pair_target_ranks_mean — TEST INFRASTRUCTURE ONLY
(tests.cpu_kernels.NumpyKernels plus those two entries).

The entries are restated from include/mi355x_rec.h on their own: member m's scores are the numpy mi_pair_topk's (the header
defines z_m by that entry), the mean is formed in numpy fp32 in member order with one division (the header's z), and a target's
rank is COUNTED from the definition — the eligible candidates whose (score, index) key is larger — not read off a sorted list,
so a test that compares it with tests.util.host_topk compares two computations."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.cpu_kernels import F32, NumpyKernels, _at, _np
from tests.util import host_topk


def oracle_ranks(scores, targets, excl):
    """int32 [U, Tmax] from the header's selection rule with k = I: a target's rank is its position in host_topk's full list
    of the query (-1: not in it — excluded, outside [0, I) or padding).  scores [U, I] numpy, targets / excl: one sequence
    per query."""
    U, I = scores.shape
    _, order = host_topk(scores, I, excl)
    out = np.full((U, max([len(t) for t in targets] + [0])), -1, np.int32)
    for u in range(U):
        pos = {int(c): r for r, c in enumerate(order[u]) if c >= 0}
        for j, t in enumerate(targets[u]):
            out[u, j] = pos.get(int(t), -1)
    return out


def beats(s, t):
    """[I] bool: does candidate c's key beat target t's, for one query's scores s — score descending, NaN below every number,
    -0 as +0, equal scores by the lower index"""
    c = np.arange(len(s))
    num_c, num_t = ~np.isnan(s), not np.isnan(s[t])
    with np.errstate(invalid="ignore"):
        higher, equal = s > s[t], (s == s[t]) | (~num_c & (not num_t))
    return (num_c & (not num_t)) | ((num_c == num_t) & (higher | (equal & (c < t))))


class RankKernels(NumpyKernels):
    def _own_scores(self, m, i, U, I):
        """member i's [U, I] score matrix: the numpy mi_pair_topk on the member's arguments (not an entry call of the code
        under test)"""
        after = [] if m.n_layers == 0 else _at(m.widths, m.n_layers + 1, np.int32).tolist()[1:-1]
        assert m.n_layers < 2 or max(after) < 32, "member %d is outside the VALU scope" % i
        solo = object.__getattribute__(self, "mi_pair_topk")
        f = lambda p, *shape: None if not p else _at(p, int(np.prod(shape)), np.float32).reshape(*shape)
        lo = _at(m.layer_off, 2 * max(m.n_layers, 1), np.int64)
        wd = _at(m.widths, m.n_layers + 1, np.int32)
        n_dense = 1
        for j in range(m.n_layers):
            n_dense = max(n_dense, int(lo[2 * j]) + int(wd[j]) * int(wd[j + 1]), int(lo[2 * j + 1]) + int(wd[j + 1]))
        z = torch.zeros(U, I)
        solo(f(m.a_q, U, m.H1), f(m.s_q, U, m.E), f(m.w_q, U), U, f(m.a_c, I, m.H1), f(m.s_c, I, m.E), f(m.w_c, I), I,
             m.H1, m.E, f(m.dense, n_dense), lo, wd, m.n_layers, m.activation, None, None, 1, torch.zeros(U, 1),
             torch.zeros(U, 1, dtype=torch.int32), z, None, 0)
        return z.numpy().astype(F32)

    @staticmethod
    def _check_call(members, M, U, I, targets, Tq, ranks, target_scores, out_shape):
        assert 1 <= M <= _lib.PAIR_TOPK_GROUP_MAX_MEMBERS and len(members) == M and 1 <= Tq <= _lib.PAIR_RANKS_MAX_TARGETS
        assert tuple(targets.shape) == (U, Tq) and targets.dtype == torch.int32 and targets.is_contiguous()
        assert tuple(ranks.shape) == out_shape and ranks.dtype == torch.int32
        assert target_scores is None or (tuple(target_scores.shape) == out_shape and target_scores.dtype == torch.float32)

    @staticmethod
    def _eligible(U, I, excl_off, excl_idx):
        """[U, I] bool: the candidates that the query's exclusion list leaves in"""
        off, idx = _np(excl_off), _np(excl_idx)
        ok = np.ones((U, I), bool)
        if off is not None:
            for u in range(U):
                ok[u, idx[off[u]:off[u + 1]]] = False
        return ok

    @staticmethod
    def _count(z, ok, targets, ranks, target_scores):
        """ranks / target_scores [U, Tq] (views of the outputs) under the [U, I] score matrix z"""
        tg = _np(targets)
        U, I = z.shape
        for u in range(U):
            for j in range(tg.shape[1]):
                t = int(tg[u, j])
                has = 0 <= t < I and ok[u, t]
                ranks[u, j] = int((beats(z[u], t) & ok[u]).sum()) if has else -1
                if target_scores is not None:
                    target_scores[u, j] = float(z[u, t]) if has else float("nan")

    def mi_pair_target_ranks(self, members, M, U, I, excl_off, excl_idx, targets, Tq, ranks, target_scores, ws, wsb):
        self._check_call(members, M, U, I, targets, Tq, ranks, target_scores, (M, U, Tq))
        ok = self._eligible(U, I, excl_off, excl_idx)
        for i in range(M):
            self._count(self._own_scores(members[i], i, U, I), ok, targets, ranks[i],
                        None if target_scores is None else target_scores[i])

    def mi_pair_target_ranks_mean(self, members, M, U, I, excl_off, excl_idx, targets, Tq, ranks, target_scores, ws, wsb):
        self._check_call(members, M, U, I, targets, Tq, ranks, target_scores, (U, Tq))
        acc = None
        for i in range(M):
            z = self._own_scores(members[i], i, U, I)
            acc = z if acc is None else (acc + z).astype(F32)
        self._count((acc / F32(M)).astype(F32), self._eligible(U, I, excl_off, excl_idx), targets, ranks, target_scores)


@pytest.fixture
def rank_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins, the two rank entries among them"""
    monkeypatch.setattr(engine, "HipKernels", RankKernels)
