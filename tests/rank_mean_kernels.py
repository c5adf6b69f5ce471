"""The numpy stand-in for mi_pair_target_ranks_mean — TEST INFRASTRUCTURE ONLY (tests.rank_kernels.RankKernels plus that one
entry).

The entry is restated from include/mi355x_rec.h on its own: member m's scores are the numpy mi_pair_topk's, the mean is formed
in numpy fp32 in member order with one division (the header's z), and a target's rank is COUNTED from the definition with
tests.rank_kernels.beats — the eligible candidates whose (score, index) key is larger — not read off a sorted list."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.cpu_kernels import F32, _at, _np
from tests.rank_kernels import RankKernels, beats


class RankMeanKernels(RankKernels):
    def _own_scores(self, m, U, I):
        """member m's [U, I] score matrix: the numpy mi_pair_topk on the member's arguments (not an entry call of the code
        under test)"""
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

    def mi_pair_target_ranks_mean(self, members, M, U, I, excl_off, excl_idx, targets, Tq, ranks, target_scores, ws, wsb):
        assert 1 <= M <= _lib.PAIR_TOPK_GROUP_MAX_MEMBERS and len(members) == M and 1 <= Tq <= _lib.PAIR_RANKS_MAX_TARGETS
        assert tuple(targets.shape) == (U, Tq) and targets.dtype == torch.int32 and targets.is_contiguous()
        assert tuple(ranks.shape) == (U, Tq) and ranks.dtype == torch.int32
        assert target_scores is None or (tuple(target_scores.shape) == (U, Tq) and target_scores.dtype == torch.float32)
        off, idx, tg = _np(excl_off), _np(excl_idx), _np(targets)
        ok = np.ones((U, I), bool)
        if off is not None:
            for u in range(U):
                ok[u, idx[off[u]:off[u + 1]]] = False
        acc = None
        for i in range(M):
            m = members[i]
            after = [] if m.n_layers == 0 else _at(m.widths, m.n_layers + 1, np.int32).tolist()[1:-1]
            assert m.n_layers < 2 or max(after) < 32, "member %d is outside the VALU scope" % i
            z = self._own_scores(m, U, I)
            acc = z if acc is None else (acc + z).astype(F32)
        mean = (acc / F32(M)).astype(F32)
        for u in range(U):
            for j in range(Tq):
                t = int(tg[u, j])
                has = 0 <= t < I and ok[u, t]
                ranks[u, j] = int((beats(mean[u], t) & ok[u]).sum()) if has else -1
                if target_scores is not None:
                    target_scores[u, j] = float(mean[u, t]) if has else float("nan")


@pytest.fixture
def rank_mean_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins, mi_pair_target_ranks_mean among them"""
    monkeypatch.setattr(engine, "HipKernels", RankMeanKernels)
