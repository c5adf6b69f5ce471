"""The numpy stand-in for mi_pair_target_ranks — TEST INFRASTRUCTURE ONLY (tests.cpu_kernels.NumpyKernels plus that one entry).

The entry is restated from include/mi355x_rec.h on its own: member m's scores are the numpy mi_pair_topk's (the header defines
z_m by that entry), and a target's rank is COUNTED from the definition — the eligible candidates whose (score, index) key is
larger — not read off a sorted list, so a test that compares it with tests.util.host_topk compares two computations."""
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
    def mi_pair_target_ranks(self, members, M, U, I, excl_off, excl_idx, targets, Tq, ranks, target_scores, ws, wsb):
        assert 1 <= M <= _lib.PAIR_TOPK_GROUP_MAX_MEMBERS and len(members) == M and 1 <= Tq <= _lib.PAIR_RANKS_MAX_TARGETS
        assert tuple(targets.shape) == (U, Tq) and targets.dtype == torch.int32 and targets.is_contiguous()
        assert tuple(ranks.shape) == (M, U, Tq) and ranks.dtype == torch.int32
        assert target_scores is None or (tuple(target_scores.shape) == (M, U, Tq) and target_scores.dtype == torch.float32)
        solo = object.__getattribute__(self, "mi_pair_topk")                 # (not an entry call of the code under test)
        off, idx, tg = _np(excl_off), _np(excl_idx), _np(targets)
        ok = np.ones((U, I), bool)
        if off is not None:
            for u in range(U):
                ok[u, idx[off[u]:off[u + 1]]] = False
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
            solo(f(m.a_q, U, m.H1), f(m.s_q, U, m.E), f(m.w_q, U), U, f(m.a_c, I, m.H1), f(m.s_c, I, m.E), f(m.w_c, I), I,
                 m.H1, m.E, f(m.dense, n_dense), lo, wd, m.n_layers, m.activation, None, None, 1, torch.zeros(U, 1),
                 torch.zeros(U, 1, dtype=torch.int32), z, None, 0)
            z = z.numpy().astype(F32)
            for u in range(U):
                for j in range(Tq):
                    t = int(tg[u, j])
                    has = 0 <= t < I and ok[u, t]
                    ranks[i, u, j] = int((beats(z[u], t) & ok[u]).sum()) if has else -1
                    if target_scores is not None:
                        target_scores[i, u, j] = float(z[u, t]) if has else float("nan")


@pytest.fixture
def rank_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins, mi_pair_target_ranks among them"""
    monkeypatch.setattr(engine, "HipKernels", RankKernels)
