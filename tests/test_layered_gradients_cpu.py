"""-m "not gpu": the checker of test_hip_gradients.py's any-shape cases (tests/layered_grad_check.py) on the numpy stand-in.

Two things are shown.  The unmodified stand-in — the header's contract in numpy fp32 — passes every case, so the bars
max(1e-5, 4 x E32) are not tighter than a plain fp32 evaluation deserves.  And the checker has teeth where the device
cases were chosen to look: a stand-in that is wrong only beyond the first 128 x 128 tile, only in the last split-K slab,
or only in an abs-max vector is reported (hold=False returns the failures)."""
import numpy as np
import pytest

from tests.cases import _numpy_engine
from tests.cpu_kernels import F32, NumpyKernels, _np, _publish
from tests.layered_grad_check import CASES, run_case
from tests.util import dropout_mask

BY_NAME = {c.name: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_unmodified_stand_in_passes(case):
    r = run_case(case, _numpy_engine)
    assert r.failures == []


class DerivativeWrongFromRow128(NumpyKernels):
    """mi_dense_bwd_data whose activation derivative is 1 % too large in the second row tile and beyond"""

    def mi_dense_bwd_data(self, dY, lddy, W, Xact, ldxa, dX, lddx, M, N, K, keep, act=1, amax=None):
        NumpyKernels.mi_dense_bwd_data(self, dY, lddy, W, Xact, ldxa, dX, lddx, M, N, K, keep, act, amax)
        if Xact is not None:
            _np(dX)[128:, :K] *= F32(1.01)


class ActivationSkippedFromColumn128(NumpyKernels):
    """mi_dense_fwd that stores the pre-activation (dropout applied) in the second column tile"""

    def mi_dense_fwd(self, X, ldx, W, bias, Y, ldy, M, N, K, relu, keep, seed, amax=None):
        NumpyKernels.mi_dense_fwd(self, X, ldx, W, bias, Y, ldy, M, N, K, relu, keep, seed, amax)
        if relu and N > 128:
            y = (_np(X)[:, :K] @ _np(W) + _np(bias)).astype(F32)
            if keep < 1.0:
                y = (y / F32(keep)) * dropout_mask(seed, M, N, keep)
            _np(Y)[:, 128:N] = y[:, 128:]


class WeightGradientDropsRowsFrom256(NumpyKernels):
    """mi_dense_bwd_weight that loses the examples of the last split-K slab"""

    def mi_dense_bwd_weight(self, X, ldx, dY, lddy, dW, db, M, N, K, ws, wsb, amax=None):
        dy = _np(dY).reshape(M, -1)[:256, :N]
        _np(dW)[:] = _np(X)[:256, :K].T @ dy
        if db is not None:
            _np(db)[:N] = dy.sum(0)


class StaleAbsMax(NumpyKernels):
    """mi_dense_fwd that leaves 2^30 in the abs-max vector of its result (a vector nobody zeroed)"""

    def mi_dense_fwd(self, X, ldx, W, bias, Y, ldy, M, N, K, relu, keep, seed, amax=None):
        NumpyKernels.mi_dense_fwd(self, X, ldx, W, bias, Y, ldy, M, N, K, relu, keep, seed, amax)
        _publish(amax.out if amax is not None else None, np.float32(2.0 ** 30))


MUTATIONS = [
    (DerivativeWrongFromRow128, "sigmoid [130, 40]", ("kernel_0", "d_concat", "d_concat/dlogit")),
    (DerivativeWrongFromRow128, "tanh dropout 0.2 [256, 128]", ("kernel_0", "d_concat", "d_concat/dlogit")),
    (ActivationSkippedFromColumn128, "sigmoid [130, 40]", ("kernel_1",)),
    (ActivationSkippedFromColumn128, "identity [256, 128]", ()),            # (nothing to skip: identity IS the pre-activation)
    (WeightGradientDropsRowsFrom256, "tanh dropout 0.2 [130, 40]", ("kernel_0", "kernel_1", "kernel_2", "bias_0")),
    (WeightGradientDropsRowsFrom256, "relu dropout 0.1 [100, 50]", ("kernel_0", "kernel_1", "kernel_2")),
    (StaleAbsMax, "sigmoid dropout 0.2 [256, 128]", ("amax x1",)),
    (StaleAbsMax, "relu dropout 0.1 [100, 50]", ("amax x1",)),
]


@pytest.mark.parametrize("kernels,case,reported", MUTATIONS, ids=["%s / %s" % (k.__name__, c) for k, c, _ in MUTATIONS])
def test_a_stand_in_wrong_past_the_first_tile_is_reported(kernels, case, reported):
    r = run_case(BY_NAME[case], lambda *a, **kw: _numpy_engine(*a, k=kernels(), **kw), hold=False)
    names = {f[0] for f in r.failures}
    print("reported:", sorted(names))
    assert set(reported) <= names, (sorted(names), r.failures)
    assert bool(names) == bool(reported)
