"""-m gpu: the epilogues of gemm.hip's any-shape entries — mi_dense_fwd, mi_dense_fwd_gathered, mi_dense_bwd_data and their
N = 1 matrix-vector forms — through the C ABI against numpy fp64: every activation, with and without dropout, under both
matrix-pipe modes, at shapes with several row and column tiles, with padded leading dimensions and unaligned base pointers
(the launcher picks its kernel by them), with the abs-max output, the exact-zero rule and saturating pre-activations.

References.  Forward: act(X W + b) in fp64, times the host replica of the dropout mask, divided by float32(keep).  Data
gradient: (dY W^T) . mask / keep . f'(pre) with f' taken from the fp64 PRE-activation — the kernels (and the oracle) go
through the stored output instead.  Xact is the forward reference's stored output cast to fp32.

Measures and bars are test_hip_kernels.py's: forward max |got - ref| / rms(fp64 pre-activation) < 1e-5; data gradient
max |got - ref| / rms(unmasked product) < 2e-5.  Where a case exceeds its bar the bar becomes max(bar, 4 x E32), E32 the
same measure for a numpy fp32 evaluation of the reference (test_hip_gradients.py's rule; E32 never comes from the device).
Every figure is printed (pytest -s): EPI <case> device ... fp32 ... bar ...

Outputs are NaN-filled between NaN guard bands (tests.util.guarded_nan), inputs sit in NaN-filled buffers: a store past
the last row or column, or a padding float that reaches a result, shows.  Every call is a shape the header accepts."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests.util import (_chk, _p, _st, dev, dropout_mask, exact_workspace, guarded_nan, guards_intact,
                        workspace_surroundings_intact)

pytestmark = pytest.mark.gpu

FWD_BAR, BWD_BAR, WGRAD_BAR = 1e-5, 2e-5, 1e-5          # (the last: test_dense_bwd_data_and_weight's for dW and db)
# (M, N, K): two row and two column tiles, both ragged, W no float4 operand; whole tiles, float4 everywhere; gemv_fwd_k /
# gemv_dgrad_k; N = 1 through the general kernel (K = 5); one ragged tile
SHAPES = [(129, 130, 70), (256, 128, 64), (300, 1, 128), (77, 1, 5), (33, 48, 36)]
ACTS = [0, 1, 2, 3]
KEEPS = [1.0, 0.8]
SEED = 0x51ED5


def _sigmoid(v):
    return 1 / (1 + np.exp(-v))


def _act(kind, v):
    with np.errstate(over="ignore"):
        return {0: lambda u: u, 1: lambda u: np.maximum(u, 0), 2: _sigmoid, 3: np.tanh}[kind](v)


def _deriv(kind, pre):
    """f'(pre) from the pre-activation"""
    if kind == 1:
        return (pre > 0).astype(pre.dtype)
    if kind == 2:
        s = _sigmoid(pre)
        return s * (1 - s)
    if kind == 3:
        t = np.tanh(pre)
        return 1 - t * t
    return np.ones_like(pre)


@contextlib.contextmanager
def _gemm_mode(lib, mode):
    prev = lib.mi_get_gemm_mode()
    _chk(lib.mi_set_gemm_mode(mode))
    try:
        yield
    finally:
        _chk(lib.mi_set_gemm_mode(prev))          # (the switch is process-wide)


def _hold(case, err, bar, e32):
    bar_used = bar if err < bar else max(bar, 4.0 * e32)
    print("EPI %-78s device %.2e  fp32 %.2e  bar %.2e%s" % (case, err, e32, bar_used, "" if err < bar else "  (4 x E32)"))
    assert err < bar_used, (case, err, e32, bar_used)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


# ---- operands and outputs with a leading dimension and a base pointer of the test's choosing ------------------------------
def _operand(a, pad=0, off=0):
    """The matrix a [R, W] on the device with leading dimension W + pad, starting `off` floats into a buffer that is NaN
    everywhere else.  Returns (the buffer — keep it alive —, address, leading dimension)."""
    if a is None:
        return None, None, 0
    R, W = a.shape
    ld = W + pad
    buf = torch.full((off + R * ld,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:].view(R, ld)[:, :W] = dev(a)
    return buf, buf.data_ptr() + 4 * off, ld


class _Output:
    """[R, W] floats with leading dimension W + pad, `off` floats into a NaN buffer between NaN guard bands"""

    def __init__(self, R, W, pad=0, off=0):
        self.R, self.W, self.ld, self.off = R, W, W + pad, off
        self.buf, self.flat = guarded_nan(off + R * self.ld)
        assert self.flat.data_ptr() % 16 == 0
        self.ptr = self.flat.data_ptr() + 4 * off

    def read(self, case):
        """the in-range elements (all finite); the guards, the floats before the base and the padding columns keep their NaN"""
        torch.cuda.synchronize()
        assert guards_intact(self.buf), (case, "a guard band was written")
        assert bool(torch.isnan(self.flat[:self.off]).all()), (case, "a float before the base pointer was written")
        m = self.flat[self.off:].view(self.R, self.ld)
        assert bool(torch.isnan(m[:, self.W:]).all()), (case, "a padding column was written")
        got = m[:, :self.W].cpu().numpy()
        assert np.isfinite(got).all(), (case, "an in-range element is not finite", int((~np.isfinite(got)).sum()))
        return got


def _amax_out():
    from mi355x_rec import _lib as L
    v = torch.zeros(L.AMAX_SLOTS, device="cuda")
    return v, L.GemmAmax(None, None, _p(v))


def _same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- the forward ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_problem(M, N, K):
    rng = np.random.default_rng(1000 * M + 10 * N + K)
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    pre64 = X.astype(np.float64) @ W.astype(np.float64) + b
    pre32 = X @ W + b
    assert pre32.dtype == np.float32
    return X, W, b, pre64, pre32


def _fwd_refs(prob, act, keep):
    """(fp64 reference, numpy fp32 evaluation of it)"""
    _, _, _, pre64, pre32 = prob
    M, N = pre64.shape
    ref, r32 = _act(act, pre64), _act(act, pre32)
    assert r32.dtype == np.float32
    if keep < 1.0:
        mask = dropout_mask(SEED, M, N, keep)
        ref = ref * mask / np.float64(np.float32(keep))
        r32 = (r32 / np.float32(keep)) * mask
    return ref, r32


def _run_fwd(lib, prob, act, keep, case, pad=0, off_x=0, off_w=0, off_y=0):
    """mi_dense_fwd on the problem; returns (in-range output, value of the abs-max vector it was given)"""
    X, W, b = prob[:3]
    (M, K), N = X.shape, W.shape[1]
    xb, xp, ldx = _operand(X, pad, off_x)
    wb, wp, _ = _operand(W, 0, off_w)
    bb = dev(b)
    out = _Output(M, N, pad, off_y)
    av, ga = _amax_out()
    _chk(lib.mi_dense_fwd(xp, ldx, wp, _p(bb), out.ptr, out.ld, M, N, K, act, keep, SEED, ga, _st()))
    got = out.read(case)
    return got, float(av.max())


def _check_fwd(lib, prob, act, keep, case, **kw):
    got, amax = _run_fwd(lib, prob, act, keep, case, **kw)
    ref, r32 = _fwd_refs(prob, act, keep)
    scale = _rms(prob[3])
    _hold(case, float(np.max(np.abs(got - ref))) / scale, FWD_BAR, float(np.max(np.abs(r32 - ref))) / scale)
    assert _same_bits(amax, np.abs(got).max()), (case, "abs-max", amax, float(np.abs(got).max()))
    return got


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dense_fwd_activations(lib, M, N, K, act):
    prob = _fwd_problem(M, N, K)
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            for keep in KEEPS:
                got = _check_fwd(lib, prob, act, keep, "fwd (%d, %d, %d) act %d keep %.1f mode %d" % (M, N, K, act, keep, mode))
                if keep < 1.0:          # dropped units are exactly 0, and about a fifth of them are dropped
                    mask = dropout_mask(SEED, M, N, keep)
                    assert not got[mask == 0].any() and 0.1 < (mask == 0).mean() < 0.3


# ---- the data gradient --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_problem(M, N, K):
    """dX[M, K] = dY[M, N] W[K, N]^T, masked by the stored output of a layer whose pre-activation is P [M, K]"""
    rng = np.random.default_rng(2000 * M + 10 * N + K)
    dY = rng.standard_normal((M, N)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    A = rng.standard_normal((M, 8)).astype(np.float32)
    Bm = (rng.standard_normal((8, K)) * 0.5).astype(np.float32)
    c = (rng.standard_normal(K) * 0.3).astype(np.float32)
    P64 = A.astype(np.float64) @ Bm.astype(np.float64) + c
    P32 = A @ Bm + c
    assert float(np.abs(P64).min()) > 1e-30                  # (no relu decision is lost in the cast of the stored output)
    full64 = dY.astype(np.float64) @ W.astype(np.float64).T
    full32 = dY @ W.T
    assert P32.dtype == np.float32 and full32.dtype == np.float32
    return dY, W, P64, P32, full64, full32


def _stored_output(prob, act, keep):
    """what the forward reference stores for the layer below: act(P) (. mask / keep), cast to fp32; and the mask"""
    P64 = prob[2]
    M, K = P64.shape
    y = _act(act, P64)
    mask = None
    if keep < 1.0:
        mask = dropout_mask(SEED + 1, M, K, keep)
        y = y * mask / np.float64(np.float32(keep))
    return y.astype(np.float32), mask


def _bwd_refs(prob, act, keep, given, mask, unit=None):
    """(fp64 reference, numpy fp32 evaluation).  Xact NULL: the plain product.  unit: positions whose stored output was
    replaced by an exact 0 — dropped when there is dropout, derivative f'(0) through the output (1 for identity and tanh)
    when there is none."""
    _, _, P64, P32, full64, full32 = prob
    if not given:
        return full64, full32
    ref, r32 = full64 * _deriv(act, P64), full32 * _deriv(act, P32)
    if unit is not None and keep == 1.0:
        ref, r32 = ref.copy(), r32.copy()
        ref[unit], r32[unit] = full64[unit], full32[unit]
    if keep < 1.0:
        ref = ref * mask / np.float64(np.float32(keep))
        r32 = (r32 / np.float32(keep)) * mask
        if unit is not None:
            ref[unit], r32[unit] = 0, 0
    assert r32.dtype == np.float32
    return ref, r32


def _run_bwd(lib, prob, act, keep, xact, case, pad=0, off_dy=0, off_w=0, off_xa=0, off_dx=0):
    dY, W = prob[:2]
    (M, N), K = dY.shape, W.shape[0]
    yb, yp, lddy = _operand(dY, pad, off_dy)
    wb, wp, _ = _operand(W, 0, off_w)
    ab, ap, ldxa = _operand(xact, pad, off_xa)
    out = _Output(M, K, pad, off_dx)
    av, ga = _amax_out()
    _chk(lib.mi_dense_bwd_data(yp, lddy, wp, ap, ldxa if xact is not None else K, out.ptr, out.ld, M, N, K, keep, act, ga, _st()))
    got = out.read(case)
    return got, float(av.max())


def _check_bwd(lib, prob, act, keep, given, case, unit=None, **kw):
    xact, mask = _stored_output(prob, act, keep)
    if unit is not None:
        xact = xact.copy()
        xact[unit] = 0
    got, amax = _run_bwd(lib, prob, act, keep, xact if given else None, case, **kw)
    ref, r32 = _bwd_refs(prob, act, keep, given, mask, unit)
    scale = _rms(prob[4]) + 1e-30
    _hold(case, float(np.max(np.abs(got - ref))) / scale, BWD_BAR, float(np.max(np.abs(r32 - ref))) / scale)
    assert _same_bits(amax, np.abs(got).max()), (case, "abs-max", amax, float(np.abs(got).max()))
    return got


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dense_bwd_data_activations(lib, M, N, K, act):
    prob = _bwd_problem(M, N, K)
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            for keep in KEEPS:
                for given in (True, False):
                    _check_bwd(lib, prob, act, keep, given, "dgrad (%d, %d, %d) act %d keep %.1f Xact %s mode %d" % (
                        M, N, K, act, keep, "given" if given else "NULL", mode))


def _planted(mask, M, K):
    """a dozen positions the mask keeps, spread over the matrix: the corners' neighbourhoods, the second row tile"""
    rng = np.random.default_rng(M + K)
    rows = np.unique(np.concatenate([[0, M - 1, min(M - 1, 128)], rng.integers(0, M, 9)]))
    idx = (rows, np.array([np.flatnonzero(mask[r])[(7 * j) % int(mask[r].sum())] for j, r in enumerate(rows)]))
    assert mask[idx].all()
    return idx


@pytest.mark.parametrize("act", [0, 3])
@pytest.mark.parametrize("M,N,K", [(129, 130, 70), (300, 1, 128)])
def test_with_dropout_a_stored_output_that_is_exactly_zero_counts_as_dropped(lib, M, N, K, act):
    """identity and tanh: exact zeros planted in Xact at positions the mask KEEPS.  keep = 0.8: the gradient there is
    exactly 0 (the general kernel's EPI_MASK branch, gemv_dgrad_k's copy of it).  keep = 1.0: nothing is ever dropped, the
    same positions get dY W^T x f'(0) = dY W^T."""
    prob = _bwd_problem(M, N, K)
    unit = _planted(dropout_mask(SEED + 1, M, K, 0.8), M, K)
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            got = _check_bwd(lib, prob, act, 0.8, True, "zero rule (%d, %d, %d) act %d keep 0.8 mode %d" % (M, N, K, act, mode), unit=unit)
            assert not got[unit].any()
            got = _check_bwd(lib, prob, act, 1.0, True, "zero rule (%d, %d, %d) act %d keep 1.0 mode %d" % (M, N, K, act, mode), unit=unit)
            assert got[unit].all()


# ---- saturation -----------------------------------------------------------------------------------------------------------------
SATURATING = np.array([30, -30, 88, -88, 100, -100, 1e4, -1e4], np.float32)


@pytest.mark.parametrize("act", [2, 3])
@pytest.mark.parametrize("M,N,K", [(33, 48, 36), (64, 1, 128)])
def test_saturating_pre_activations(lib, M, N, K, act):
    """Pre-activations of +-30, +-88, +-100 and +-1e4 in column 0 (rows 0..7: X[r, 0] is the value, W[:, 0] the first unit
    vector, no bias there): sigmoid and tanh come out finite and within 1e-7 absolute of fp64, everything else stays
    finite, and so does the data gradient through those outputs."""
    rng = np.random.default_rng(M + N + K + act)
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    X[:8, 0] = SATURATING
    W[:, 0], W[0, 0], b[0] = 0, 1, 0
    pre64 = X.astype(np.float64) @ W.astype(np.float64) + b
    assert np.array_equal(pre64[:8, 0], SATURATING.astype(np.float64))
    prob = (X, W, b, pre64, None)
    ref = _act(act, pre64)
    dY = rng.standard_normal((M, 5)).astype(np.float32)
    W2 = rng.standard_normal((N, 5)).astype(np.float32)
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            for keep in KEEPS:
                case = "saturation (%d, %d, %d) act %d keep %.1f mode %d" % (M, N, K, act, keep, mode)
                got, _ = _run_fwd(lib, prob, act, keep, case)              # (finite everywhere: _Output.read)
                kept = dropout_mask(SEED, M, N, keep)[:8, 0] if keep < 1.0 else np.ones(8, np.float32)
                err = np.abs(got[:8, 0].astype(np.float64) - ref[:8, 0] * kept / np.float64(np.float32(keep)))
                print("EPI %-78s worst |got - fp64| at the saturating units %.2e (bar 1e-07)" % (case, float(err.max())))
                assert err.max() < 1e-7, (case, err.tolist())
                # the layer above's data gradient through these stored outputs: dX [M, N] = dY [M, 5] W2 [N, 5]^T, masked
                _run_bwd(lib, (dY, W2), act, keep, got, case + " dgrad")    # (finite everywhere)


# ---- leading dimensions and alignment: what the launcher's vec_ok / gemv_ok decide by ------------------------------------------
LD_SHAPES = [(129, 132, 68), (129, 1, 68)]          # every width a multiple of 4: pad 0 and 8 take float4 loads, pad 1 cannot


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", LD_SHAPES)
def test_dense_fwd_leading_dimensions_and_base_pointers(lib, M, N, K, act):
    prob = _fwd_problem(M, N, K)
    variants = [("ld + 8", dict(pad=8)), ("ld + 1", dict(pad=1)), ("X one float in", dict(off_x=1)),
                ("W one float in", dict(off_w=1)), ("Y one float in", dict(off_y=1))]
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            for name, kw in variants:
                _check_fwd(lib, prob, act, 0.8, "fwd (%d, %d, %d) act %d keep 0.8 mode %d %s" % (M, N, K, act, mode, name), **kw)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", LD_SHAPES)
def test_dense_bwd_data_leading_dimensions_and_base_pointers(lib, M, N, K, act):
    prob = _bwd_problem(M, N, K)
    variants = [("ld + 8", dict(pad=8)), ("ld + 1", dict(pad=1)), ("dY one float in", dict(off_dy=1)),
                ("W one float in", dict(off_w=1)), ("Xact one float in", dict(off_xa=1)), ("dX one float in", dict(off_dx=1))]
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            for name, kw in variants:
                _check_bwd(lib, prob, act, 0.8, True, "dgrad (%d, %d, %d) act %d keep 0.8 mode %d %s" % (M, N, K, act, mode, name), **kw)


@pytest.mark.parametrize("M,N,K", [(300, 132, 68), (300, 1, 68)])
def test_dense_bwd_weight_leading_dimensions_and_base_pointers(lib, M, N, K):
    """dW = X^T dY, db = column sums of dY in three split-K slabs (N = 1: gemv_wgrad_k and its fallback), with the operands'
    abs-max (the f16x2 split where both are float4 operands) and without, into guarded outputs and a workspace of exactly
    the size the library asks for."""
    from mi355x_rec import _lib as L
    rng = np.random.default_rng(M + N + K)
    X = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    dY = (rng.standard_normal((M, N)) * 1e-4).astype(np.float32)
    refW, refb = X.astype(np.float64).T @ dY.astype(np.float64), dY.astype(np.float64).sum(0, keepdims=True)
    eW = float(np.max(np.abs(X.T @ dY - refW))) / _rms(refW)
    eb = float(np.max(np.abs(dY.sum(0, keepdims=True, dtype=np.float32) - refb))) / (_rms(refb) + 1e-30)
    ax, ady = torch.zeros(L.AMAX_SLOTS, device="cuda"), torch.zeros(L.AMAX_SLOTS, device="cuda")
    ax[3], ady[5] = float(np.abs(X).max()), float(np.abs(dY).max())          # (the value is the vector's largest entry)
    nb = lib.mi_dense_bwd_weight_workspace_bytes(M, N, K)
    variants = [("ld + 8", dict(pad=8)), ("ld + 1", dict(pad=1)), ("X one float in", dict(off_x=1)),
                ("dY one float in", dict(off_dy=1)), ("dW one float in", dict(off_dw=1))]
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            for name, kw in variants:
                for ga in (None, L.GemmAmax(_p(ax), _p(ady), None)):
                    case = "wgrad (%d, %d, %d) mode %d %s %s" % (M, N, K, mode, name, "abs-max" if ga is not None else "no abs-max")
                    xb, xp, ldx = _operand(X, kw.get("pad", 0), kw.get("off_x", 0))
                    yb, yp, lddy = _operand(dY, kw.get("pad", 0), kw.get("off_dy", 0))
                    dW, db = _Output(K, N, 0, kw.get("off_dw", 0)), _Output(1, N)
                    wbuf, ws = exact_workspace(nb)
                    _chk(lib.mi_dense_bwd_weight(xp, ldx, yp, lddy, dW.ptr, db.ptr, M, N, K, _p(ws), ws.numel(), ga, _st()))
                    gW, gb = dW.read(case), db.read(case)
                    assert workspace_surroundings_intact(wbuf, ws), case
                    _hold(case + " dW", float(np.max(np.abs(gW - refW))) / _rms(refW), WGRAD_BAR, eW)
                    _hold(case + " db", float(np.max(np.abs(gb - refb))) / (_rms(refb) + 1e-30), WGRAD_BAR, eb)


# ---- the gathered layer 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [2, 3])
@pytest.mark.parametrize("pad", [0, 1])
def test_gathered_forward_equals_the_materialised_concat_bitwise(lib, act, pad):
    """test_gathered_layer1_matches_materialised_bitwise's idea for sigmoid and tanh under dropout (its own cases are relu),
    into a padded, guarded output: the same bits as mi_dense_fwd on the materialised concat, and fp64-accurate."""
    B, F, E, N, keep = 129, 5, 12, 40, 0.8
    rng = np.random.default_rng(B + F + E)
    vocab = rng.integers(2, 60, F)
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    table = rng.standard_normal((int(off[-1]), E)).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    K = F * E
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    t, fo, di, w, bb = dev(table), dev(off[:-1].copy()), dev(ids), dev(W), dev(b)
    concat = torch.empty(B, K, device="cuda")
    _chk(lib.mi_embed_fm_linear_fwd(_p(t), None, _p(fo), _p(di), B, F, E, _p(concat), K, None, None, None, None, 1, 0, _st()))
    X = table[off[:-1][None, :] + ids].reshape(B, K)
    assert np.array_equal(concat.cpu().numpy(), X)
    pre64 = X.astype(np.float64) @ W.astype(np.float64) + b
    ref, r32 = _fwd_refs((X, W, b, pre64, X @ W + b), act, keep)
    for mode in (0, 1):
        with _gemm_mode(lib, mode):
            case = "gathered fwd (%d, %d, %d, %d) act %d keep %.1f ldy N + %d mode %d" % (B, F, E, N, act, keep, pad, mode)
            y0, y1 = _Output(B, N, pad), _Output(B, N, pad)
            a0, g0 = _amax_out()
            a1, g1 = _amax_out()
            _chk(lib.mi_dense_fwd(_p(concat), K, _p(w), _p(bb), y0.ptr, y0.ld, B, N, K, act, keep, SEED, g0, _st()))
            _chk(lib.mi_dense_fwd_gathered(_p(t), _p(fo), _p(di), F, E, _p(w), _p(bb), y1.ptr, y1.ld, B, N, act, keep, SEED, g1, 0, _st()))
            got0, got1 = y0.read(case), y1.read(case)
            assert np.array_equal(got0.view(np.uint32), got1.view(np.uint32)), case
            _hold(case, float(np.max(np.abs(got1 - ref))) / _rms(pre64), FWD_BAR, float(np.max(np.abs(r32 - ref))) / _rms(pre64))
            assert _same_bits(float(a1.max()), np.abs(got1).max()) and _same_bits(float(a0.max()), float(a1.max())), case
