"""-m gpu: every HIP kernel of libmi355x_rec.so, through the C ABI, against the CPU oracle.

Tolerances: index / byte work and pure copies are compared bit for bit; fp32 reductions against
the fp64 oracle at 1e-5 relative (north_star's bar) with the error measured against
max(|ref|, rms(ref)) so that entries that cancel to ~0 do not blow the ratio up; optimizer kernels
fed identical gradients are compared bit for bit with the fp32 oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.util import (_chk, _p, _st, bounded_catchup_error, dev, dropout_mask, exact_workspace, guarded_nan, guards_intact,
                        max_err_scaled, workspace_surroundings_intact)

pytestmark = pytest.mark.gpu

TOL = 1e-5


def test_single_hip_runtime(lib):
    """The C ABI must share torch's HIP runtime (one libamdhip64 mapped), else pointers are foreign."""
    from mi355x_rec import _lib
    torch.zeros(1, device="cuda")
    paths = _lib.hip_runtime_paths()
    assert len(paths) == 1, paths


@pytest.mark.parametrize("E", [4, 8, 12, 16, 64, 128, 256])
@pytest.mark.parametrize("B,F", [(1, 1), (7, 5), (300, 26), (65, 40)])
def test_embed_fm_linear_fwd(lib, E, B, F):
    rng = np.random.default_rng(E * 1000 + B + F)
    vocab = rng.integers(2, 50, F)
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    R = int(off[-1])
    table = rng.standard_normal((R, E)).astype(np.float32)
    lin_w = rng.standard_normal(R).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    t, lw, fo, di = dev(table), dev(lin_w), dev(off[:-1].copy()), dev(ids)
    ld = F * E + 8                                     # exercise a padded leading dimension
    concat = torch.full((B, ld), -7.0, device="cuda")
    sumv = torch.empty(B, E, device="cuda")
    fm = torch.empty(B, device="cuda")
    lin = torch.empty(B, device="cuda")
    _chk(lib.mi_embed_fm_linear_fwd(_p(t), _p(lw), _p(fo), _p(di), B, F, E, _p(concat), ld, _p(sumv), _p(fm),
                                    _p(lin), None, 1, 0, _st()))
    rows = off[:-1][None, :] + ids
    ref = table[rows]                                  # [B,F,E]
    got = concat.cpu().numpy()
    assert np.array_equal(got[:, :F * E].reshape(B, F, E), ref)      # gather = exact copy
    assert np.all(got[:, F * E:] == -7.0)                              # padding untouched
    r64 = ref.astype(np.float64)
    assert max_err_scaled(sumv.cpu().numpy(), r64.sum(1)) < TOL
    # fm = 0.5*sum_e(s^2 - q) cancels: measure the error against the magnitude that cancels
    mag = 0.5 * ((r64.sum(1) ** 2).sum(1) + (r64 ** 2).sum((1, 2))) + 1e-30
    assert np.max(np.abs(fm.cpu().numpy() - O.fm_pairwise(ref)) / mag) < 2e-6
    if F == 1:
        assert np.all(fm.cpu().numpy() == 0.0)          # a single field has no pairs: exactly 0
    assert max_err_scaled(lin.cpu().numpy(), lin_w[rows].astype(np.float64).sum(1)) < TOL


def test_embed_fwd_linear_only_and_gather_rows(lib):
    rng = np.random.default_rng(5)
    F, B, E = 6, 100, 16
    vocab = rng.integers(2, 30, F)
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    R = int(off[-1])
    table = rng.standard_normal((R, E)).astype(np.float32)
    lin_w = rng.standard_normal(R).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    lw, fo, di = dev(lin_w), dev(off[:-1].copy()), dev(ids)
    lin = torch.empty(B, device="cuda")
    _chk(lib.mi_embed_fm_linear_fwd(None, _p(lw), _p(fo), _p(di), B, F, E, None, 0, None, None, _p(lin), None, 1, 0, _st()))
    rows = (off[:-1][None, :] + ids)
    ref = np.zeros(B, np.float32)
    for f in range(F):
        ref = ref + lin_w[rows[:, f]]
    assert np.array_equal(lin.cpu().numpy(), ref)       # same sequential fp32 order
    # global rows + gather_rows
    grow = torch.empty(B * F, dtype=torch.int32, device="cuda")
    _chk(lib.mi_global_rows(_p(di), _p(fo), B, F, _p(grow), _st()))
    assert np.array_equal(grow.cpu().numpy(), rows.reshape(-1).astype(np.int32))
    out = torch.empty(B * F, E, device="cuda")
    olin = torch.empty(B * F, device="cuda")
    t = dev(table)
    _chk(lib.mi_gather_rows(_p(t), _p(lw), _p(grow), B * F, E, _p(out), _p(olin), 1, 0, 0, _st()))
    assert np.array_equal(out.cpu().numpy(), table[rows.reshape(-1)])
    assert np.array_equal(olin.cpu().numpy(), lin_w[rows.reshape(-1)])
    # the packed exchange's form (round 4): one record [row | weight | pad x 3] of E + 4 floats per request
    rec = torch.full((B * F, E + 4), 7.0, device="cuda")
    _chk(lib.mi_gather_rows(_p(t), _p(lw), _p(grow), B * F, E, _p(rec), rec.data_ptr() + 4 * E, 1, 0, E + 4, _st()))
    assert torch.equal(rec[:, :E], out) and torch.equal(rec[:, E], olin) and float(rec[:, E + 1:].min()) == 7.0


@pytest.mark.parametrize("E,F,B", [(4, 26, 33), (64, 26, 129), (16, 3, 50)])
def test_embed_bwd_entries(lib, E, F, B):
    rng = np.random.default_rng(E + F + B)
    dc = rng.standard_normal((B, F * E)).astype(np.float32)
    cc = rng.standard_normal((B, F * E)).astype(np.float32)
    sv = cc.reshape(B, F, E).sum(1).astype(np.float32)
    dl = rng.standard_normal(B).astype(np.float32)
    pos = rng.permutation(B * F).astype(np.int32)
    d_rows = torch.empty(B * F, E, device="cuda")
    d_lin = torch.empty(B * F, device="cuda")
    a = [dev(x) for x in (dc, cc, sv, dl, pos)]
    _chk(lib.mi_embed_fm_linear_bwd(_p(a[0]), F * E, _p(a[1]), F * E, None, _p(a[2]), _p(a[3]), _p(a[3]), _p(a[4]), B, F,
                                    E, _p(d_rows), _p(d_lin), _st()))
    ref = dc.reshape(B, F, E).astype(np.float64) + dl[:, None, None].astype(np.float64) * (
        sv[:, None, :].astype(np.float64) - cc.reshape(B, F, E))
    g = d_rows.cpu().numpy()
    assert max_err_scaled(g[pos], ref.reshape(B * F, E)) < TOL
    assert np.array_equal(d_lin.cpu().numpy()[pos], np.repeat(dl, F))
    # the same with the gathered rows held in slot order (multi-GPU receive buffer) instead of a concat
    by_slot = np.empty((B * F, E), np.float32)
    by_slot[pos] = cc.reshape(B * F, E)
    rs = dev(by_slot)
    d_rows2 = torch.empty(B * F, E, device="cuda")
    _chk(lib.mi_embed_fm_linear_bwd(_p(a[0]), F * E, None, 0, _p(rs), _p(a[2]), _p(a[3]), None, _p(a[4]), B, F,
                                    E, _p(d_rows2), None, _st()))
    assert torch.equal(d_rows, d_rows2)


GEMM_SHAPES = [(32, 16, 104), (300, 128, 256), (1000, 1, 128), (257, 130, 70), (128, 128, 32), (513, 64, 1),
               (4096, 512, 1664), (77, 3, 5)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("relu", [0, 1])
def test_dense_fwd(lib, M, N, K, relu):
    rng = np.random.default_rng(M + N + K)
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    Y = torch.empty(M, N, device="cuda")
    x, w, bb = dev(X), dev(W), dev(b)
    _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y), N, M, N, K, relu, 1.0, 0, None, _st()))
    ref = X.astype(np.float64) @ W.astype(np.float64) + b
    pre = ref.copy()
    if relu:
        ref = np.maximum(ref, 0)
    got = Y.cpu().numpy().astype(np.float64)
    scale = np.sqrt(np.mean(pre * pre))
    assert np.max(np.abs(got - ref)) / scale < TOL


def test_dense_fwd_dropout_mask_matches_host_replica(lib):
    M, N, K = 200, 48, 64
    rng = np.random.default_rng(9)
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = rng.standard_normal((K, N)).astype(np.float32)
    b = np.zeros(N, np.float32)
    x, w, bb = dev(X), dev(W), dev(b)
    Y0 = torch.empty(M, N, device="cuda"); Y1 = torch.empty(M, N, device="cuda")
    seed, keep = 0x1234567, 0.9
    _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y0), N, M, N, K, 1, 1.0, seed, None, _st()))
    _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y1), N, M, N, K, 1, keep, seed, None, _st()))
    mask = dropout_mask(seed, M, N, keep)
    assert 0.85 < (mask > 0).mean() < 0.95
    assert np.array_equal(Y1.cpu().numpy(), (Y0.cpu().numpy() / np.float32(keep)) * mask)   # bit exact: y / keep or 0


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_dense_bwd_data_and_weight(lib, M, N, K):
    rng = np.random.default_rng(M * 3 + N + K)
    X = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)     # a post-relu activation
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    dY = rng.standard_normal((M, N)).astype(np.float32)
    x, w, dy = dev(X), dev(W), dev(dY)
    dX = torch.empty(M, K, device="cuda")
    keep = 0.8
    _chk(lib.mi_dense_bwd_data(_p(dy), N, _p(w), _p(x), K, _p(dX), K, M, N, K, keep, 1, None, _st()))
    full = dY.astype(np.float64) @ W.astype(np.float64).T
    ref = full * (X > 0) / np.float64(np.float32(keep))
    scale = np.sqrt(np.mean(full * full)) + 1e-30
    assert np.max(np.abs(dX.cpu().numpy() - ref)) / scale < 2 * TOL
    _chk(lib.mi_dense_bwd_data(_p(dy), N, _p(w), None, K, _p(dX), K, M, N, K, 1.0, 1, None, _st()))
    assert np.max(np.abs(dX.cpu().numpy() - full)) / scale < TOL
    # weight + bias gradient (split-K over M)
    nb = lib.mi_dense_bwd_weight_workspace_bytes(M, N, K)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    dW = torch.empty(K, N, device="cuda"); db = torch.empty(N, device="cuda")
    _chk(lib.mi_dense_bwd_weight(_p(x), K, _p(dy), N, _p(dW), _p(db), M, N, K, _p(ws), ws.numel(), None, _st()))
    refW = X.astype(np.float64).T @ dY.astype(np.float64)
    sW = np.sqrt(np.mean(refW * refW)) + 1e-30
    assert np.max(np.abs(dW.cpu().numpy() - refW)) / sW < TOL
    refb = dY.astype(np.float64).sum(0)
    assert np.max(np.abs(db.cpu().numpy() - refb)) / (np.sqrt(np.mean(refb * refb)) + 1e-30) < TOL
    # reproducible: a second run gives the same bits
    dW2 = torch.empty(K, N, device="cuda")
    _chk(lib.mi_dense_bwd_weight(_p(x), K, _p(dy), N, _p(dW2), None, M, N, K, _p(ws), ws.numel(), None, _st()))
    assert torch.equal(dW, dW2)


@pytest.mark.parametrize("B,F,E,N", [(300, 26, 64, 512), (33, 26, 4, 16), (129, 5, 12, 40), (4096, 3, 128, 64)])
def test_gathered_layer1_matches_materialised_bitwise(lib, B, F, E, N):
    """mi_dense_fwd_gathered / mi_dense_bwd_weight_gathered read the concat in place from the table:
    same tiles, same MFMA order as the materialised operand => identical bits."""
    rng = np.random.default_rng(B + F + E)
    vocab = rng.integers(2, 60, F)
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    table = rng.standard_normal((int(off[-1]), E)).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    K = F * E
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dY = rng.standard_normal((B, N)).astype(np.float32)
    t, fo, di, w, bb, dy = dev(table), dev(off[:-1].copy()), dev(ids), dev(W), dev(b), dev(dY)
    concat = torch.empty(B, K, device="cuda")
    _chk(lib.mi_embed_fm_linear_fwd(_p(t), None, _p(fo), _p(di), B, F, E, _p(concat), K, None, None, None, None, 1, 0, _st()))
    Y0 = torch.empty(B, N, device="cuda"); Y1 = torch.empty(B, N, device="cuda")
    _chk(lib.mi_dense_fwd(_p(concat), K, _p(w), _p(bb), _p(Y0), N, B, N, K, 1, 0.9, 77, None, _st()))
    _chk(lib.mi_dense_fwd_gathered(_p(t), _p(fo), _p(di), F, E, _p(w), _p(bb), _p(Y1), N, B, N, 1, 0.9, 77, None, 0, _st()))
    assert torch.equal(Y0, Y1)
    ws = torch.empty(lib.mi_dense_bwd_weight_workspace_bytes(B, N, K) + 256, dtype=torch.uint8, device="cuda")
    dW0 = torch.empty(K, N, device="cuda"); dW1 = torch.empty(K, N, device="cuda")
    db0 = torch.empty(N, device="cuda"); db1 = torch.empty(N, device="cuda")
    _chk(lib.mi_dense_bwd_weight(_p(concat), K, _p(dy), N, _p(dW0), _p(db0), B, N, K, _p(ws), ws.numel(), None, _st()))
    _chk(lib.mi_dense_bwd_weight_gathered(_p(t), _p(fo), _p(di), F, E, _p(dy), N, _p(dW1), _p(db1), B, N, _p(ws),
                                          ws.numel(), None, 0, _st()))
    assert torch.equal(dW0, dW1) and torch.equal(db0, db1)
    ref = table[off[:-1][None, :] + ids].reshape(B, K).astype(np.float64).T @ dY.astype(np.float64)
    assert np.max(np.abs(dW1.cpu().numpy() - ref)) / (np.sqrt(np.mean(ref * ref)) + 1e-30) < TOL


@pytest.mark.parametrize("M,N,K", [(1000, 512, 1664), (300, 256, 512), (129, 1664, 512), (4096, 384, 264)])
def test_bf16x3_and_fp32_gemm_modes_agree(lib, M, N, K):
    """Both matrix-pipe paths (bf16x3 split, fp32-input MFMA) against the fp64 reference, forward
    (bias + relu + dropout) and masked data gradient."""
    rng = np.random.default_rng(M + N + K)
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dY = rng.standard_normal((M, N)).astype(np.float32)
    x, w, bb, dy = dev(X), dev(W), dev(b), dev(dY)
    assert lib.mi_get_gemm_mode() == 1
    outs = {}
    for tag, mode in (("bf16x3", 1), ("fp32", 0)):
        _chk(lib.mi_set_gemm_mode(mode))
        Y = torch.empty(M, N, device="cuda"); dX = torch.empty(M, K, device="cuda")
        _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y), N, M, N, K, 1, 0.9, 5, None, _st()))
        _chk(lib.mi_dense_bwd_data(_p(dy), N, _p(w), _p(x), K, _p(dX), K, M, N, K, 0.9, 1, None, _st()))
        outs[tag] = (Y.cpu(), dX.cpu())
    _chk(lib.mi_set_gemm_mode(1))
    pre = X.astype(np.float64) @ W.astype(np.float64) + b
    ref = np.maximum(pre, 0) / np.float64(np.float32(0.9)) * dropout_mask(5, M, N, 0.9)
    sc = np.sqrt(np.mean(pre * pre))
    full = dY.astype(np.float64) @ W.astype(np.float64).T
    refd = full * (X > 0) / np.float64(np.float32(0.9))
    for tag in ("bf16x3", "fp32"):
        assert np.max(np.abs(outs[tag][0].numpy() - ref)) / sc < TOL, tag
        assert np.max(np.abs(outs[tag][1].numpy() - refd)) / np.sqrt(np.mean(full * full)) < 2 * TOL, tag


def test_bf16x3_split_error_is_fp32_level(lib):
    """Against fp64 the split path must be as accurate as the fp32-input MFMA (within 2x), also for
    operands with a wide dynamic range — the split is exact, only terms below 2^-24 are dropped."""
    rng = np.random.default_rng(1)
    M, N, K = 512, 256, 2048
    X = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-8, 8, (M, K)))).astype(np.float32)
    W = (rng.standard_normal((K, N)) * np.exp(rng.uniform(-8, 8, (K, N)))).astype(np.float32)
    x, w, bb = dev(X), dev(W), dev(np.zeros(N, np.float32))
    ref = X.astype(np.float64) @ W.astype(np.float64)
    mag = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)      # sum |a||b|: the natural error scale
    err = {}
    for mode in (0, 1):
        _chk(lib.mi_set_gemm_mode(mode))
        Y = torch.empty(M, N, device="cuda")
        _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y), N, M, N, K, 0, 1.0, 0, None, _st()))
        err[mode] = float(np.max(np.abs(Y.cpu().numpy() - ref) / mag))
    _chk(lib.mi_set_gemm_mode(1))
    assert err[0] < 2e-6 and err[1] < 2e-6, err            # both ~ a few fp32 ulps of sum|a||b|
    assert err[1] < 4 * err[0] + 1e-7, err


def _amax_vec(lib, t):
    """abs-max vector (mi_gemm_amax_t entry) of a device tensor via mi_absmax"""
    from mi355x_rec import _lib as L
    v = torch.zeros(L.AMAX_SLOTS, device="cuda")
    _chk(lib.mi_absmax(_p(t), t.numel(), _p(v), _st()))
    return v


def _ga(a, b, out=None):
    from mi355x_rec import _lib as L
    return L.GemmAmax(_p(a), _p(b), None if out is None else _p(out))


# whole-tile shapes take the predicate-free kernels, the others the any-shape ones
F16_SHAPES = [(256, 128, 64), (1024, 512, 1664), (384, 256, 512), (300, 130, 70), (129, 128, 96), (4096, 384, 264)]


@pytest.mark.parametrize("M,N,K", F16_SHAPES)
def test_f16x2_gemms_against_fp64(lib, M, N, K):
    """The scaled fp16 high/low split (three products, abs-max supplied): forward with bias, relu and
    dropout, masked data gradient, weight + bias gradient, all against fp64; and the abs-max the
    forward epilogue emits is exactly max |Y|."""
    rng = np.random.default_rng(M + 7 * N + K)
    X = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dY = (rng.standard_normal((M, N)) * 1e-5).astype(np.float32)          # gradient-sized values (below fp16's normal range)
    x, w, bb, dy = dev(X), dev(W), dev(b), dev(dY)
    ax, aw, ady = _amax_vec(lib, x), _amax_vec(lib, w), _amax_vec(lib, dy)
    from mi355x_rec import _lib as L
    ay = torch.zeros(L.AMAX_SLOTS, device="cuda")
    Y = torch.empty(M, N, device="cuda"); dX = torch.empty(M, K, device="cuda")
    _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y), N, M, N, K, 1, 0.9, 5, _ga(ax, aw, ay), _st()))
    pre = X.astype(np.float64) @ W.astype(np.float64) + b
    ref = np.maximum(pre, 0) / np.float64(np.float32(0.9)) * dropout_mask(5, M, N, 0.9)
    assert np.max(np.abs(Y.cpu().numpy() - ref)) / np.sqrt(np.mean(pre * pre)) < TOL
    assert float(ay.max()) == float(Y.abs().max())
    _chk(lib.mi_dense_bwd_data(_p(dy), N, _p(w), _p(x), K, _p(dX), K, M, N, K, 0.9, 1, _ga(ady, aw), _st()))
    full = dY.astype(np.float64) @ W.astype(np.float64).T
    refd = full * (X > 0) / np.float64(np.float32(0.9))
    assert np.max(np.abs(dX.cpu().numpy() - refd)) / np.sqrt(np.mean(full * full)) < 2 * TOL
    ws = torch.empty(lib.mi_dense_bwd_weight_workspace_bytes(M, N, K) + 256, dtype=torch.uint8, device="cuda")
    dW = torch.empty(K, N, device="cuda"); db = torch.empty(N, device="cuda")
    _chk(lib.mi_dense_bwd_weight(_p(x), K, _p(dy), N, _p(dW), _p(db), M, N, K, _p(ws), ws.numel(), _ga(ax, ady), _st()))
    refW = X.astype(np.float64).T @ dY.astype(np.float64)
    assert np.max(np.abs(dW.cpu().numpy() - refW)) / (np.sqrt(np.mean(refW * refW)) + 1e-30) < TOL
    refb = dY.astype(np.float64).sum(0)
    assert np.max(np.abs(db.cpu().numpy() - refb)) / (np.sqrt(np.mean(refb * refb)) + 1e-30) < TOL


@pytest.mark.parametrize("sx,sw", [(1.0, 1.0), (1e-20, 1e12), (3e18, 2e-9), (1e-30, 1e-6)])
def test_f16x2_error_is_fp32_level_at_any_magnitude(lib, sx, sw):
    """Against fp64, relative to sum |a||b|, the f16x2 path must be as accurate as the fp32-input MFMA
    whatever the operands' magnitudes (the power-of-two scales are exact) and with a wide dynamic
    range inside an operand (small elements lose low bits only relative to the largest)."""
    rng = np.random.default_rng(1)
    M, N, K = 512, 256, 2048
    X = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-8, 8, (M, K))) * sx).astype(np.float32)
    W = (rng.standard_normal((K, N)) * np.exp(rng.uniform(-8, 8, (K, N))) * sw).astype(np.float32)
    x, w, bb = dev(X), dev(W), dev(np.zeros(N, np.float32))
    ref = X.astype(np.float64) @ W.astype(np.float64)
    mag = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)
    err = {}
    ax, aw = _amax_vec(lib, x), _amax_vec(lib, w)          # must outlive the calls: the struct holds raw pointers
    for tag, mode, ga in (("fp32", 0, None), ("f16x2", 1, _ga(ax, aw))):
        _chk(lib.mi_set_gemm_mode(mode))
        Y = torch.empty(M, N, device="cuda")
        _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y), N, M, N, K, 0, 1.0, 0, ga, _st()))
        assert torch.isfinite(Y).all()
        err[tag] = float(np.max(np.abs(Y.cpu().numpy() - ref) / mag))
    _chk(lib.mi_set_gemm_mode(1))
    assert err["fp32"] < 2e-6 and err["f16x2"] < 2e-6, err
    assert err["f16x2"] < 4 * err["fp32"] + 1e-7, err


@pytest.mark.parametrize("B,F,E,N", [(256, 26, 64, 512), (384, 4, 32, 128), (300, 26, 64, 512), (129, 5, 12, 40)])
def test_f16x2_gathered_layer1_matches_materialised_bitwise(lib, B, F, E, N):
    """Gathered layer-1 operand in f16x2 mode (whole-tile and any-shape kernels): the abs-max comes
    from the embedding kernel, the results equal the materialised operand's bit for bit."""
    rng = np.random.default_rng(B + F + E)
    vocab = rng.integers(2, 60, F)
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    table = rng.standard_normal((int(off[-1]), E)).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    K = F * E
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dY = (rng.standard_normal((B, N)) * 1e-4).astype(np.float32)
    t, fo, di, w, bb, dy = dev(table), dev(off[:-1].copy()), dev(ids), dev(W), dev(b), dev(dY)
    from mi355x_rec import _lib as L
    concat = torch.empty(B, K, device="cuda")
    arows = torch.zeros(L.AMAX_SLOTS, device="cuda")
    _chk(lib.mi_embed_fm_linear_fwd(_p(t), None, _p(fo), _p(di), B, F, E, _p(concat), K, None, None, None, _p(arows), 1, 0, _st()))
    assert float(arows.max()) == float(concat.abs().max())
    aw, ady = _amax_vec(lib, w), _amax_vec(lib, dy)
    Y0 = torch.empty(B, N, device="cuda"); Y1 = torch.empty(B, N, device="cuda")
    _chk(lib.mi_dense_fwd(_p(concat), K, _p(w), _p(bb), _p(Y0), N, B, N, K, 1, 0.9, 77, _ga(arows, aw), _st()))
    _chk(lib.mi_dense_fwd_gathered(_p(t), _p(fo), _p(di), F, E, _p(w), _p(bb), _p(Y1), N, B, N, 1, 0.9, 77,
                                   _ga(arows, aw), 0, _st()))
    assert torch.equal(Y0, Y1)
    pre = concat.cpu().numpy().astype(np.float64) @ W.astype(np.float64) + b
    ref = np.maximum(pre, 0) / np.float64(np.float32(0.9)) * dropout_mask(77, B, N, 0.9)
    assert np.max(np.abs(Y1.cpu().numpy() - ref)) / np.sqrt(np.mean(pre * pre)) < TOL
    ws = torch.empty(lib.mi_dense_bwd_weight_workspace_bytes(B, N, K) + 256, dtype=torch.uint8, device="cuda")
    dW0 = torch.empty(K, N, device="cuda"); dW1 = torch.empty(K, N, device="cuda")
    db0 = torch.empty(N, device="cuda"); db1 = torch.empty(N, device="cuda")
    _chk(lib.mi_dense_bwd_weight(_p(concat), K, _p(dy), N, _p(dW0), _p(db0), B, N, K, _p(ws), ws.numel(),
                                 _ga(arows, ady), _st()))
    _chk(lib.mi_dense_bwd_weight_gathered(_p(t), _p(fo), _p(di), F, E, _p(dy), N, _p(dW1), _p(db1), B, N, _p(ws),
                                          ws.numel(), _ga(arows, ady), 0, _st()))
    assert torch.equal(dW0, dW1) and torch.equal(db0, db1)
    ref = concat.cpu().numpy().astype(np.float64).T @ dY.astype(np.float64)
    assert np.max(np.abs(dW1.cpu().numpy() - ref)) / (np.sqrt(np.mean(ref * ref)) + 1e-30) < TOL


@pytest.mark.parametrize("name", ["Adam", "Ftrl", "Ftrl l1=0.01 l2=0.1"])
def test_sparse_apply_fused_equals_bwd_then_apply_bitwise(lib, name):
    """mi_sparse_apply_fused == mi_embed_fm_linear_bwd followed by mi_sparse_apply, bit for bit (the third case: with Ftrl's
    l1 clip and 2 * l2 term switched on)."""
    from mi355x_rec.engine import OptimizerSpec
    rng = np.random.default_rng(4)
    B, F, E = 200, 6, 16
    vocab = rng.integers(2, 15, F)                       # small vocab: many duplicates
    off = np.concatenate([[0], np.cumsum(vocab)]).astype(np.int64)
    R = int(off[-1])
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    rows = (off[:-1][None, :] + ids).reshape(-1).astype(np.int32)
    table = rng.standard_normal((R, E)).astype(np.float32)
    lin_w = rng.standard_normal(R).astype(np.float32)
    cc = table[rows].reshape(B, F * E)
    sv = cc.reshape(B, F, E).sum(1).astype(np.float32)
    dc = rng.standard_normal((B, F * E)).astype(np.float32)
    dl = rng.standard_normal(B).astype(np.float32)
    n = B * F
    r = dev(rows)
    se = torch.empty(n, dtype=torch.int32, device="cuda"); uq = torch.empty(n, dtype=torch.int32, device="cuda")
    sg = torch.empty(n + 1, dtype=torch.int32, device="cuda"); nu = torch.empty(1, dtype=torch.int32, device="cuda")
    wsb = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_rows(_p(r), n, R, _p(se), _p(uq), _p(sg), _p(nu), _p(wsb), wsb.numel(), _st()))
    spec = OptimizerSpec("Ftrl", 0.01, l1=0.01, l2=0.1) if name.startswith("Ftrl l1") else OptimizerSpec(name, 0.01)
    h = spec.hparams(0.00316)
    a, b = spec.slot_init
    res = []
    d_dc, d_cc, d_sv, d_dl = dev(dc), dev(cc), dev(sv), dev(dl)
    for fused in (False, True):
        T, L = dev(table), dev(lin_w)
        t0, t1 = torch.full_like(T, a), torch.full_like(T, b)
        l0, l1 = torch.full_like(L, a), torch.full_like(L, b)
        if fused:
            _chk(lib.mi_sparse_apply_fused(_p(T), _p(t0), _p(t1), _p(L), _p(l0), _p(l1), None, _p(uq), _p(sg), _p(se),
                                           _p(nu), n, _p(d_dc), F * E, _p(d_sv), _p(d_dl), _p(d_dl), F, E, 1,
                                           C.byref(h), 1, 0, _st()))
        else:
            d_rows = torch.empty(n, E, device="cuda"); d_lin = torch.empty(n, device="cuda")
            _chk(lib.mi_embed_fm_linear_bwd(_p(d_dc), F * E, _p(d_cc), F * E, None, _p(d_sv), _p(d_dl), _p(d_dl), None, B, F,
                                            E, _p(d_rows), _p(d_lin), _st()))
            _chk(lib.mi_sparse_apply(_p(T), _p(t0), _p(t1), _p(L), _p(l0), _p(l1), None, _p(uq), _p(sg), _p(se),
                                     _p(nu), n, _p(d_rows), _p(d_lin), E, 1, C.byref(h), 1, 0, 0, _st()))
        torch.cuda.synchronize()
        res.append((T.cpu(), L.cpu(), t0.cpu(), t1.cpu()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert not torch.equal(res[0][0], torch.from_numpy(table))


@pytest.mark.parametrize("E", [64, 4, 128])
def test_sparse_apply_long_segments(lib, E):
    """Skewed ids: a few rows own thousands of entries (a workgroup per row sums them in slices).
    SGD, so row_new = row - lr * sum(grads): checked against fp64, and run twice for reproducibility;
    rows with short segments keep the one-pass order and must match the fp32 sequential sum exactly."""
    from mi355x_rec.engine import OptimizerSpec
    rng = np.random.default_rng(E)
    n, R = 20000, 300
    p = 1.0 / np.arange(1, R + 1) ** 1.3
    rows = rng.choice(R, size=n, p=p / p.sum()).astype(np.int32)
    counts = np.bincount(rows, minlength=R)
    assert counts.max() > 2000 and (counts > 48).sum() > 10 and ((counts > 0) & (counts <= 48)).sum() > 50
    table = rng.standard_normal((R, E)).astype(np.float32)
    lin_w = rng.standard_normal(R).astype(np.float32)
    d_rows = rng.standard_normal((n, E)).astype(np.float32)
    d_lin = rng.standard_normal(n).astype(np.float32)
    r = dev(rows)
    se = torch.empty(n, dtype=torch.int32, device="cuda"); uq = torch.empty(n, dtype=torch.int32, device="cuda")
    sg = torch.empty(n + 1, dtype=torch.int32, device="cuda"); nu = torch.empty(1, dtype=torch.int32, device="cuda")
    wsb = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_rows(_p(r), n, R, _p(se), _p(uq), _p(sg), _p(nu), _p(wsb), wsb.numel(), _st()))
    h = OptimizerSpec("SGD", 0.01).hparams(0.0)
    dr, dli = dev(d_rows), dev(d_lin)
    outs = []
    for _ in range(2):
        T, L = dev(table), dev(lin_w)
        _chk(lib.mi_sparse_apply(_p(T), None, None, _p(L), None, None, None, _p(uq), _p(sg), _p(se), _p(nu), n, _p(dr),
                                 _p(dli), E, 1, C.byref(h), 1, 0, 0, _st()))
        torch.cuda.synchronize()
        outs.append((T.cpu().numpy(), L.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    g64 = np.zeros((R, E)); np.add.at(g64, rows, d_rows.astype(np.float64))
    gl64 = np.zeros(R); np.add.at(gl64, rows, d_lin.astype(np.float64))
    scale = np.sqrt(counts)[:, None] + 1.0                   # error of an fp32 sum of c terms ~ sqrt(c) ulps
    assert np.max(np.abs(outs[0][0] - (table - 0.01 * g64)) / scale) < 1e-6
    assert np.max(np.abs(outs[0][1] - (lin_w - 0.01 * gl64)) / scale[:, 0]) < 1e-6
    g32 = np.zeros((R, E), np.float32); np.add.at(g32, rows, d_rows)           # sequential fp32, ascending entry
    short = (counts > 0) & (counts <= 48)
    expect = table - np.float32(0.01) * g32
    assert np.array_equal(outs[0][0][short], expect[short])


def test_fast_sqrt_equals_sqrtf_on_every_value_in_range(lib):
    """The replay loop's square root (v_rsq_f32 + one coupled Newton step + residual correction, all packable FMAs)
    must return the bits of the correctly rounded sqrtf.  Proven by exhaustion on the device it runs on: every fp32
    value in [2^-100, 2^24] (the loop is entered with v in [2^-93, 2^20] only, decayed by at most 2^-3), ~1.04e9
    values.  The v_sqrt_f32 + one-ulp-test form round 1 used is swept alongside."""
    lo = np.array([2.0 ** -100], np.float32).view(np.uint32)[0]
    hi = np.array([2.0 ** 24], np.float32).view(np.uint32)[0]
    mism = torch.zeros(2, dtype=torch.int64, device="cuda")
    first, chunk = int(lo), 1 << 28
    while first <= int(hi):
        n = min(chunk, int(hi) - first + 1)
        _chk(lib.mi_selftest_sqrt(first, n, _p(mism), _st()))
        first += n
    torch.cuda.synchronize()
    assert mism.tolist() == [0, 0], mism.tolist()
    # and the counter does count: 0 is outside the fast form's domain (0 * inf)
    _chk(lib.mi_selftest_sqrt(0, 1, _p(mism), _st()))
    torch.cuda.synchronize()
    assert mism.tolist() == [1, 0], mism.tolist()


@pytest.mark.parametrize("d", [0.9, 0.75, 0.5, 0.8, 0.3])
def test_division_by_a_host_constant_is_the_ieee_quotient_for_every_fp32(lib, d):
    """The GEMM epilogues divide by keep_prob (tf.nn.dropout: div(x, keep_prob)) with mi_div_const (csrc/common.h): q = x r,
    e = fma(-d, q, x), fma(e, r, q) with r = RN(1 / d) from the host — Markstein's short division, 3 instructions for
    hipcc's 12.  That it returns the bits of x / d is checked on the device for ALL 2^32 bit patterns of x: no mismatch
    with 2^-100 <= |x| <= 2^100 (below, the residual of a quotient is no longer exactly representable; above, x r can
    overflow where x / d does not; an infinite activation gives NaN instead of inf)."""
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    step = 1 << 30
    for first in range(0, 1 << 32, step):
        _chk(lib.mi_selftest_div(float(np.float32(d)), first, step, _p(out), _st()))
    torch.cuda.synchronize()
    n_in, n_all = out.tolist()
    print("mi_div_const, d = %g: %d of the quotients with 2^-100 <= |x| <= 2^100 differ from '/', %d of all 2^32" % (d, n_in, n_all))
    assert n_in == 0, (n_in, n_all)
    assert n_all < (1 << 32) // 8          # (and the counter counts)


def test_catchup_exact_at_range_edges(lib):
    """mi_sparse_catchup takes an exactly rounded sqrt/divide without range scaling when a whole wave's
    values are in a safe range, hipcc's sqrtf and '/' otherwise: both must give the bits of the
    sequential fp32 sweep (numpy: IEEE sqrt and divide), for values from denormal to huge, zeros, gaps
    beyond the fast path's limit, and waves that mix both kinds of rows."""
    rng = np.random.default_rng(12)
    R, E, step_to = 4096, 64, 300
    b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-8)
    w = rng.standard_normal((R, E)).astype(np.float32)
    m = (rng.choice([-1.0, 1.0], (R, E)) * 10.0 ** rng.uniform(-30, 1, (R, E))).astype(np.float32)
    v = (10.0 ** rng.uniform(-42, 2, (R, E))).astype(np.float32)
    calm = rng.random(R) < 0.6                                   # rows well inside the fast range
    m[calm] = (rng.standard_normal((int(calm.sum()), E)) * 1e-6).astype(np.float32)
    v[calm] = (10.0 ** rng.uniform(-14, -8, (int(calm.sum()), E))).astype(np.float32)
    m[rng.random((R, E)) < 0.05] = 0.0
    v[rng.random((R, E)) < 0.05] = 0.0
    # whole waves AT the fast loop's limits (catchup_in_range: |m| in [2^-50, 2^60], v in [2^-93, 2^20], gaps <= 200), so
    # that the unscaled sqrt / divide themselves run with the smallest and the largest values they are allowed to see
    # (lr_t m down to 2^-101, its residuals down to 2^-125; v b2^k down to 2^-96) — and just outside (generic loop)
    edge = {}
    for gi, (mlo, mhi, vlo, vhi) in enumerate([(-50, -49, -93, -92), (59, 60, 19, 20), (-50, -49, 19, 20), (59, 60, -93, -92),
                                               (-51, -50, -94, -93), (-45, -44, -88, -87)]):
        rows_g = slice(64 * gi, 64 * gi + 64)
        n_g = 64
        m[rows_g] = (rng.choice([-1.0, 1.0], (n_g, E)) * 2.0 ** rng.uniform(mlo, mhi, (n_g, E))).astype(np.float32)
        v[rows_g] = (2.0 ** rng.uniform(vlo, vhi, (n_g, E))).astype(np.float32)
        edge[gi] = rows_g
    lw = rng.standard_normal(R).astype(np.float32)
    lmm = (rng.standard_normal(R) * 1e-5).astype(np.float32); lvv = (10.0 ** rng.uniform(-12, -6, R)).astype(np.float32)
    last = rng.integers(1, step_to, R).astype(np.int32)          # gaps 1 .. 299 (> 200: generic path)
    last[rng.random(R) < 0.1] = 0                                # never applied: untouched
    for gi, rows_g in edge.items():
        last[rows_g] = step_to - rng.integers(150, 201, 64)       # long replays inside the fast loop's step limit
    lr = (1e-3 * np.sqrt(1 - 0.999 ** np.arange(step_to + 1)) / np.maximum(1 - 0.9 ** np.arange(step_to + 1), 1e-30)).astype(np.float32)
    ew, em, ev = w.copy(), m.copy(), v.copy()
    elw, elm, elv = lw.copy(), lmm.copy(), lvv.copy()
    with np.errstate(all="ignore"):
        for r in range(R):
            if last[r] == 0:
                continue
            for s in range(last[r] + 1, step_to + 1):
                em[r] = em[r] * b1; ev[r] = ev[r] * b2
                ew[r] = ew[r] - (lr[s] * em[r]) / (np.sqrt(ev[r]) + eps)
                elm[r] = elm[r] * b1; elv[r] = elv[r] * b2
                elw[r] = elw[r] - (lr[s] * elm[r]) / (np.sqrt(elv[r]) + eps)
    dW, dM, dV, dL, dLm, dLv, dlast, dlr = dev(w), dev(m), dev(v), dev(lw), dev(lmm), dev(lvv), dev(last), dev(lr)
    _chk(lib.mi_sparse_catchup(_p(dW), _p(dM), _p(dV), _p(dL), _p(dLm), _p(dLv), _p(dlast), None, None, R, E, step_to,
                               _p(dlr), float(b1), float(b2), float(eps), 0, 1, 0, _st()))
    torch.cuda.synchronize()
    for got, exp in ((dW, ew), (dM, em), (dV, ev), (dL, elw), (dLm, elm), (dLv, elv)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(dlast.cpu().numpy(), np.where(last < step_to, step_to, last))


def test_bounded_catchup_stays_within_its_bound_of_the_sweep(lib):
    """MI_CATCHUP_BOUNDED (include/mi355x_rec.h): the replay with sqrt(v_j) ~ sqrtf(v_0) beta2^(j/2) and a 1-ulp reciprocal
    against the literal fp32 sweep (numpy: IEEE sqrt and divide), 150-200 replayed steps, (m, v) pairs spanning everything
    Adam can produce — gradient scales from 2^-46 (v = 2^-92) to 2^10 (v = 2^20), plus elements with m = v = 0 and rows
    never applied.  What is asserted, per variable:
        |w_bounded - w_sweep| <= 3 ulp(w) + 2e-6 * sum_j |t_j|          (t_j: the replayed updates; the analytic bound)
    and in distribution: >= 95 % of the variables bit-identical, >= 98 % within 1e-7 relative (a 1-ulp difference is by
    itself up to 1.19e-7 relative, so "1e-7 for every variable" is not a bound ANY non-bit-exact form can meet).
    m, v and the stamps must be the exact chains in both modes; with MI_CATCHUP_DEFER_SLOTS only w moves."""
    rng = np.random.default_rng(31)
    R, E, step_to = 4096, 64, 300
    f = np.float32
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    sig = 2.0 ** rng.uniform(-46, 10, (R, 1))
    sig[:256] = 2.0 ** rng.uniform(-46, -45, (256, 1))              # whole waves at the small edge ...
    sig[256:512] = 2.0 ** rng.uniform(9, 10, (256, 1))              # ... and at the large one
    v = (sig ** 2 * rng.uniform(0.2, 1.0, (R, E))).astype(f)
    m = (sig * rng.standard_normal((R, E)) * 0.5).astype(f)
    zero = rng.random((R, E)) < 0.03                                # elements whose gradient has always been 0
    m[zero] = 0.0; v[zero] = 0.0
    v[600:604, ::7] = np.inf                                        # an overflowed second moment: the sweep's update is u / inf = 0
    w = (rng.standard_normal((R, E)) * 0.3).astype(f)
    lw = (rng.standard_normal(R) * 0.3).astype(f)
    lsig = 2.0 ** rng.uniform(-46, 10, R)
    lvv = (lsig ** 2 * rng.uniform(0.2, 1.0, R)).astype(f); lmm = (lsig * rng.standard_normal(R) * 0.5).astype(f)
    last = (step_to - rng.integers(150, 201, R)).astype(np.int32)
    last[rng.random(R) < 0.05] = 0                                  # never applied: untouched
    last[rng.random(R) < 0.05] = step_to                            # up to date: untouched
    lr = (1e-3 * np.sqrt(1 - 0.999 ** np.arange(step_to + 1)) / np.maximum(1 - 0.9 ** np.arange(step_to + 1), 1e-30)).astype(f)
    ew, em, ev, moved = w.copy(), m.copy(), v.copy(), np.zeros((R, E))
    elw, elm, elv, lmoved = lw.copy(), lmm.copy(), lvv.copy(), np.zeros(R)
    with np.errstate(all="ignore"):
        for r in range(R):
            if last[r] == 0:
                continue
            for s in range(last[r] + 1, step_to + 1):
                em[r] = em[r] * b1; ev[r] = ev[r] * b2
                t = (lr[s] * em[r]) / (np.sqrt(ev[r]) + eps)
                ew[r] = ew[r] - t; moved[r] += np.abs(t)
                elm[r] = elm[r] * b1; elv[r] = elv[r] * b2
                t = (lr[s] * elm[r]) / (np.sqrt(elv[r]) + eps)
                elw[r] = elw[r] - t; lmoved[r] += abs(t)

    def check_w(got, exp, mv, what):
        worst, same, within = bounded_catchup_error(got, exp, mv, what)
        assert same >= 0.95 and within >= 0.98, (what, same, within)

    # (a) all rows, slots written (the form that runs before an evaluation / a checkpoint)
    dW, dM, dV, dL, dLm, dLv, dlast, dlr = dev(w), dev(m), dev(v), dev(lw), dev(lmm), dev(lvv), dev(last), dev(lr)
    _chk(lib.mi_sparse_catchup(_p(dW), _p(dM), _p(dV), _p(dL), _p(dLm), _p(dLv), _p(dlast), None, None, R, E, step_to,
                               _p(dlr), float(b1), float(b2), float(eps), 2, 1, 0, _st()))
    torch.cuda.synchronize()
    check_w(dW.cpu().numpy(), ew, moved, "rows")
    check_w(dL.cpu().numpy(), elw, lmoved, "wide part")
    for got, exp in ((dM, em), (dV, ev), (dLm, elm), (dLv, elv)):        # the slots: exact chains, as in the exact mode
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(dlast.cpu().numpy(), np.where(last < step_to, step_to, last))
    # (b) the rows of a batch with deferred slots (inside a train step): only w moves
    uq = rng.permutation(R)[:3000].astype(np.int32)
    dW, dM, dV, dL, dLm, dLv, dlast = dev(w), dev(m), dev(v), dev(lw), dev(lmm), dev(lvv), dev(last)
    duq, dnu = dev(np.concatenate([uq, np.zeros(96, np.int32)])), dev(np.array([3000], np.int32))
    _chk(lib.mi_sparse_catchup(_p(dW), _p(dM), _p(dV), _p(dL), _p(dLm), _p(dLv), _p(dlast), _p(duq), _p(dnu), 3096, E, step_to,
                               _p(dlr), float(b1), float(b2), float(eps), 3, 1, 0, _st()))
    torch.cuda.synchronize()
    sel = np.zeros(R, bool); sel[uq] = True
    gw, gl = dW.cpu().numpy(), dL.cpu().numpy()
    check_w(gw[sel], ew[sel], moved[sel], "rows (deferred slots)")
    check_w(gl[sel], elw[sel], lmoved[sel], "wide part (deferred slots)")
    assert np.array_equal(gw[~sel], w[~sel]) and np.array_equal(gl[~sel], lw[~sel])
    for got, exp in ((dM, m), (dV, v), (dLm, lmm), (dLv, lvv), (dlast, last)):
        assert np.array_equal(got.cpu().numpy(), exp)
    # (c) the flag is ignored where the bounded form has no meaning (eps too small to keep sqrt(v) + eps normal): the
    # exact form runs, and an unknown flag is refused
    assert lib.mi_sparse_catchup(_p(dW), _p(dM), _p(dV), None, None, None, _p(dlast), None, None, R, E, step_to, _p(dlr),
                                 float(b1), float(b2), float(eps), 8, 1, 0, _st()) != 0


@pytest.mark.parametrize("B", [1, 37, 5000])
def test_sigmoid_ce_head(lib, B):
    rng = np.random.default_rng(B)
    lin = rng.standard_normal(B).astype(np.float32) * 3
    fm = rng.standard_normal(B).astype(np.float32)
    dnn = rng.standard_normal(B).astype(np.float32)
    bias = np.array([0.25], np.float32)
    y = (rng.random(B) < 0.4).astype(np.uint8)
    a = [dev(v) for v in (lin, bias, fm, dnn, y)]
    logits = torch.empty(B, device="cuda"); loss = torch.empty(1, device="cuda"); dl = torch.empty(B, device="cuda")
    ws = torch.empty(lib.mi_head_workspace_bytes(B) + 256, dtype=torch.uint8, device="cuda")
    for scale in (1.0 / B, 1.0):
        dsum = torch.empty(1, device="cuda")
        _chk(lib.mi_sigmoid_ce_head(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), B, scale, _p(logits),
                                    _p(loss), _p(dl), _p(dsum), _p(ws), ws.numel(), _st()))
        x32 = ((lin + bias[0]) + fm) + dnn                          # the reference's summation order
        assert np.array_equal(logits.cpu().numpy(), x32)
        l64, d64, _, _ = O.head(x32.astype(np.float64), y, "mean" if scale != 1.0 else "sum")
        assert abs(loss.item() - l64) / abs(l64) < TOL
        assert max_err_scaled(dl.cpu().numpy(), d64) < TOL
        assert abs(dsum.item() - d64.sum()) < TOL * np.abs(d64).sum()
    # a term left out is skipped, not read
    _chk(lib.mi_sigmoid_ce_head(None, None, _p(a[2]), None, None, B, 1.0, _p(logits), None, None, None, None, 0,
                                _st()))
    assert np.array_equal(logits.cpu().numpy(), fm)


@pytest.mark.parametrize("U,n_groups,Rl", [(1, 1, 10), (5000, 4, 4000), (200000, 32, 50000), (70000, 7, 123457), (300, 64, 9)])
def test_route_requests_counts_runs_of_sorted_keys(lib, U, n_groups, Rl):
    """mi_route_requests: send_rows[u] = key % rows_per_rank, counts[g] = number of distinct keys of group
    g = key // rows_per_rank — from the ends of the runs of the SORTED keys (empty groups in front, in between and at the
    end; slots past *num_uniq are not looked at)."""
    rng = np.random.default_rng(U + n_groups)
    live = rng.random(n_groups) < 0.7 if n_groups > 2 else np.ones(n_groups, bool)     # some groups get no request
    if not live.any():
        live[n_groups // 2] = True
    g = rng.choice(np.flatnonzero(live), U)
    keys = np.unique(g.astype(np.int64) * Rl + rng.integers(0, Rl, U)).astype(np.int32)  # sorted, distinct
    u = len(keys)
    n_max = u + 37
    buf = np.concatenate([keys, np.full(37, 2 ** 31 - 1, np.int32)])
    dk, dn = dev(buf), dev(np.array([u], np.int32))
    send = torch.full((n_max,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((n_groups,), 12345, dtype=torch.int32, device="cuda")                 # the entry zeroes them itself
    _chk(lib.mi_route_requests(_p(dk), _p(dn), n_max, Rl, n_groups, _p(send), _p(counts), _st()))
    assert np.array_equal(send.cpu().numpy()[:u], keys % Rl) and np.all(send.cpu().numpy()[u:] == -1)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(keys // Rl, minlength=n_groups))


@pytest.mark.parametrize("world,self_rank,chunks", [(1, 0, 1), (8, -1, 1), (8, 3, 2), (4, 0, 4), (5, 4, 1)])
def test_shard_keys_number_the_asking_rank_last(lib, world, self_rank, chunks):
    """mi_shard_keys: key = ((chunk * world + pos(owner)) * rows_per_rank + local row), owner = row % world; pos is the
    rank itself (self_rank = -1) or — self_rank >= 0 — the other ranks in rank order with the asking rank LAST, so that a
    rank's requests to itself end every chunk's run (they never enter an exchange: DESIGN section 4)."""
    rng = np.random.default_rng(world * 10 + chunks)
    R, n = 100003, 4096 * chunks
    rows = rng.integers(0, R, n).astype(np.int32)
    Rl = (R + world - 1) // world
    epc = n // chunks if chunks > 1 else 0
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    _chk(lib.mi_shard_keys(_p(dev(rows)), n, world, epc, Rl, self_rank, _p(keys), _st()))
    o = rows.astype(np.int64) % world
    if self_rank >= 0:
        o = np.where(o == self_rank, world - 1, np.where(o > self_rank, o - 1, o))
    chunk = (np.arange(n) // epc) if epc else 0
    assert np.array_equal(keys.cpu().numpy(), ((chunk * world + o) * Rl + rows // world).astype(np.int32))
    assert lib.mi_shard_keys(_p(dev(rows)), n, world, epc, Rl, world, _p(keys), _st()) != 0       # self_rank outside [-1, world)


def test_entry_grads_segsum_writes_a_range_at_its_own_base(lib):
    """mi_entry_grads_segsum(out_row0): request u is written at row u - out_row0 of the out buffers — a rank's requests to
    itself are summed straight into the buffer its own apply reads.  The same range written both ways gives the same bits,
    rows outside the range are not touched, and a base past the range's start is refused."""
    rng = np.random.default_rng(77)
    B, F, E = 512, 5, 16
    n = B * F
    rows = rng.integers(0, 300, n).astype(np.int32)                 # ~300 distinct requests, segments of ~8 entries
    key = dev(rows)
    se = torch.empty(n, dtype=torch.int32, device="cuda"); uq = torch.empty(n, dtype=torch.int32, device="cuda")
    sg = torch.empty(n + 1, dtype=torch.int32, device="cuda"); nu = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.mi_sort_unique_workspace_bytes(n)) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_rows(_p(key), n, 300, _p(se), _p(uq), _p(sg), _p(nu), _p(ws), ws.numel(), _st()))
    U = int(nu.item())
    d_concat = dev(rng.standard_normal((B, F * E)).astype(np.float32))
    dl = dev(rng.standard_normal(B).astype(np.float32))
    full_r = torch.full((U, E), 7.0, device="cuda"); full_l = torch.full((U,), 7.0, device="cuda")
    _chk(lib.mi_entry_grads_segsum(None, _p(sg), _p(se), 0, U, _p(d_concat), F * E, None, None, _p(dl), 0, F, E, _p(full_r), _p(full_l), 0, 0, 0, _st()))
    u0, cnt = U // 3, U // 2
    part_r = torch.full((cnt + 2, E), 7.0, device="cuda"); part_l = torch.full((cnt + 2,), 7.0, device="cuda")
    _chk(lib.mi_entry_grads_segsum(None, _p(sg), _p(se), u0, cnt, _p(d_concat), F * E, None, None, _p(dl), 0, F, E, _p(part_r), _p(part_l), u0, 0, 0, _st()))
    assert torch.equal(part_r[:cnt], full_r[u0:u0 + cnt]) and torch.equal(part_l[:cnt], full_l[u0:u0 + cnt])
    assert float(part_r[cnt:].min()) == 7.0 and float(part_l[cnt:].min()) == 7.0
    assert lib.mi_entry_grads_segsum(None, _p(sg), _p(se), u0, cnt, _p(d_concat), F * E, None, None, _p(dl), 0, F, E, _p(part_r), _p(part_l),
                                     u0 + 1, 0, 0, _st()) != 0
    # the packed exchange's form (round 4): the rows the FM term reads and the sums it writes are records of E + 4 floats
    # [row | weight | pad]; the same bits as with separate arrays, pads untouched
    got = dev(rng.standard_normal((U, E)).astype(np.float32))
    sumv = dev(rng.standard_normal((B, E)).astype(np.float32))
    ref_r = torch.empty(U, E, device="cuda"); ref_l = torch.empty(U, device="cuda")
    _chk(lib.mi_entry_grads_segsum(_p(got), _p(sg), _p(se), 0, U, _p(d_concat), F * E, _p(sumv), _p(dl), _p(dl), 0, F, E, _p(ref_r), _p(ref_l), 0, 0, 0, _st()))
    got_rec = torch.full((U, E + 4), 3.0, device="cuda"); got_rec[:, :E] = got
    out_rec = torch.full((cnt + 1, E + 4), 7.0, device="cuda")
    _chk(lib.mi_entry_grads_segsum(_p(got_rec), _p(sg), _p(se), u0, cnt, _p(d_concat), F * E, _p(sumv), _p(dl), _p(dl), 0, F, E,
                                   _p(out_rec), out_rec.data_ptr() + 4 * E, u0, E + 4, E + 4, _st()))
    assert torch.equal(out_rec[:cnt, :E], ref_r[u0:u0 + cnt]) and torch.equal(out_rec[:cnt, E], ref_l[u0:u0 + cnt])
    assert float(out_rec[:, E + 1:].min()) == 7.0 and float(out_rec[cnt:].min()) == 7.0
    # ... and mi_sparse_apply takes gradients in that form (grad_stride): same bits as from two arrays
    from mi355x_rec.engine import OptimizerSpec
    h = OptimizerSpec("Adagrad", 0.05).hparams(0.0)
    R = 300
    outs = []
    for packed in (False, True):
        W = dev(np.linspace(-1, 1, R * E, dtype=np.float32).reshape(R, E)); A = torch.full((R, E), 0.1, device="cuda")
        L = dev(np.linspace(-1, 1, R, dtype=np.float32)); LA = torch.full((R,), 0.1, device="cuda")
        gr = dev(rng.standard_normal((n, E)).astype(np.float32)) if not packed else None
        if packed:
            grec = torch.full((n, E + 4), 9.0, device="cuda"); grec[:, :E] = g_keep; grec[:, E] = gl_keep
            pr, pl, st_ = grec.data_ptr(), grec.data_ptr() + 4 * E, E + 4
        else:
            g_keep, gl_keep = gr, dev(rng.standard_normal(n).astype(np.float32))
            pr, pl, st_ = g_keep.data_ptr(), gl_keep.data_ptr(), 0
        _chk(lib.mi_sparse_apply(_p(W), _p(A), None, _p(L), _p(LA), None, None, _p(uq), _p(sg), _p(se), _p(nu), n, pr, pl, E, 1,
                                 C.byref(h), 1, 0, st_, _st()))
        torch.cuda.synchronize()
        outs.append((W, A, L, LA))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_binary_predictions_match_oracle(lib):
    """mi_binary_predictions: get_binary_predictions / get_binary_losses (model_utils.py:9-36) per example."""
    rng = np.random.default_rng(5)
    B = 4099
    x = np.concatenate([rng.standard_normal(B - 6) * 6, [0.0, -0.0, 40.0, -40.0, 100.0, -100.0]]).astype(np.float32)
    y = (rng.random(B) < 0.4).astype(np.uint8)
    dx, dy = dev(x), dev(y)
    p = torch.empty(B, device="cuda"); pr = torch.empty(B, 2, device="cuda")
    cls = torch.empty(B, dtype=torch.int64, device="cuda"); ul = torch.empty(B, device="cuda")
    _chk(lib.mi_binary_predictions(_p(dx), _p(dy), B, _p(p), _p(pr), _p(cls), _p(ul), _st()))
    x64 = x.astype(np.float64)
    o = O.predictions(x64)
    assert np.max(np.abs(p.cpu().numpy() - o["logistic"])) < 1e-7
    assert np.array_equal(pr.cpu().numpy()[:, 1], p.cpu().numpy()) and np.max(np.abs(pr.cpu().numpy().sum(1) - 1)) < 1e-7
    assert np.array_equal(cls.cpu().numpy(), (p.cpu().numpy() > 0.5).astype(np.int64))
    near = np.abs(x) > 1e-6                                  # (class at x == 0 is p > 0.5 = False, as TF's)
    assert np.array_equal(cls.cpu().numpy()[near], o["class_id"][near]) and cls.cpu().numpy()[B - 6] == 0
    per = O.head(x64, y)[2]
    assert np.max(np.abs(ul.cpu().numpy() - per) / (1 + per)) < 1e-6
    # outputs are optional; the per-example loss needs labels
    _chk(lib.mi_binary_predictions(_p(dx), None, B, _p(p), None, None, None, _st()))
    assert lib.mi_binary_predictions(_p(dx), None, B, None, None, None, _p(ul), _st()) != 0


@pytest.mark.parametrize("n,R", [(1, 10), (100, 7), (5000, 300), (70000, 4106), (200000, 26_000_000), (4097, 65536)])
def test_sort_unique_rows(lib, n, R):
    rng = np.random.default_rng(n + R)
    rows = rng.integers(0, R, n).astype(np.int32)
    if n > 10:
        rows[n // 2:n // 2 + 5] = rows[0]
    r = dev(rows)
    se = torch.empty(n, dtype=torch.int32, device="cuda")
    uq = torch.empty(n, dtype=torch.int32, device="cuda")
    sg = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    nu = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_rows(_p(r), n, R, _p(se), _p(uq), _p(sg), _p(nu), _p(ws), ws.numel(), _st()))
    order = np.argsort(rows, kind="stable").astype(np.int32)
    assert np.array_equal(se.cpu().numpy(), order)                  # stable: bit exact
    u = np.unique(rows)
    U = int(nu.item())
    assert U == len(u)
    assert np.array_equal(uq.cpu().numpy()[:U], u)
    sr = rows[order]
    starts = np.flatnonzero(np.r_[True, sr[1:] != sr[:-1]])
    assert np.array_equal(sg.cpu().numpy()[:U + 1], np.r_[starts, n].astype(np.int32))


@pytest.mark.parametrize("n,R", [(100, 7), (4097, 300), (70000, 26_000_000)])
def test_sort_unique_rows_without_uniq_rows_is_the_permutation_alone(lib, n, R):
    """uniq_rows = NULL: only the stable sort permutation — the last pass writes straight into sorted_entry — and nothing
    else is written.  One workgroup; one pass with a partial tile; three passes."""
    rng = np.random.default_rng(n + R)
    rows = rng.integers(0, R, n).astype(np.int32)
    rows[n // 2:n // 2 + 5] = rows[0]
    r = dev(rows)
    se = torch.full((n + 128,), -7, dtype=torch.int32, device="cuda")
    sg = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    nu = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_rows(_p(r), n, R, _p(se[64:]), None, _p(sg), _p(nu), _p(ws), ws.numel(), _st()))
    assert np.array_equal(se[64:64 + n].cpu().numpy(), np.argsort(rows, kind="stable").astype(np.int32))
    assert bool((se[:64] == -7).all()) and bool((se[64 + n:] == -7).all())
    assert bool((sg == -7).all()) and int(nu.item()) == -7
    assert torch.equal(r, dev(rows))


@pytest.mark.parametrize("n,R", [(1, 10), (100, 7), (1000, 3), (5000, 300), (70000, 4106), (300000, 26_000_000), (4097, 65536)])
def test_sort_unique_rows_slots_equals_sort_then_segment_slots(lib, n, R):
    """mi_sort_unique_rows_slots = mi_sort_unique_rows + mi_segment_slots (the entry the row-sharded step's routing used until
    round 5), bit for bit: same sort outputs, and slot_of_entry[e] = the segment of entry e"""
    rng = np.random.default_rng(n + R)
    rows = rng.integers(0, R, n).astype(np.int32)
    r = dev(rows)
    def outs():
        return (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                torch.empty(n + 1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
                torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    ws = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    se, uq, sg, nu, sl = outs()
    _chk(lib.mi_sort_unique_rows_slots(_p(r), n, R, _p(se), _p(uq), _p(sg), _p(nu), _p(sl), _p(ws), ws.numel(), _st()))
    se2, uq2, sg2, nu2, sl2 = outs()
    _chk(lib.mi_sort_unique_rows(_p(r), n, R, _p(se2), _p(uq2), _p(sg2), _p(nu2), _p(ws), ws.numel(), _st()))
    _chk(lib.mi_segment_slots(_p(sg2), _p(se2), _p(nu2), n, _p(sl2), _st()))
    U = int(nu.item())
    assert U == int(nu2.item()) and torch.equal(se, se2) and torch.equal(uq[:U], uq2[:U]) and torch.equal(sg[:U + 1], sg2[:U + 1])
    assert torch.equal(sl, sl2)
    assert np.array_equal(np.unique(rows)[sl.cpu().numpy()], rows)          # the slot's row is the entry's row


@pytest.mark.parametrize("n_max,U,st", [(5000, 4100, 1), (200000, 150000, 4), (4097, 4097, 1), (70, 0, 4)])
def test_catchup_rows_by_gap_is_the_stable_sort_of_the_gap_keys(lib, n_max, U, st):
    """mi_catchup_rows_by_gap == mi_catchup_gap_keys + stable sort + gather (the three entries it replaces)"""
    rng = np.random.default_rng(n_max + U)
    R, step_to = 300000, 90
    rows = np.sort(rng.choice(R, n_max, replace=False)).astype(np.int32)
    stamps = rng.integers(0, step_to + 2, R).astype(np.int32)          # 0: never applied; >= step_to: nothing to replay
    rec = np.zeros((R, st), np.int32)
    rec[:, 0] = stamps
    r, ls, nu = dev(rows), dev(rec.reshape(-1)), dev(np.array([U], np.int32))
    out = torch.full((n_max,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mi_sort_unique_workspace_bytes(n_max) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_catchup_rows_by_gap(_p(r), _p(nu), _p(ls), n_max, step_to, st, _p(out), _p(ws), ws.numel(), _st()))
    keys = torch.empty(n_max, dtype=torch.int32, device="cuda")
    _chk(lib.mi_catchup_gap_keys(_p(r), _p(nu), _p(ls), n_max, step_to, _p(keys), st, _st()))
    s_ = stamps[rows[:U]]
    want_keys = np.full(n_max, 63, np.int32)
    want_keys[:U] = np.where((s_ > 0) & (s_ < step_to), np.minimum(step_to - s_, 62), 0)
    assert np.array_equal(keys.cpu().numpy(), want_keys)
    order = np.argsort(want_keys, kind="stable")
    assert np.array_equal(out.cpu().numpy()[:U], rows[order][:U])


@pytest.mark.parametrize("beside", [0, 1])
@pytest.mark.parametrize("B,F,vocab", [(4096, 26, 1_000_000), (8192, 3, 50), (4096, 40, 1_250_000), (4096, 1, 7), (65536, 26, 1_000_000),
                                       (65536, 5, -1_000_000), (12288, 64, 3_000_000)])
def test_sort_unique_fields_equals_global_rows_then_sort(lib, B, F, vocab, beside):
    """the per-field (segmented) sort gives the outputs of mi_global_rows + mi_sort_unique_rows bit for bit — in both of its
    forms (beside = 0: one launch per radix pass, the tiles of a field exchanging their digit counts inside it, and one for the
    compaction; beside = 1: the 14 short launches), up to config 3's full size, with Zipf-skewed ids (vocab < 0: most of a
    field's entries share a few rows, segments of thousands) and with more than 2^20 ids per field (3 passes)"""
    rng = np.random.default_rng(B + F)
    zipf, vocab = vocab < 0, abs(vocab)
    vs = [max(2, vocab - 13 * f) for f in range(F)]
    if zipf:
        ids = np.stack([np.minimum(rng.zipf(1.05, B) - 1, v - 1) for v in vs], 1).astype(np.int32)
    else:
        ids = np.stack([rng.integers(0, v, B) for v in vs], 1).astype(np.int32)
    ids[B // 2] = ids[0]                                   # duplicates across examples
    if F > 1:
        ids[:, 1] = ids[0, 1] if B < 5000 else ids[:, 1]   # a field with ONE id: a segment of B duplicates
    off = np.zeros(F, np.int64); off[1:] = np.cumsum(vs)[:-1]
    n = B * F
    d_ids, d_off = dev(ids), dev(off)
    def outs():
        return (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                torch.empty(n + 1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
    se, uq, sg, nu = outs()
    ws = torch.empty(lib.mi_sort_unique_fields_workspace_bytes(B, F) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_fields(_p(d_ids), _p(d_off), B, F, max(vs), _p(se), _p(uq), _p(sg), _p(nu), _p(ws), ws.numel(), beside, _st()))
    rows = torch.empty(n, dtype=torch.int32, device="cuda")
    _chk(lib.mi_global_rows(_p(d_ids), _p(d_off), B, F, _p(rows), _st()))
    se2, uq2, sg2, nu2 = outs()
    ws2 = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_sort_unique_rows(_p(rows), n, int(sum(vs)), _p(se2), _p(uq2), _p(sg2), _p(nu2), _p(ws2), ws2.numel(), _st()))
    U = int(nu2.item())
    assert int(nu.item()) == U
    assert torch.equal(se, se2)
    assert torch.equal(uq[:U], uq2[:U]) and torch.equal(sg[:U + 1], sg2[:U + 1])
    assert lib.mi_sort_unique_fields(_p(d_ids), _p(d_off), B - 1, F, max(vs), _p(se), _p(uq), _p(sg), _p(nu), _p(ws), ws.numel(), beside, _st()) != 0


def test_colsum_and_layer_stats(lib):
    rng = np.random.default_rng(3)
    M, N = 3000, 70
    X = np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32)
    x = dev(X)
    out = torch.empty(N, device="cuda")
    ws = torch.empty(lib.mi_colsum_workspace_bytes(M, N) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_colsum(_p(x), N, M, N, _p(out), _p(ws), ws.numel(), _st()))
    assert max_err_scaled(out.cpu().numpy(), X.astype(np.float64).sum(0)) < TOL
    o4 = torch.empty(4, device="cuda")
    ws = torch.empty(lib.mi_layer_stats_workspace_bytes(M * N) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_layer_stats(_p(x), M * N, _p(o4), _p(ws), ws.numel(), _st()))
    s = O.layer_summary(X)
    g = o4.cpu().numpy()
    assert abs(g[0] - s["fraction_of_zero_values"]) < 1e-6 and g[1] == s["min"] and g[2] == s["max"]
    assert abs(g[3] - s["mean"]) < 1e-5


def _hp(lib, spec, lr_t=0.0):
    from mi355x_rec.engine import OptimizerSpec
    return OptimizerSpec(**spec).hparams(lr_t)


@pytest.mark.parametrize("name", OO.NAMES)
def test_dense_apply_bit_exact(lib, name):
    rng = np.random.default_rng(11)
    n = 1000
    hp = OO.Hyper(name, lr=0.05 if name != "Adam" else 0.001)
    w = rng.standard_normal(n).astype(np.float32)
    s0, s1 = OO.slot_init(hp, w)
    s0 = s0.copy(); s1 = s1.copy()
    dw, d0, d1 = dev(w), dev(s0), dev(s1)
    powers = OO.AdamPowers(hp, np.float32) if name == "Adam" else None
    from mi355x_rec.engine import OptimizerSpec
    spec = OptimizerSpec(name, hp.lr)
    for step in range(3):
        g = rng.standard_normal(n).astype(np.float32)
        lr_t = powers.lr_t(hp.lr) if powers else 0.0
        OO.dense_apply(hp, w, s0, s1, g, lr_t)
        if powers:
            powers.finish()
        h = spec.hparams(float(lr_t))
        dg = dev(g)          # keep a reference: the launch is asynchronous
        _chk(lib.mi_dense_apply(_p(dw), _p(d0) if name != "SGD" else None,
                                _p(d1) if name in ("Adam", "Ftrl", "RMSProp") else None, _p(dg), n,
                                C.byref(h), _st()))
        torch.cuda.synchronize()
    assert np.array_equal(dw.cpu().numpy(), w)
    if name != "SGD":
        assert np.array_equal(d0.cpu().numpy(), s0)
    if name in ("Adam", "Ftrl", "RMSProp"):                # v, linear, mom (RMSProp's stays 0 at the default momentum)
        assert np.array_equal(d1.cpu().numpy(), s1)
        assert s1.any() or name == "RMSProp"


@pytest.mark.parametrize("layout", ["arrays", "records"])
@pytest.mark.parametrize("name", OO.NAMES)
@pytest.mark.parametrize("E", [4, 64])
def test_sparse_apply_and_catchup_bit_exact(lib, name, E, layout):
    """Sparse apply (+ for Adam the lazy catch-up) against the oracle's TF rule — for Adam that is
    the literal whole-table sweep of adam.py _apply_sparse_shared, so equality here shows that
    lazy catch-up == sweep, bit for bit, including rows that sit out several steps.
    layout "records" (round 4, what the engine allocates): one [w | slot0 | slot1] record per row, the three pointers E
    floats apart and table_stride = 3 E; "arrays": three [R, E] arrays (table_stride 0)."""
    from mi355x_rec.engine import OptimizerSpec, AdamSchedule
    rng = np.random.default_rng(E)
    R, steps = 50, 7
    hp = OO.Hyper(name, lr=0.05 if name != "Adam" else 0.001)
    spec = OptimizerSpec(name, hp.lr)
    W = rng.standard_normal((R, E)).astype(np.float32)
    L = rng.standard_normal((R, 1)).astype(np.float32)
    ws0, ws1 = [a.copy() for a in OO.slot_init(hp, W)]
    ls0, ls1 = [a.copy() for a in OO.slot_init(hp, L)]
    dW, dL = dev(W), dev(L[:, 0].copy())
    d_ws0, d_ws1, d_ls0, d_ls1 = dev(ws0), dev(ws1), dev(ls0[:, 0].copy()), dev(ls1[:, 0].copy())
    tst = 0
    if layout == "records":
        rec = torch.full((R, 3 * E), float("nan"), device="cuda")
        rec[:, :E] = dW; rec[:, E:2 * E] = d_ws0; rec[:, 2 * E:] = d_ws1
        dW, d_ws0, d_ws1, tst = rec[:, :E], rec[:, E:2 * E], rec[:, 2 * E:], 3 * E
    last = torch.zeros(R, dtype=torch.int32, device="cuda")
    powers = OO.AdamPowers(hp, np.float32) if name == "Adam" else None
    sched = AdamSchedule(spec, "cuda", 64) if name == "Adam" else None
    need0, need1 = name != "SGD", name in ("Adam", "Ftrl", "RMSProp")
    for step in range(1, steps + 1):
        n = 40
        rows = rng.integers(0, R // 2 if step % 2 else R, n).astype(np.int32)   # some rows sit out
        rows[5] = rows[0]; rows[6] = rows[0]
        g = rng.standard_normal((n, E)).astype(np.float32)
        gl = rng.standard_normal((n, 1)).astype(np.float32)
        lr_t = powers.lr_t(hp.lr) if powers else 0.0
        OO.sparse_apply(hp, W, ws0, ws1, rows, g, lr_t)
        OO.sparse_apply(hp, L, ls0, ls1, rows, gl, lr_t)
        if powers:
            powers.finish()
        r = dev(rows)
        se = torch.empty(n, dtype=torch.int32, device="cuda"); uq = torch.empty(n, dtype=torch.int32, device="cuda")
        sg = torch.empty(n + 1, dtype=torch.int32, device="cuda"); nu = torch.empty(1, dtype=torch.int32, device="cuda")
        wsb = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
        _chk(lib.mi_sort_unique_rows(_p(r), n, R, _p(se), _p(uq), _p(sg), _p(nu), _p(wsb), wsb.numel(), _st()))
        if name == "Adam" and step > 1:
            assert abs(sched.lr_t(step) - float(lr_t)) == 0.0
            _chk(lib.mi_sparse_catchup(_p(dW), _p(d_ws0), _p(d_ws1), _p(dL), _p(d_ls0), _p(d_ls1), _p(last), _p(uq),
                                       _p(nu), n, E, step - 1, _p(sched.table), hp.beta1, hp.beta2, hp.epsilon, 0, 1, tst, _st()))
        h = spec.hparams(float(lr_t))
        dg, dgl = dev(g), dev(gl[:, 0].copy())      # keep references: launches are asynchronous
        _chk(lib.mi_sparse_apply(_p(dW), _p(d_ws0) if need0 else None, _p(d_ws1) if need1 else None, _p(dL),
                                 _p(d_ls0) if need0 else None, _p(d_ls1) if need1 else None,
                                 _p(last) if name == "Adam" else None, _p(uq), _p(sg), _p(se), _p(nu), n,
                                 _p(dg), _p(dgl), E, step, C.byref(h), 1, tst, 0, _st()))
        torch.cuda.synchronize()
    if name == "Adam":   # bring the rows that sat out the last steps up to date: all-rows catch-up
        _chk(lib.mi_sparse_catchup(_p(dW), _p(d_ws0), _p(d_ws1), _p(dL), _p(d_ls0), _p(d_ls1), _p(last), None, None,
                                   R, E, steps, _p(sched.table), hp.beta1, hp.beta2, hp.epsilon, 0, 1, tst, _st()))
        assert np.all(last.cpu().numpy() == steps)
    assert np.array_equal(dW.cpu().numpy(), W)
    assert np.array_equal(dL.cpu().numpy(), L[:, 0])
    if need0:
        assert np.array_equal(d_ws0.cpu().numpy(), ws0)
    if need1:
        assert np.array_equal(d_ws1.cpu().numpy(), ws1)


def test_eval_accumulate_matches_metrics_oracle(lib):
    from oracle.metrics import BinaryMetrics
    rng = np.random.default_rng(2)
    hist = torch.zeros(2 * 201, dtype=torch.int64, device="cuda")
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    bm = BinaryMetrics()
    for B in (1000, 37):
        x = (rng.standard_normal(B) * 2).astype(np.float32)
        x[:3] = [0.0, 30.0, -30.0]
        y = (rng.random(B) < 0.3).astype(np.uint8)
        bm.update(x, y)
        dx, dy = dev(x), dev(y)
        _chk(lib.mi_eval_accumulate(_p(dx), _p(dy), B, _p(hist), _p(counts), _p(sums), _st()))
        torch.cuda.synchronize()
    from mi355x_rec.metrics import metrics_from_counters
    got = metrics_from_counters(hist.cpu().numpy(), counts.cpu().numpy(), sums.cpu().numpy())
    ref = bm.result()
    for k in ref:
        assert abs(got[k] - ref[k]) < 1e-6, (k, got[k], ref[k])


@pytest.mark.parametrize("M,N,K", [(512, 256, 512), (300, 40, 104)])
def test_gemm_entries_row_relative_error_with_rows_far_below_the_matrix_absmax(lib, M, N, K):
    """VERDICT r1 / ADVICE r1: rows of X / dY 2^-16 ... 2^-24 below the matrix abs-max (the dY rows of well-fit
    examples) must keep fp32-level accuracy RELATIVE TO THEIR OWN NORM in the forward pass and the data
    gradient — a matrix-wide fp16 scale loses their low bits (round 1: 8e-6 at 2^-20, 1.4e-4 at 2^-24).  The
    any-shape entries therefore never take the matrix-wide f16x2 split for these two products (bf16x3: no scale);
    the weight gradient does (its reduction runs over the examples: a tiny row's error is tiny in every dW row)."""
    rng = np.random.default_rng(M + K)
    scale = np.exp2(-rng.integers(16, 25, M)).astype(np.float32)
    scale[: M // 8] = 1.0                                            # some rows at full scale
    X = (rng.standard_normal((M, K)).astype(np.float32)) * scale[:, None]
    dY = (rng.standard_normal((M, N)).astype(np.float32)) * scale[:, None]
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    x, w, dy, bb = dev(X), dev(W), dev(dY), dev(np.zeros(N, np.float32))
    ax, aw, ady = _amax_vec(lib, x), _amax_vec(lib, w), _amax_vec(lib, dy)

    def rowrel(got, ref):
        rms = np.sqrt(np.mean(ref * ref, 1))
        return float((np.abs(got - ref).max(1) / rms).max())

    _chk(lib.mi_set_gemm_mode(1))
    Y = torch.empty(M, N, device="cuda")
    _chk(lib.mi_dense_fwd(_p(x), K, _p(w), _p(bb), _p(Y), N, M, N, K, 0, 1.0, 0, _ga(ax, aw), _st()))
    assert rowrel(Y.cpu().numpy().astype(np.float64), X.astype(np.float64) @ W.astype(np.float64)) < TOL
    dX = torch.empty(M, K, device="cuda")
    _chk(lib.mi_dense_bwd_data(_p(dy), N, _p(w), None, K, _p(dX), K, M, N, K, 1.0, 1, _ga(ady, aw), _st()))
    assert rowrel(dX.cpu().numpy().astype(np.float64), dY.astype(np.float64) @ W.astype(np.float64).T) < TOL
    ws = torch.empty(lib.mi_dense_bwd_weight_workspace_bytes(M, N, K) + 256, dtype=torch.uint8, device="cuda")
    dW = torch.empty(K, N, device="cuda"); db = torch.empty(N, device="cuda")
    _chk(lib.mi_dense_bwd_weight(_p(x), K, _p(dy), N, _p(dW), _p(db), M, N, K, _p(ws), ws.numel(), _ga(ax, ady), _st()))
    assert rowrel(dW.cpu().numpy().astype(np.float64), X.astype(np.float64).T @ dY.astype(np.float64)) < TOL


def test_layer_histogram_matches_tensorflow_bucketing(lib):
    """the histogram half of layer_summary (model_utils.py:6): TensorFlow's default limits, upper_bound bucketing"""
    from mi355x_rec.metrics import histogram_limits, histogram_proto
    rng = np.random.default_rng(3)
    x = np.concatenate([np.maximum(rng.standard_normal(50000), 0), -np.abs(rng.standard_normal(777)) * 1e-5, [0.0, 1e-13, 3e19]]).astype(np.float32)
    lim = histogram_limits()
    assert len(lim) == 1551 and lim[775] == 0.0 and np.all(np.diff(lim) > 0)
    counts = torch.zeros(len(lim) + 1, dtype=torch.int64, device="cuda")
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    dx, dl = dev(x), dev(lim)
    _chk(lib.mi_layer_histogram(_p(dx), len(x), _p(dl), len(lim), _p(counts), _p(sums), _st()))
    ref = np.bincount(np.searchsorted(lim, x.astype(np.float64), side="right"), minlength=len(lim) + 1)
    assert np.array_equal(counts.cpu().numpy(), ref)
    assert abs(sums[0].item() - x.astype(np.float64).sum()) < 1e-6 * np.abs(x).sum()
    assert abs(sums[1].item() - (x.astype(np.float64) ** 2).sum()) < 1e-6 * (x.astype(np.float64) ** 2).sum()
    pr = histogram_proto(lim, counts.cpu().numpy(), sums.cpu().numpy(), x.min(), x.max())
    assert pr["num"] == len(x) and sum(pr["bucket"]) == len(x) and len(pr["bucket"]) == len(pr["bucket_limit"]) < 400


# ---- the numeric columns' backward kernels, as kernels ----------------------------------------------------------------------
# (B = 255 / 256 / 257: around one block of 256 examples; 65536 with 13 columns is BASELINE config 4's call.)  Inputs are made
# on the device and the fp64 reference is torch's, so that the largest case costs no host time.  Bar: 1e-5 of the rms of the
# exact result; the same measure for a plain fp32 sum (torch, fp32) is printed beside it (pytest -s).
# x and d_logit_lin are head-like rather than zero-mean — values around 0.5, (sigmoid(z) - y) / B with a quarter of the labels 1 —
# because dw_num of ONE column is one number whose "rms" is its own magnitude: a zero-mean sum over the examples lands
# arbitrarily near 0 and the ratio then measures the draw, not the kernel.
NUMERIC_B = [1, 255, 256, 257, 65536]


def _numeric_inputs(g, B, nd):
    x = torch.randn(B, nd, device="cuda", generator=g) + 0.5
    z = torch.randn(B, device="cuda", generator=g)
    y = (torch.rand(B, device="cuda", generator=g) < 0.25).float()
    return x, (torch.sigmoid(z) - y) / B


def _rms_rel(got, ref):
    got, ref = got.double(), ref.double()
    rms = float(ref.pow(2).mean().sqrt())
    err = float((got - ref).abs().max())
    if rms == 0:
        assert err == 0
        return 0.0
    return err / rms


@pytest.mark.parametrize("nd", [1, 13])
@pytest.mark.parametrize("B", NUMERIC_B)
def test_numeric_raw_bwd_against_fp64(lib, B, nd):
    """dw_num[j] = sum_b d_logit_lin[b] x[b, j]: exact workspace between guard bytes, twice the same bits (fixed order)"""
    g = torch.Generator(device="cuda"); g.manual_seed(B * 31 + nd)
    x, dll = _numeric_inputs(g, B, nd)
    wbuf, ws = exact_workspace(lib.mi_numeric_raw_bwd_workspace_bytes(B, nd))
    outs = []
    for _ in range(2):
        og, dw = guarded_nan(nd)
        _chk(lib.mi_numeric_raw_bwd(x.data_ptr(), dll.data_ptr(), B, nd, dw.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
        torch.cuda.synchronize()
        assert guards_intact(og) and workspace_surroundings_intact(wbuf, ws)
        outs.append(dw.clone())
    ref = (dll.double()[:, None] * x.double()).sum(0)
    err, e32 = _rms_rel(outs[0], ref), _rms_rel((dll[:, None] * x).sum(0), ref)
    print("NUMERIC raw   B=%-6d n_d=%-2d        dw_num %.2e (plain fp32 %.2e)" % (B, nd, err, e32))
    assert bool(torch.isfinite(outs[0]).all()) and err < TOL
    assert torch.equal(outs[0], outs[1])
    assert lib.mi_numeric_raw_bwd(x.data_ptr(), dll.data_ptr(), B, nd, dw.data_ptr(), ws.data_ptr(), ws.numel() - 1, _st()) != 0


@pytest.mark.parametrize("parts", ["all", "no-d_concat", "no-d_logit_fm", "no-d_logit_lin", "no-dw_num"])
@pytest.mark.parametrize("E", [4, 12, 64, 128])
@pytest.mark.parametrize("nd", [1, 13])
@pytest.mark.parametrize("B", NUMERIC_B)
def test_numeric_embed_bwd_against_fp64(lib, B, nd, E, parts):
    """dV[j, e] = sum_b x[b, j] (d_concat[b, col0 + j E + e] + d_logit_fm[b] (sumv[b, e] - concat[b, col0 + j E + e])) and
    dw_num[j] = sum_b d_logit_lin[b] x[b, j], with each optional input absent in turn; the numeric block sits behind one
    categorical field's columns (col0 = E) in padded leading dimensions."""
    g = torch.Generator(device="cuda"); g.manual_seed(B * 131 + nd * 17 + E)
    col0, ld, lddc = E, (1 + nd) * E + 8, (1 + nd) * E + 4
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    x, dlogit = _numeric_inputs(g, B, nd)
    concat, sumv = r(B, ld), r(B, E)
    d_concat = r(B, lddc) / B if parts != "no-d_concat" else None
    dlf = dlogit if parts != "no-d_logit_fm" else None
    dll = dlogit.clone() if parts != "no-d_logit_lin" else None
    want_dw = parts != "no-dw_num"
    wbuf, ws = exact_workspace(lib.mi_numeric_embed_bwd_workspace_bytes(B, nd, E))
    outs = []
    for _ in range(2):
        vg, dV = guarded_nan(nd, E); wg, dw = guarded_nan(nd)
        _chk(lib.mi_numeric_embed_bwd(x.data_ptr(), _p(d_concat), lddc, concat.data_ptr(), ld, col0, sumv.data_ptr(), _p(dlf),
                                      _p(dll), B, nd, E, dV.data_ptr(), dw.data_ptr() if want_dw else None, ws.data_ptr(),
                                      ws.numel(), _st()))
        torch.cuda.synchronize()
        assert guards_intact(vg) and guards_intact(wg) and workspace_surroundings_intact(wbuf, ws)
        assert want_dw or bool(torch.isnan(dw).all())
        outs.append((dV.clone(), dw.clone()))

    def exact(dt):
        blk = lambda t, w: t[:, col0:col0 + nd * E].to(dt).reshape(B, nd, E)
        gv = torch.zeros(B, nd, E, dtype=dt, device="cuda")
        if d_concat is not None:
            gv = gv + blk(d_concat, lddc)
        if dlf is not None:
            gv = gv + dlf.to(dt)[:, None, None] * (sumv.to(dt)[:, None, :] - blk(concat, ld))
        dV = (x.to(dt)[:, :, None] * gv).sum(0)
        dw = (dll.to(dt)[:, None] * x.to(dt)).sum(0) if dll is not None else torch.zeros(nd, dtype=dt, device="cuda")
        return dV, dw
    (rV, rw), (fV, fw) = exact(torch.float64), exact(torch.float32)
    eV, eV32 = _rms_rel(outs[0][0], rV), _rms_rel(fV, rV)
    line = "NUMERIC embed B=%-6d n_d=%-2d E=%-3d %-14s dV %.2e (plain fp32 %.2e)" % (B, nd, E, parts, eV, eV32)
    assert bool(torch.isfinite(outs[0][0]).all()) and eV < TOL, line
    if want_dw:
        ew, ew32 = _rms_rel(outs[0][1], rw), _rms_rel(fw, rw)
        line += "  dw_num %.2e (plain fp32 %.2e)" % (ew, ew32)
        assert bool(torch.isfinite(outs[0][1]).all()) and ew < TOL, line
        assert torch.equal(outs[0][1], outs[1][1])
    print(line)
    assert torch.equal(outs[0][0], outs[1][0])
