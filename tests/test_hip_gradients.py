"""-m gpu: the gradients of ONE train step on the planes path (engine._backward_dense as the benchmark runs it) against
the oracle's own backward in fp64.

What is read: every dense gradient (DeepFM.d_grad: kernels, biases, linear bias, numeric embeddings, numeric linear
weights), the gradient of the concat (_ws["dact0"]), sumv and dlogit.  The embedding-row gradients need no comparison of
their own: test_embed_bwd_entries (test_hip_kernels.py) holds the entry kernel to the oracle GIVEN d_concat, sumv and
dlogit, and test_sparse_apply_fused_equals_bwd_then_apply_bitwise ties the fused sparse apply to that kernel — a correct
d_concat, sumv and dlogit is what was missing, and that is what is compared here.

Why one step and raw gradients: Adam's update is m / (sqrt(v) + eps), lr * sign(g) after one step — a gradient wrong by a
constant factor (a power of two from a mishandled row or matrix exponent) cancels exactly in every Adam trajectory test.

Measures.  Dense variables: max |g - ref| / rms(ref).  d_concat: test_hip_planes.row_rel_err (per example, relative to
that example's own rms).  Bars: max(1e-5, 4 x E32), where E32 is the SAME measure for the oracle's fp32 backward (numpy, same
inputs, same relu / dropout masks) against its fp64 one — the reference at the precision the kernels claim; the factor 4
is the headroom the project's "fp32-level" GEMM tests give over a plain fp32 product.  E32 never comes from the device.
Every figure is printed (pytest -s): variable, device error, fp32-oracle error, bar.

Relu decisions are the device's (read back after the step, handed to oracle.forward(relu_masks=...)); they may differ from
the fp64 oracle's own sign test only where the fp64 pre-activation is within 1e-6 of 0 — asserted.  Dropout masks are
replayed on the host (tests.util.dropout_mask)."""
import time

import numpy as np
import pytest
import torch

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import _hip_engine
from tests.util import (_compare_vars, _device_relu_masks, dev, dropout_mask, make_problem, planned_splits,
                        row_rel_err)

pytestmark = pytest.mark.gpu

SEED = 319                                                   # test_hip_model.CONFIG3_SAFE_SEED's problem
VOCAB3 = [40 + 3 * i for i in range(26)]                     # config 3's 26 fields, small vocabularies


def _rms_err(got, ref):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / (np.sqrt(np.mean(ref * ref)) + 1e-300))


def _bar(e32):
    return max(1e-5, 4.0 * e32)


def _report(case, name, err, e32):
    print("GRAD %-34s %-12s device %.2e  fp32-oracle %.2e  bar %.2e%s" % (
        case, name, err, e32, _bar(e32), "  (second term)" if err >= 1e-5 else ""))


def _merged(m, name, B, K):
    out = torch.empty(B, K, device="cuda")
    m.k.mi_merge_rows(m._pl[name].struct, B, K, out, K)
    return out


def _top_fused(m):
    return getattr(m, "_top_step", None) == m.step - 1


def _relu_masks(m, B):
    """_device_relu_masks, and for a last hidden layer that ran inside the fused logits + head launch (its output never
    reaches memory) the units whose gradient that launch let through: dY of that layer is dlogit * w masked, and neither
    factor is 0 here — checked by the caller's assertion that a decision differs from the fp64 sign test only within 1e-6
    of 0, which an unexplained zero would fail."""
    masks = _device_relu_masks(m, B)
    if _top_fused(m):
        nh = len(m.hidden)
        assert bool((m._ws["dlogit"][:B] != 0).all())
        masks[nh - 1] = (_merged(m, "dy%dp" % (nh - 1), B, m.hidden[-1]) != 0).cpu().numpy()
    return masks


def _dense_grads(m):
    """name -> device gradient, in oracle.Params.dense_list() order (kernel_0 without its zero pad rows, which must have
    got exactly zero gradients)"""
    g = m.d_grad
    out = []
    for i in range(len(m.layers)):
        k = m.kernel(i, g)
        if i == 0 and m.D_in < m.D:
            assert float(k[m.D_in:].abs().max()) == 0.0
            k = k[:m.D_in]
        out += [("kernel_%d" % i, k.cpu().numpy()), ("bias_%d" % i, m.bias(i, g).cpu().numpy())]
    out.append(("lin_bias", g[m.lin_bias_off:m.lin_bias_off + 1].cpu().numpy()))
    if m.num_emb_off is not None:
        out.append(("num_emb", m._seg(g, m.num_emb_off, (m.n_numeric, m.E)).cpu().numpy()))
    if m.lin_num_off is not None:
        out.append(("dw_num", g[m.lin_num_off:m.lin_num_off + m.n_numeric].cpu().numpy()))
    return out


def _oracle_grads(p, ids, x, y, dt, masks, drop, keep, flags, numeric, reduction):
    q = p.astype(dt)
    xx = None if x is None else x.astype(dt)
    c = O.forward(q, ids, xx, *flags, dropout_masks=drop, numeric=numeric, keep_prob=keep, relu_masks=masks)
    loss, dlogit, _, _ = O.head(c["logits"], y, reduction)
    dense, _, _ = O.backward(q, c, dlogit, drop)
    nh = len(q.mlp) - 1
    # d loss / d concat as the MLP sees it (the engine's dact0): backward() folds it into the row gradients
    d = dlogit[:, None] * q.mlp[nh][0][:, 0][None, :]
    for i in range(nh - 1, -1, -1):
        if drop is not None:
            d = (d * drop[i].astype(dt)) / dt(keep)
        d = (d * masks[i].astype(dt)) @ q.mlp[i][0].T
    return dict(dense=dense, d_concat=d, dlogit=dlogit, sumv=c.get("sumv"), pre=c["pre"], loss=float(loss),
                logits=c["logits"])


def _check_masks(masks, pre64, drop):
    """the device's relu decisions against the fp64 sign test: they may differ only on marginal units"""
    flips = 0
    for i, (mk, q) in enumerate(zip(masks, pre64)):
        own = q > 0
        if drop is not None:
            own &= drop[i] > 0                  # (a dropped unit's stored activation is 0: its mask bit is off)
        diff = mk != own
        flips += int(diff.sum())
        assert not diff.any() or float(np.abs(q[diff]).max()) < 1e-6, (i, int(diff.sum()), float(np.abs(q[diff]).max()))
    return flips


def _check_amax_chain(m, B):
    """Every abs-max vector the weight gradients consume (x<i>, dy<i> of each hidden layer) against the matrix it
    describes: same binary exponent as the true abs-max, and not below it by more than the planes' own rounding (2^-20
    relative).  A stale, unzeroed or undersized vector fails here.  dY in fp32 where this step wrote it (need_f), as
    planes (merged) otherwise; activations from the planes the GEMMs read."""
    nh = len(m.hidden)
    for i in range(nh):
        fan, h = m.layers[i][2], m.layers[i][3]
        x_true = float(_merged(m, "x%dp" % i, B, fan).abs().max())
        # dact<i+1> = dY of layer i in fp32: written when the layer above is the fused tail / gemv and this layer's weight
        # gradient reads fp32, or when the data gradient above could not write planes straight (see _backward_dense)
        if i == nh - 1:
            need_f = not m._wgrad_planes_ok(B, i)
        else:
            need_f = not (h <= 512 and m._wgrad_planes_ok(B, i))
        if need_f:
            dy_true = float(m._ws["dact%d" % (i + 1)][:B * h].abs().max())
        else:
            dy_true = float(_merged(m, "dy%dp" % i, B, h).abs().max())
        for name, true in (("x%d" % i, x_true), ("dy%d" % i, dy_true)):
            assert name in m._amax_idx, name
            got = float(m._av(name).max())
            assert true > 0 and np.isfinite(true), (name, true)
            assert np.frexp(got)[1] == np.frexp(true)[1], (name, got, true)
            assert got >= true * (1 - 2.0 ** -20), (name, got, true)


def _one_step(case, vocab, E, hidden, B, nn=0, numeric="embed", dropout=0.0, flags=(True, True, True), reduction="mean",
              prepare=None, expect_planes=True, small_rows_may_vanish=None):
    """One train_step of an engine loaded with oracle parameters; every gradient against the fp64 oracle.  Returns the engine."""
    if numeric == "embed":
        p, ids, x, y = make_problem(SEED, vocab, E, hidden, B, n_numeric=nn)
    else:
        rng = np.random.default_rng(SEED)
        p = O.init_params(rng, vocab, E, hidden, n_numeric=nn, dtype=np.float32, lin_scale=0.05, numeric=numeric)
        p.lin_bias[:] = 0.1
        for _, b in p.mlp:
            b[:] = (rng.standard_normal(b.shape) * 0.05).astype(np.float32)
        ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
        ids[B // 2] = ids[0]
        x = rng.standard_normal((B, nn)).astype(np.float32)
        y = (rng.random(B) < 0.3).astype(np.uint8)
    if prepare is not None:
        y = prepare(p, ids, x, y)
    m = _hip_engine(vocab, E, hidden, nn, gemm="f16x2", numeric=numeric, dropout=dropout, seed=7, reduction=reduction,
                use_linear=flags[0], use_mf=flags[1], use_dnn=flags[2])
    assert bool(m.planes) == expect_planes
    m.load_oracle_params(p)
    keep = 1.0 - dropout
    drop = [dropout_mask(m._layer_seed(i), B, h, keep) for i, h in enumerate(hidden)] if dropout else None   # (step 0's seeds)
    loss_g, logit_g = m.train_step(dev(ids), dev(y), dev(x))
    torch.cuda.synchronize()
    # Nothing in _apply writes d_grad unless variables are frozen (deep_numeric / wide_numeric column subsets: none here),
    # so the gradients of the step survive it.  A buffer nobody filled must not pass: finite and non-zero.
    assert m._frozen is None
    assert bool(torch.isfinite(m.d_grad).all()) and float(m.d_grad.abs().max()) > 0
    masks = _relu_masks(m, B)
    t0 = time.perf_counter()
    r64 = _oracle_grads(p, ids, x, y, np.float64, masks, drop, keep, flags, numeric, reduction)
    r32 = _oracle_grads(p, ids, x, y, np.float32, masks, drop, keep, flags, numeric, reduction)
    host_s = time.perf_counter() - t0
    flips = _check_masks(masks, r64["pre"], drop)
    print("GRAD %-34s B=%d  oracle fp64 + fp32 on the host: %.1f s, marginal relu decisions taken from the device: %d, "
          "top layer fused: %s" % (case, B, host_s, flips, _top_fused(m)))
    assert abs(loss_g.item() - r64["loss"]) <= 1e-5 * abs(r64["loss"])
    failures = []

    def hold(name, err, e32):
        _report(case, name, err, e32)
        if not err < _bar(e32):
            failures.append((name, err, e32, _bar(e32)))
    dev_dense = _dense_grads(m)
    assert len(dev_dense) == len(r64["dense"])
    for (name, g), g64, g32 in zip(dev_dense, r64["dense"], r32["dense"]):
        g64 = np.asarray(g64).reshape(g.shape)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name
        hold(name, _rms_err(g, g64), _rms_err(np.asarray(g32).reshape(g.shape), g64))
    D = m.D
    dc = m._ws["dact0"][:B * D].view(B, D)
    if m.D_in < D:
        dc = dc[:, :m.D_in]
    dc = dc.cpu().numpy()
    assert np.isfinite(dc).all() and np.abs(dc).max() > 0
    dc64 = r64["d_concat"]
    if small_rows_may_vanish is not None:
        # rows the documented cut-off may drop (fp64 dlogit below 2^-38 of the largest): either right or exactly zero
        tiny = small_rows_may_vanish(r64["dlogit"])
        gone = tiny & ~dc.any(1)
        print("GRAD %-34s rows below 2^-38 of the largest dlogit: %d, of them zero on the device: %d" % (
            case, int(tiny.sum()), int(gone.sum())))
        dc, dc64, dc32 = dc[~gone], dc64[~gone], r32["d_concat"][~gone]
    else:
        dc32 = r32["d_concat"]
    hold("d_concat", row_rel_err(dc, dc64), row_rel_err(dc32, dc64))
    # An example's row of d_concat is its dlogit times a row that does not depend on it, and sigmoid(x) - y loses relative
    # precision by cancellation wherever the two are close (in fp32 on every side): the measure above then shows the head's
    # conditioning.  Per unit of each side's OWN dlogit the row is the chain of data gradients alone.
    dl = m._ws["dlogit"][:B].cpu().numpy().astype(np.float64)
    dl64, dl32 = r64["dlogit"], r32["dlogit"].astype(np.float64)
    if small_rows_may_vanish is not None:
        dl, dl64, dl32 = dl[~gone], dl64[~gone], dl32[~gone]
    assert (dl != 0).all() and (dl32 != 0).all()
    unit64 = dc64 / dl64[:, None]
    hold("d_concat/dlogit", row_rel_err(dc / dl[:, None], unit64), row_rel_err(dc32 / dl32[:, None], unit64))
    hold("dlogit", _rms_err(m._ws["dlogit"][:B].cpu().numpy(), r64["dlogit"]), _rms_err(r32["dlogit"], r64["dlogit"]))
    if flags[1]:
        hold("sumv", row_rel_err(m._ws["sumv"][:B * E].view(B, E).cpu().numpy(), r64["sumv"]),
             row_rel_err(r32["sumv"], r64["sumv"]))
    if m.planes:
        _check_amax_chain(m, B)
    assert not failures, failures
    return m, r64


def _planes_wgrad_layers(m, B):
    return [i for i in range(len(m.hidden)) if m._wgrad_planes_ok(B, i)]


def _splits(m, B, i):
    """split-K slabs of hidden layer i's planes weight gradient (the library's launch plan, restated in test_hip_planes)"""
    _, _, fan, h = m.layers[i]
    return planned_splits(B, h, fan)


@pytest.mark.parametrize("B,splits", [(64, 1), (1024, 2), (2080, None), (4096, None)])
def test_config3_shape_gradients(B, splits):
    """26 fields, E = 64, hidden [512, 256, 128]: every weight gradient reads planes, as one batch.  B = 64: one split,
    every job direct; 1024: the first B with two splits; 2080 = 65 x 32: an uneven last split and a partial 256-thread
    block of the per-example factors; 4096: the last hidden layer inside the fused head launch."""
    m, _ = _one_step("config3 B=%d" % B, VOCAB3, 64, [512, 256, 128], B)
    assert _planes_wgrad_layers(m, B) == [0, 1, 2] and "wgrad_batch_ws" in m._ws
    got = [_splits(m, B, i) for i in range(3)]
    print("GRAD config3 B=%d splits per layer %s" % (B, got))
    if splits == 1:
        assert got == [1, 1, 1]
    else:
        assert max(got) >= (splits or 2)
    assert _top_fused(m) == (B >= 4096)


def test_config3_shape_gradients_with_dropout():
    """keep_prob in the data gradients, the mbits masks"""
    B = 4096
    m, _ = _one_step("config3 B=4096 dropout 0.1", VOCAB3, 64, [512, 256, 128], B, dropout=0.1)
    assert _planes_wgrad_layers(m, B) == [0, 1, 2] and "wgrad_batch_ws" in m._ws and "mbits0" in m._ws


@pytest.mark.parametrize("hidden", [[512, 384, 128], [640, 256]])
def test_register_staged_weight_gradient_beside_the_lds_dma_one(hidden):
    """N = 384 / 640: gemm_wgrad_pl.inc's kernel and wgrad_pl.hip's in one batch"""
    B = 2080
    m, _ = _one_step("hidden %s B=%d" % (hidden, B), VOCAB3, 64, hidden, B)
    assert _planes_wgrad_layers(m, B) == list(range(len(hidden))) and "wgrad_batch_ws" in m._ws
    assert any(h not in (128, 256, 512) for h in hidden) and any(h in (128, 256, 512) for h in hidden)


def test_wide_layers_data_gradient_through_fp32_then_split():
    """fan-in 1024 > 512: the data gradient that is not written straight as planes (mi_split_rows after it)"""
    B = 2080
    m, _ = _one_step("hidden [1024, 512, 128] B=%d" % B, VOCAB3, 64, [1024, 512, 128], B)
    assert _planes_wgrad_layers(m, B) == [0, 1, 2] and "wgrad_batch_ws" in m._ws
    assert m.layers[1][2] == 1024 and "dact1" in m._ws          # (direct is false for layer 1's input gradient)


def test_top_hidden_layer_off_the_tile_grid():
    """Hidden [512, 256, 112]: the top hidden layer's weight gradient runs on fp32 operands (112 is no multiple of 128)
    above two planes ones, its dY exists in fp32 (need_f), and the tail is not fused (112 is none of 64 / 128 / 256)."""
    B = 2080
    m, _ = _one_step("hidden [512, 256, 112] B=%d" % B, VOCAB3, 64, [512, 256, 112], B)
    assert _planes_wgrad_layers(m, B) == [0, 1] and "wgrad_batch_ws" in m._ws
    assert not m._tail_fusable() and "dact3" in m._ws


def test_top_hidden_layer_of_100_units_leaves_the_planes_path():
    """Hidden [512, 256, 100]: 100 is no multiple of 16, so the WHOLE model leaves the planes path (engine.planes is
    all-or-nothing) and every GEMM is the any-shape one on fp32 operands — the same gradients, the same bars."""
    B = 2080
    m, _ = _one_step("hidden [512, 256, 100] B=%d" % B, VOCAB3, 64, [512, 256, 100], B, expect_planes=False)
    assert _planes_wgrad_layers(m, B) == [] and "wgrad_batch_ws" not in m._ws


def test_wide_and_deep_raw_numeric_columns_in_the_planes():
    """canned Wide&Deep, E = 32, three raw numeric columns: the gather writes them into the planes (pl_numeric), 131 -> 160
    columns are no whole k-tile, so every weight gradient takes the fp32 operands (the concat back through mi_merge_rows);
    dw_num from mi_numeric_raw_bwd."""
    B = 1024
    m, _ = _one_step("wide&deep raw numeric B=%d" % B, [9, 13, 5, 6], 32, [64, 32], B, nn=3, numeric="raw",
                     flags=(True, False, True), reduction="sum")
    assert m.pl_numeric and m.D_in == 131 and m.D == 160
    assert _planes_wgrad_layers(m, B) == [] and "wgrad_batch_ws" not in m._ws and "concat" in m._ws


def test_deepfm_numeric_embeddings_gradients():
    """13 numeric embeddings at E = 64, B = 2080: mi_numeric_embed_bwd with nine blocks, the last one partial"""
    B = 2080
    m, _ = _one_step("deepfm 13 numeric embeddings B=%d" % B, VOCAB3, 64, [512, 256, 128], B, nn=13)
    assert m.num_emb_off is not None and m.D == 39 * 64
    # (39 x 64 = 2496 input columns are no multiple of 128: layer 1's weight gradient reads the fp32 concat, the two above planes)
    assert _planes_wgrad_layers(m, B) == [1, 2] and "wgrad_batch_ws" in m._ws


# ---- wide dynamic range: the state late in training --------------------------------------------------------------------
WIDE_B, WIDE_WRONG, WIDE_LIN = 4096, 48, -16.0


def _wide_range_problem(p, ids, x, y):
    """Every wide weight is lowered by 16 / 26, so every example's wide sum — and, the FM and MLP terms being a few units,
    its logit — sits around -16; the labels agree with the logit's sign (confidently right: dlogit = sigmoid(x) / B, about
    e^-16 / B) except for WIDE_WRONG examples spread over the batch (confidently wrong: dlogit about -1 / B).  The
    confident side is the NEGATIVE one on purpose: sigmoid(x) - 0 keeps its full relative precision in fp32 however small
    it is, while for a label 1 and x > 16.6 fp32's sigmoid(x) - 1 is exactly 0 (in TensorFlow as here), and there would be
    no small rows to follow.  Returns the labels."""
    F = len(p.lin_w)
    for f in range(F):
        p.lin_w[f] += np.float32(WIDE_LIN / F)
    c = O.forward(p.astype(np.float64), ids, x)
    y = (c["logits"] > 0).astype(np.uint8)
    y[np.arange(0, len(y), len(y) // WIDE_WRONG)[:WIDE_WRONG]] ^= 1
    return y


def _wide_range_facts(dlogit):
    a = np.abs(dlogit)
    return a, a < a.max() * 2.0 ** -38


def test_wide_range_inputs_by_the_oracle_alone():
    """(needs no GPU work: the construction's promises, checked in fp64) the examples' dlogit span at least 2^20, most rows
    sit 2^-20 and more below the largest, and at most 1 % fall below the weight gradient's documented 2^-38 cut-off"""
    p, ids, x, y = make_problem(SEED, VOCAB3, 64, [512, 256, 128], WIDE_B)
    y = _wide_range_problem(p, ids, x, y)
    c = O.forward(p.astype(np.float64), ids, x)
    a, tiny = _wide_range_facts(O.head(c["logits"], y)[1])
    print("GRAD wide range: |logit| median %.1f, dlogit span 2^%.1f, rows 2^-20 below the largest %d / %d, below 2^-38: %d" % (
        float(np.median(np.abs(c["logits"]))), float(np.log2(a.max() / a.min())), int((a < a.max() * 2.0 ** -20).sum()), len(a),
        int(tiny.sum())))
    assert a.min() > 0 and a.max() / a.min() >= 2.0 ** 20
    assert (a < a.max() * 2.0 ** -20).sum() > len(a) // 2
    assert tiny.sum() <= len(a) // 100
    assert 24 <= (a > a.max() * 0.25).sum() <= 4 * WIDE_WRONG


def test_wide_dynamic_range_gradients():
    """Most examples confidently right, a few dozen wrong: most rows of every dY lie 2^-20 and more below the matrix
    abs-max, where the weight gradient's per-example factors go subnormal (kflag).  The weights' measure is relative to
    the rms the few large examples set; d_concat is measured per row, which is what shows whether small rows survive."""
    B = WIDE_B
    m, r64 = _one_step("config3 B=4096 wide range", VOCAB3, 64, [512, 256, 128], B, prepare=_wide_range_problem,
                       small_rows_may_vanish=lambda d: _wide_range_facts(d)[1])
    a, tiny = _wide_range_facts(r64["dlogit"])
    assert a.max() / a.min() >= 2.0 ** 20 and tiny.sum() <= B // 100
    assert _planes_wgrad_layers(m, B) == [0, 1, 2] and "wgrad_batch_ws" in m._ws


# ---- the optimizers that do not normalise the gradient, on the planes path ------------------------------------------------
@pytest.mark.parametrize("name,lr", [("SGD", 0.05), ("Adagrad", 0.05)])
def test_non_normalising_optimizers_on_the_planes_path(name, lr):
    """test_other_optimizers_training's bars (loss 5e-5, variables 2e-5) at a shape whose weight gradients read planes in two
    splits: an update proportional to the gradient shows a wrong scale that Adam's m / sqrt(v) cancels."""
    from mi355x_rec.engine import OptimizerSpec
    hidden, B = [512, 256, 128], 1024
    p, ids, x, y = make_problem(SEED, VOCAB3, 64, hidden, B)
    m = _hip_engine(VOCAB3, 64, hidden, gemm="f16x2", optimizer=OptimizerSpec(name, lr))
    assert m.planes
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper(name, lr))
    for step in range(3):
        loss_g, _ = m.train_step(dev(ids), dev(y))
        masks = _device_relu_masks(m, B)
        pre = O.forward(p.astype(np.float64), ids)["pre"]
        for mk, q in zip(masks, pre):
            diff = mk != (q > 0)
            assert not diff.any() or float(np.abs(q[diff]).max()) < 1e-6, (step, float(np.abs(q[diff]).max()))
        loss_o, _ = O.train_step(p, st, ids, y, relu_masks=masks)
        assert abs(loss_g.item() - float(loss_o)) / abs(float(loss_o)) < 5e-5, step
    assert _planes_wgrad_layers(m, B) == [0, 1, 2] and "wgrad_batch_ws" in m._ws and max(_splits(m, B, i) for i in range(3)) > 1
    _compare_vars(m, p, 2e-5)


# ---- config 3 itself --------------------------------------------------------------------------------------------------
def _torch_reference(dt, v, lin, dense, m, y, masks, sel, chunk=8192):
    """forward, head and the three layers' backward written out in torch on the device, in chunks of examples; the
    weight gradients accumulate over the chunks in dt.  v [B, F, E], lin [B, F]: the rows the batch reads, taken BEFORE
    the step; dense: the dense variables before the step.  Returns ({name: gradient}, d_concat[sel], worst |pre| among
    the units whose device decision differs from this precision's own sign test)."""
    B, nl = v.shape[0], len(m.layers)
    K = [m.kernel(i, dense).to(dt) for i in range(nl)]
    b = [m.bias(i, dense).to(dt) for i in range(nl)]
    gK = [torch.zeros_like(k) for k in K]
    gb = [torch.zeros_like(x) for x in b]
    g_lin_bias = torch.zeros((), dtype=dt, device=v.device)
    dc_sel, worst = [], 0.0
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        e = v[sl].to(dt)
        logits = lin[sl].to(dt).sum(1) + dense[m.lin_bias_off].to(dt)
        logits = logits + 0.5 * ((e.sum(1) ** 2).sum(1) - (e * e).sum((1, 2)))
        acts = [e.reshape(e.shape[0], -1)]
        for i in range(nl - 1):
            pre = acts[-1] @ K[i] + b[i]
            mk = masks[i][sl]
            diff = mk != (pre > 0)
            if bool(diff.any()):
                worst = max(worst, float(pre[diff].abs().max()))
            acts.append(torch.where(mk, pre, torch.zeros_like(pre)))
        logits = logits + (acts[-1] @ K[-1] + b[-1])[:, 0]
        dlogit = (torch.sigmoid(logits) - y[sl].to(dt)) / B
        g_lin_bias += dlogit.sum()
        d = dlogit[:, None]
        for i in range(nl - 1, -1, -1):
            if i < nl - 1:
                d = d * masks[i][sl].to(dt)
            gK[i] += acts[i].T @ d
            gb[i] += d.sum(0)
            d = d @ K[i].T
        inside = sel[(sel >= sl.start) & (sel < sl.stop)] - sl.start
        dc_sel.append(d[inside])
    out = {"lin_bias": g_lin_bias.reshape(1)}
    for i in range(nl):
        out["kernel_%d" % i], out["bias_%d" % i] = gK[i], gb[i]
    return out, torch.cat(dc_sel), worst


def test_full_size_gradients():
    """BASELINE config 3 itself (B = 65536, 26 x 1M rows, E = 64, [512, 256, 128]), one step: every dense gradient — a sum
    over all examples, so nothing can be sampled — and d_concat on the examples arange(0, B, 997), against torch fp64 on
    the device made from the engine's own tables (the rows and dense variables as they were before the step); the bar's
    second term from the same code in torch fp32."""
    F, V, E, B = 26, 1_000_000, 64, 65536
    m = _hip_engine([V] * F, E, [512, 256, 128], gemm="f16x2")
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    m.init_variables(g, lin_scale=1e-3)
    for i in range(len(m.layers)):
        m.bias(i).normal_(0.0, 0.05, generator=g)
    ids = torch.randint(0, V, (B, F), device="cuda", dtype=torch.int32, generator=g)
    y = (torch.rand(B, device="cuda", generator=g) < 0.25).to(torch.uint8)
    rows = ids.long() + m.field_off[None, :]
    v0, lin0, dense0 = m.table[rows].clone(), m.lin_w[rows].clone(), m.dense.clone()
    sel = torch.arange(0, B, 997, device="cuda")
    m.train_step(ids, y)
    torch.cuda.synchronize()
    assert m.planes and _top_fused(m) and m._frozen is None
    assert _planes_wgrad_layers(m, B) == [0, 1, 2] and "wgrad_batch_ws" in m._ws and min(_splits(m, B, i) for i in range(3)) > 1
    assert bool(torch.isfinite(m.d_grad).all()) and float(m.d_grad.abs().max()) > 0
    masks = [torch.from_numpy(a).cuda() for a in _relu_masks(m, B)]
    t0 = time.perf_counter()
    r64, dc64, worst = _torch_reference(torch.float64, v0, lin0, dense0, m, y, masks, sel)
    r32, dc32, _ = _torch_reference(torch.float32, v0, lin0, dense0, m, y, masks, sel)
    torch.cuda.synchronize()
    print("GRAD config 3 full size: torch fp64 + fp32 references %.1f s; worst |pre| of a differing relu decision %.2e" % (
        time.perf_counter() - t0, worst))
    assert worst < 1e-6
    failures = []
    case = "config3 full size B=65536"
    for name, got in _dense_grads(m):
        err = _rms_err(got, r64[name].cpu().numpy())
        e32 = _rms_err(r32[name].cpu().numpy(), r64[name].cpu().numpy())
        _report(case, name, err, e32)
        if not err < _bar(e32):
            failures.append((name, err, e32))
    dc = m._ws["dact0"][:B * m.D].view(B, m.D)[sel].cpu().numpy()
    err, e32 = row_rel_err(dc, dc64.cpu().numpy()), row_rel_err(dc32.cpu().numpy(), dc64.cpu().numpy())
    _report(case, "d_concat", err, e32)
    if not err < _bar(e32):
        failures.append(("d_concat", err, e32))
    _check_amax_chain(m, B)
    assert not failures, failures
