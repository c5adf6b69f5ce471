"""-m gpu: the gradients of ONE train step — on the planes path (engine._backward_dense as the benchmark runs it) and on the
any-shape path every other model takes (layered_grad_check.CASES) — against the oracle's own backward in fp64.  The
checker is tests/layered_grad_check.py, which test_layered_gradients_cpu.py runs on the numpy stand-in.

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
from tests.layered_grad_check import CASES, SEED, bar as _bar, check_amax_chain, dense_grads as _dense_grads, one_step
from tests.layered_grad_check import relu_masks as _relu_masks, report as _report, rms_err as _rms_err, run_case
from tests.layered_grad_check import top_fused as _top_fused
from tests.util import _compare_vars, _device_relu_masks, dev, make_problem, planned_splits, row_rel_err

pytestmark = pytest.mark.gpu

VOCAB3 = [40 + 3 * i for i in range(26)]                     # config 3's 26 fields, small vocabularies


def _one_step(case, vocab, E, hidden, B, **kw):
    """layered_grad_check.one_step on a HIP engine (gemm "f16x2", relu unless told otherwise).  Returns (engine, fp64 reference)."""
    r = one_step(case, _hip_engine, vocab, E, hidden, B, **kw)
    return r.m, r.r64


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


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_any_shape_path_gradients(case):
    """The models that leave the planes path (an activation other than relu, a width that is no multiple of 16, gemm "fp32" /
    "bf16x3"): every gradient of one step, and the abs-max chain of the f16x2 weight gradients, at shapes with several row
    tiles, column tiles and split-K slabs.  Which kernel each GEMM reaches is stated with the case and asserted there."""
    run_case(case, _hip_engine)


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
    failures += check_amax_chain(m, B)
    assert not failures, failures
