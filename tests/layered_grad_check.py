"""The gradients of ONE layered train step (engine._backward_dense) against the oracle's own backward in fp64 (shared by
test_hip_gradients.py, on the device, and test_layered_gradients_cpu.py, on the numpy stand-in).  Not a test file.

What is read: every dense gradient (DeepFM.d_grad: kernels, biases, linear bias, numeric embeddings, numeric linear
weights), the gradient of the concat (_ws["dact0"]), sumv and dlogit.  The embedding-row gradients need no comparison of
their own: test_embed_bwd_entries (test_hip_kernels.py) holds the entry kernel to the oracle GIVEN d_concat, sumv and
dlogit, and test_sparse_apply_fused_equals_bwd_then_apply_bitwise ties the fused sparse apply to that kernel.

Measures.  Dense variables: max |g - ref| / rms(ref).  d_concat: tests.util.row_rel_err (per example, relative to that
example's own rms).  Bars: max(1e-5, 4 x E32), where E32 is the SAME measure for the oracle's fp32 backward (numpy, same
inputs, same relu / dropout masks) against its fp64 one; E32 never comes from the engine.  Every figure is printed
(pytest -s): variable, engine error, fp32-oracle error, bar.

Relu decisions are the engine's (read back after the step, handed to oracle.forward(relu_masks=...)); they may differ
from the fp64 oracle's own sign test only where the fp64 pre-activation is within 1e-6 of 0.  The other activations have
no decisions: the oracle applies them itself, and the d_concat chain takes f' from the oracle's PRE-activation (the
engine and oracle.backward both go through the stored output).  Under dropout no kept unit's stored output may be
exactly 0 there, so that the rule "an output that is exactly 0 counts as dropped" stays out of the comparison.  Dropout
masks are replayed on the host (tests.util.dropout_mask).

one_step(..., hold=False) returns the failures instead of raising: test_layered_gradients_cpu.py shows with it that a
stand-in wrong in one tile, one slab or one abs-max vector does not pass."""
import time
from collections import namedtuple

import numpy as np
import torch

from oracle import deepfm as O
from tests.util import _device_relu_masks, dev, dropout_mask, make_problem, row_rel_err

SEED = 319                                                   # test_hip_model.CONFIG3_SAFE_SEED's problem

Result = namedtuple("Result", "m r64 failures")


def rms_err(got, ref):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / (np.sqrt(np.mean(ref * ref)) + 1e-300))


def bar(e32):
    return max(1e-5, 4.0 * e32)


def report(case, name, err, e32):
    print("GRAD %-34s %-15s device %.2e  fp32-oracle %.2e  bar %.2e%s" % (
        case, name, err, e32, bar(e32), "  (second term)" if err >= 1e-5 else ""))


def merged(m, name, B, K):
    out = torch.empty(B, K, device="cuda")
    m.k.mi_merge_rows(m._pl[name].struct, B, K, out, K)
    return out


def top_fused(m):
    return getattr(m, "_top_step", None) == m.step - 1


def relu_masks(m, B):
    """_device_relu_masks, and for a last hidden layer that ran inside the fused logits + head launch (its output never
    reaches memory) the units whose gradient that launch let through: dY of that layer is dlogit * w masked, and neither
    factor is 0 here — checked by the caller's assertion that a decision differs from the fp64 sign test only within 1e-6
    of 0, which an unexplained zero would fail."""
    masks = _device_relu_masks(m, B)
    if top_fused(m):
        nh = len(m.hidden)
        assert bool((m._ws["dlogit"][:B] != 0).all()), "a dlogit that is exactly 0"
        masks[nh - 1] = (merged(m, "dy%dp" % (nh - 1), B, m.hidden[-1]) != 0).cpu().numpy()
    return masks


def dense_grads(m):
    """name -> engine gradient, in oracle.Params.dense_list() order (kernel_0 without its zero pad rows, which must have
    got exactly zero gradients)"""
    g = m.d_grad
    out = []
    for i in range(len(m.layers)):
        k = m.kernel(i, g)
        if i == 0 and m.D_in < m.D:
            assert float(k[m.D_in:].abs().max()) == 0.0, "kernel_0's pad rows got a gradient"
            k = k[:m.D_in]
        out += [("kernel_%d" % i, k.cpu().numpy()), ("bias_%d" % i, m.bias(i, g).cpu().numpy())]
    out.append(("lin_bias", g[m.lin_bias_off:m.lin_bias_off + 1].cpu().numpy()))
    if m.num_emb_off is not None:
        out.append(("num_emb", m._seg(g, m.num_emb_off, (m.n_numeric, m.E)).cpu().numpy()))
    if m.lin_num_off is not None:
        out.append(("dw_num", g[m.lin_num_off:m.lin_num_off + m.n_numeric].cpu().numpy()))
    return out


def act_deriv(activation, pre):
    """f'(pre) from the pre-activation itself, in pre's precision (relu has masks instead)"""
    if activation == "sigmoid":
        s = 1 / (1 + np.exp(-pre))
        return s * (1 - s)
    if activation == "tanh":
        t = np.tanh(pre)
        return 1 - t * t
    assert activation is None, activation
    return np.ones_like(pre)


def oracle_grads(p, ids, x, y, dt, masks, drop, keep, flags, numeric, reduction, activation="relu"):
    q = p.astype(dt)
    xx = None if x is None else x.astype(dt)
    c = O.forward(q, ids, xx, *flags, dropout_masks=drop, numeric=numeric, keep_prob=keep, relu_masks=masks,
                  activation=activation)
    loss, dlogit, _, _ = O.head(c["logits"], y, reduction)
    dense, _, _ = O.backward(q, c, dlogit, drop)
    nh = len(q.mlp) - 1
    # d loss / d concat as the MLP sees it (the engine's dact0): backward() folds it into the row gradients
    d = dlogit[:, None] * q.mlp[nh][0][:, 0][None, :]
    for i in range(nh - 1, -1, -1):
        if drop is not None:
            d = (d * drop[i].astype(dt)) / dt(keep)
        fp = masks[i].astype(dt) if activation == "relu" else act_deriv(activation, c["pre"][i]).astype(dt)
        d = (d * fp) @ q.mlp[i][0].T
    return dict(dense=dense, d_concat=d, dlogit=dlogit, sumv=c.get("sumv"), pre=c["pre"], loss=float(loss),
                logits=c["logits"], concat=c.get("concat"))


def check_masks(masks, pre64, drop):
    """the engine's relu decisions against the fp64 sign test: they may differ only on marginal units"""
    flips = 0
    for i, (mk, q) in enumerate(zip(masks, pre64)):
        own = q > 0
        if drop is not None:
            own &= drop[i] > 0                  # (a dropped unit's stored activation is 0: its mask bit is off)
        diff = mk != own
        flips += int(diff.sum())
        assert not diff.any() or float(np.abs(q[diff]).max()) < 1e-6, (i, int(diff.sum()), float(np.abs(q[diff]).max()))
    return flips


def check_amax_chain(m, B, x0_true=None):
    """Every abs-max vector the weight gradients consume (x<i>, dy<i> of each hidden layer) against the matrix it
    describes: same binary exponent as the true abs-max, and not below it by more than the planes' own rounding (2^-20
    relative).  A stale, unzeroed or undersized vector is reported.  Planes path: dY in fp32 where this step wrote it
    (need_f), as planes (merged) otherwise; activations from the planes the GEMMs read.  Any-shape f16x2 path: the fp32
    buffers themselves — x<i> is act<i-1> (x0: the concat, or x0_true where layer 1 gathers it and no concat exists),
    dy<i> is dact<i+1>.  Returns the failures."""
    failures = []
    nh = len(m.hidden)
    amax_of = lambda t: float(t.abs().max())
    for i in range(nh):
        fan, h = m.layers[i][2], m.layers[i][3]
        if m.planes:
            x_true = amax_of(merged(m, "x%dp" % i, B, fan))
            # dact<i+1> = dY of layer i in fp32: written when the layer above is the fused tail / gemv and this layer's weight
            # gradient reads fp32, or when the data gradient above could not write planes straight (see _backward_dense)
            if i == nh - 1:
                need_f = not m._wgrad_planes_ok(B, i)
            else:
                need_f = not (h <= 512 and m._wgrad_planes_ok(B, i))
            if need_f:
                dy_true = amax_of(m._ws["dact%d" % (i + 1)][:B * h])
            else:
                dy_true = amax_of(merged(m, "dy%dp" % i, B, h))
        else:
            if i > 0:
                x_true = amax_of(m._ws["act%d" % (i - 1)][:B * fan])
            elif m.gather_mlp:
                assert x0_true is not None, "the gathered concat's abs-max comes from the caller"
                x_true = float(x0_true)
            else:
                x_true = amax_of(m._ws["concat"][:B * fan])
            dy_true = amax_of(m._ws["dact%d" % (i + 1)][:B * h])
        for name, true in (("x%d" % i, x_true), ("dy%d" % i, dy_true)):
            assert name in m._amax_idx, name
            got = float(m._av(name).max())
            assert true > 0 and np.isfinite(true), (name, true)
            if np.frexp(got)[1] != np.frexp(true)[1] or not got >= true * (1 - 2.0 ** -20):
                failures.append(("amax " + name, got, true))
    return failures


def gemm_families(m, B):
    """Which kernel of gemm.hip's launcher each GEMM of the any-shape path reaches, restated from the launcher's rules and
    decided by the ENGINE's own pointers and widths: per layer {"fwd", "dgrad", "wgrad"} -> family.
      gemv           N = 1 and every operand float4-addressable (gemv_fwd_k / gemv_dgrad_k / gemv_wgrad_k)
      f16x2 whole    weight gradient, both abs-max vectors, whole 128 x 128 x 32 tiles
      f16x2 ragged   weight gradient, both abs-max vectors, any shape
      bf16x3         both operands float4-addressable, mode 1
      f32 AB         the fp32-input MFMA kernel; A / B: v = float4 loads, s = scalar loads, g = gathered rows
    (dgrad of layer 0 is the gradient of the concat.)"""
    assert not m.planes
    vec = lambda ptr_ok, ld, extent: bool(ptr_ok and ld % 4 == 0 and extent % 4 == 0)
    mode1 = m.gemm != "fp32"
    f16 = m.gemm == "f16x2"
    nh = len(m.layers) - 1
    out = []
    for i, (_, _, fan, h) in enumerate(m.layers):
        w_ok = m.kernel(i).data_ptr() % 16 == 0
        gathered = i == 0 and m.gather_mlp
        ws_ok = lambda name: m._ws[name].data_ptr() % 16 == 0       # (the step has run: its buffers exist)
        xv = True if gathered else vec(ws_ok("act%d" % (i - 1) if i else "concat"), fan, fan)
        wv = vec(w_ok, h, h)
        dyv = vec(ws_ok("dact%d" % (i + 1)) if i < nh else ws_ok("dlogit"), h, h)

        def f32(a, b):
            return "f32 %s%s" % ("g" if (a and gathered) else "v" if a else "s", "v" if b else "s")
        fam = {}
        if h == 1:
            ok = vec(w_ok, fan, fan)
            fam = {"fwd": "gemv" if ok else f32(xv, wv), "dgrad": "gemv" if ok else "f32 %s%s" % ("v" if dyv else "s", "v" if wv else "s"),
                   "wgrad": "gemv" if (ok and not gathered) else f32(xv, dyv)}
        else:
            fam["fwd"] = ("bf16x3" + (" g" if gathered else "")) if (mode1 and xv and wv) else f32(xv, wv)
            fam["dgrad"] = "bf16x3" if (mode1 and dyv and wv) else "f32 %s%s" % ("v" if dyv else "s", "v" if wv else "s")
            if mode1 and xv and dyv:
                if f16 and i < nh:
                    whole = fan % 128 == 0 and h % 128 == 0 and B % 32 == 0
                    fam["wgrad"] = ("f16x2 whole" if whole else "f16x2 ragged") + (" g" if gathered else "")
                else:
                    fam["wgrad"] = "bf16x3" + (" g" if gathered else "")
            else:
                fam["wgrad"] = f32(xv, dyv)
        out.append(fam)
    return out


def wgrad_splits(M, N, K):
    """split-K slabs of mi_dense_bwd_weight (gemm.hip's wgrad_splits, restated)"""
    cdiv = lambda a, b: -(-a // b)
    return max(1, min(1024 // (cdiv(K, 128) * cdiv(N, 128)), cdiv(M, 128), 256))


def one_step(case, make_engine, vocab, E, hidden, B, nn=0, numeric="embed", dropout=0.0, flags=(True, True, True),
             reduction="mean", prepare=None, expect_planes=True, small_rows_may_vanish=None, activation="relu",
             gemm="f16x2", hold=True):
    """One train_step of an engine (make_engine(vocab, E, hidden, n_numeric=..., **kw), any device) loaded with oracle
    parameters; every gradient against the fp64 oracle.  Returns Result(engine, fp64 reference, failures); with hold a
    non-empty list of failures is an AssertionError."""
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
    m = make_engine(vocab, E, hidden, n_numeric=nn, gemm=gemm, numeric=numeric, dropout=dropout, seed=7, reduction=reduction,
                    use_linear=flags[0], use_mf=flags[1], use_dnn=flags[2], activation=activation)
    assert bool(m.planes) == expect_planes, (case, bool(m.planes))
    m.load_oracle_params(p)
    keep = 1.0 - dropout
    drop = [dropout_mask(m._layer_seed(i), B, h, keep) for i, h in enumerate(hidden)] if dropout else None   # (step 0's seeds)
    loss_g, logit_g = m.train_step(dev(ids, m.device), dev(y, m.device), dev(x, m.device))
    if m.device.type == "cuda":
        torch.cuda.synchronize()
    # Nothing in _apply writes d_grad unless variables are frozen (deep_numeric / wide_numeric column subsets: none here),
    # so the gradients of the step survive it.  A buffer nobody filled must not pass: finite and non-zero.
    assert m._frozen is None, case
    assert bool(torch.isfinite(m.d_grad).all()) and float(m.d_grad.abs().max()) > 0, case
    relu = activation == "relu"
    masks = relu_masks(m, B) if relu else None
    if not relu and drop is not None:
        for i, h in enumerate(hidden):
            a = m._ws["act%d" % i][:B * h].view(B, h).cpu().numpy()
            assert np.array_equal(a == 0, drop[i] == 0), (case, "layer %d: a kept unit's stored output is exactly 0" % i)
    t0 = time.perf_counter()
    r64 = oracle_grads(p, ids, x, y, np.float64, masks, drop, keep, flags, numeric, reduction, activation)
    r32 = oracle_grads(p, ids, x, y, np.float32, masks, drop, keep, flags, numeric, reduction, activation)
    host_s = time.perf_counter() - t0
    flips = check_masks(masks, r64["pre"], drop) if relu else 0
    print("GRAD %-34s B=%d  oracle fp64 + fp32 on the host: %.1f s, marginal relu decisions taken from the device: %d, "
          "top layer fused: %s" % (case, B, host_s, flips, top_fused(m)))
    failures = []
    loss_err = abs(loss_g.item() - r64["loss"]) / abs(r64["loss"])
    if not loss_err <= 1e-5:
        failures.append(("loss", loss_err))

    def hold_to(name, err, e32):
        report(case, name, err, e32)
        if not err < bar(e32):
            failures.append((name, err, e32, bar(e32)))
    dev_dense = dense_grads(m)
    assert len(dev_dense) == len(r64["dense"]), case
    for (name, g), g64, g32 in zip(dev_dense, r64["dense"], r32["dense"]):
        g64 = np.asarray(g64).reshape(g.shape)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name
        hold_to(name, rms_err(g, g64), rms_err(np.asarray(g32).reshape(g.shape), g64))
    D = m.D
    dc = m._ws["dact0"][:B * D].view(B, D)
    if m.D_in < D:
        dc = dc[:, :m.D_in]
    dc = dc.cpu().numpy()
    assert np.isfinite(dc).all() and np.abs(dc).max() > 0, case
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
    hold_to("d_concat", row_rel_err(dc, dc64), row_rel_err(dc32, dc64))
    # An example's row of d_concat is its dlogit times a row that does not depend on it, and sigmoid(x) - y loses relative
    # precision by cancellation wherever the two are close (in fp32 on every side): the measure above then shows the head's
    # conditioning.  Per unit of each side's OWN dlogit the row is the chain of data gradients alone.
    dl = m._ws["dlogit"][:B].cpu().numpy().astype(np.float64)
    dl64, dl32 = r64["dlogit"], r32["dlogit"].astype(np.float64)
    if small_rows_may_vanish is not None:
        dl, dl64, dl32 = dl[~gone], dl64[~gone], dl32[~gone]
    assert (dl != 0).all() and (dl32 != 0).all(), case
    unit64 = dc64 / dl64[:, None]
    hold_to("d_concat/dlogit", row_rel_err(dc / dl[:, None], unit64), row_rel_err(dc32 / dl32[:, None], unit64))
    hold_to("dlogit", rms_err(m._ws["dlogit"][:B].cpu().numpy(), r64["dlogit"]), rms_err(r32["dlogit"], r64["dlogit"]))
    if flags[1]:
        hold_to("sumv", row_rel_err(m._ws["sumv"][:B * E].view(B, E).cpu().numpy(), r64["sumv"]),
                row_rel_err(r32["sumv"], r64["sumv"]))
    if m.planes or (m.gemm == "f16x2" and m.use_dnn and hidden):
        # (the gathered concat of the any-shape path is the oracle's: the rows as loaded, fp32)
        failures += check_amax_chain(m, B, None if r32["concat"] is None else float(np.abs(r32["concat"]).max()))
    if hold:
        assert not failures, (case, failures)
    return Result(m, r64, failures)


# ---- the any-shape (layered, non-planes) cases --------------------------------------------------------------------------
# Case.families: per layer (fwd, dgrad, wgrad) as gemm_families names them — asserted against the engine, not assumed.
Case = namedtuple("Case", "name E hidden B kw families splits")
SMALL = [9, 13, 5, 6]
_GEMV = ("gemv", "gemv", "gemv")
# [130, 40], E = 8 (D = 32), B = 300: three ragged row tiles, two column tiles in layer 1's output.  130 % 4 = 2: layer 1's
# kernel and output are no float4 operands — gathered forward with scalar B loads, an all-scalar gradient of the concat, a
# gathered weight gradient with scalar dY loads; every weight gradient in three split-K slabs; layer 2 (130 -> 40): scalar A beside float4 B in the
# forward and the weight gradient, the split kernel (fp32 mode: float4 loads) in the data gradient; N = 1: gemv.
_F130 = lambda split: [("f32 gs", "f32 ss", "f32 gs"), ("f32 sv", split, "f32 sv"), _GEMV]
# [256, 128], E = 64 (D = 256), B = 256: whole tiles everywhere, every operand float4-addressable — the gathered bf16x3
# forward, bf16x3 data gradients, the f16x2 whole-tile weight gradients (layer 1's gathered, two slabs each); N = 1: gemv.
_F256 = [("bf16x3 g", "bf16x3", "f16x2 whole g"), ("bf16x3", "bf16x3", "f16x2 whole"), _GEMV]
_ACTS = [("sigmoid", dict(activation="sigmoid")), ("tanh dropout 0.2", dict(activation="tanh", dropout=0.2)),
         ("identity", dict(activation=None)), ("sigmoid dropout 0.2", dict(activation="sigmoid", dropout=0.2))]
CASES = [Case("%s [130, 40]" % n, 8, [130, 40], 300, kw, _F130("bf16x3"), [3, 3, 3]) for n, kw in _ACTS]
CASES += [Case("%s [256, 128]" % n, 64, [256, 128], 256, kw, _F256, [2, 2, 2]) for n, kw in _ACTS]
CASES += [
    # [100, 50], E = 8: 100 is no multiple of 16 (the model leaves the planes path) but one of 4, 50 is neither — gathered
    # bf16x3 forward and f16x2 ragged weight gradient in layer 1, scalar loads of the 50-wide operands in layer 2, and an
    # N = 1 layer that no float4 reads (fan-in 50): the general kernel in all three of its GEMMs.
    Case("relu dropout 0.1 [100, 50]", 8, [100, 50], 300, dict(dropout=0.1),
         [("bf16x3 g", "bf16x3", "f16x2 ragged g"), ("f32 vs", "f32 ss", "f32 vs"), ("f32 ss", "f32 ss", "f32 ss")], [3, 3, 3]),
]
# gemm = "fp32": mode 0, the fp32-input MFMA kernel wherever the 16-bit split ran; "bf16x3": no abs-max, no f16x2
CASES += [Case("%s gemm=%s [130, 40]" % (a, g), 8, [130, 40], 300, dict(activation=a, gemm=g),
               _F130("bf16x3" if g == "bf16x3" else "f32 vv"), [3, 3, 3]) for g in ("fp32", "bf16x3") for a in ("relu", "tanh")]
CASES += [
    # three numeric embeddings: D = 7 x 8 = 56, the concat is materialised and layer 1 reads it as a float4 operand
    Case("tanh 3 numeric [130, 40]", 8, [130, 40], 300, dict(activation="tanh", nn=3),
         [("f32 vs", "f32 ss", "f32 vs"), ("f32 sv", "bf16x3", "f32 sv"), _GEMV], [3, 3, 3]),
]


def run_case(case, make_engine, hold=True):
    kw = dict(case.kw)
    r = one_step(case.name, make_engine, SMALL, case.E, case.hidden, case.B, expect_planes=False, hold=hold, **kw)
    m = r.m
    assert not m.planes, case.name
    got = [(f["fwd"], f["dgrad"], f["wgrad"]) for f in gemm_families(m, case.B)]
    assert got == [tuple(f) for f in case.families], (case.name, got)
    assert bool(m.gather_mlp) == ("nn" not in kw), case.name
    splits = [wgrad_splits(case.B, h, fan) for (_, _, fan, h) in m.layers]
    assert splits == case.splits, (case.name, splits)
    return r
