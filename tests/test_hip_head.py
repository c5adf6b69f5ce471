"""-m gpu: the entries of csrc/head.hip and mi_colsum through the C ABI against the fp64 references of tests/head_cases.py, at
the sizes where a two-stage reduction or a histogram kernel goes wrong: either side of one block becoming two (1024 | 1025), the
cap of 1,024 blocks with a last block of 2 examples (2^20 + 1), saturated logits, labels of one class, every subset of the
optional arguments, padded leading dimensions, values on the bucket limits.  These entries anchor three bitwise chains of the
suite (the fused tails, the population evaluation kernel, the serving head): here they are held to fp64 themselves.

The eval counters are integers, so they are compared exactly, in three ways.  Independent of the kernels: on the examples whose
fp64 sigmoid is further than P_BAR from every threshold (head_cases.near; the input is split on the host, the not-near part is
an input of its own) the counters are those of the fp64 sigmoid.  Rule given p: on the whole input they are those of the
logistic mi_binary_predictions reports for the same logits — itself held to fp64 within P_BAR here.  Ties: logits swept ulp by
ulp across every threshold, where a logistic equal to a threshold must not count as above it.

Every output sits between NaN guard bands and every workspace is exactly the size its query gives (tests.util); both are
checked after every call.  Figures are printed (pytest -s): HEAD <what> ..."""
import itertools

import numpy as np
import pytest
import torch

from tests import head_cases as H
from tests.util import _chk, _p, _st, dev, exact_workspace, guarded_nan, guards_intact, workspace_surroundings_intact

pytestmark = pytest.mark.gpu

F32 = np.float32
MI_ERR_WORKSPACE = -4
SMALL_B = H.HEAD_B[:-1]


def _guarded(dtype, n):
    """(whole buffer, zeroed view of n int64 / float64 inside it): an accumulator between two NaN guard bands"""
    buf, v = guarded_nan(2 * n)
    v = v.view(dtype)
    v.zero_()
    assert v.numel() == n and v.data_ptr() % 8 == 0
    return buf, v


# ---- mi_sigmoid_ce_head ----------------------------------------------------------------------------------------------------------
class _HeadOut:
    def __init__(self, B, want):
        self.bufs = {k: guarded_nan(B if k in ("logits", "d") else 1) for k in want}

    def ptr(self, k):
        return _p(self.bufs[k][1]) if k in self.bufs else None

    def intact(self):
        return all(guards_intact(b) for b, _ in self.bufs.values())

    def host(self):
        return {k: v.cpu().numpy().copy() for k, (_, v) in self.bufs.items()}


def _head(lib, parts, y, B, scale, want=("logits", "loss", "d", "dsum"), expect_ok=True, ws_bytes=None, ws_null=False):
    """one call of mi_sigmoid_ce_head with the outputs in `want`; returns (return code, outputs on the host — views into
    NaN-filled buffers, so an output that was not written is NaN)"""
    out = _HeadOut(max(B, 1), want)
    need = lib.mi_head_workspace_bytes(B) if ws_bytes is None else ws_bytes
    wbuf, ws = exact_workspace(need)
    d = {k: dev(parts.get(k)) for k in ("lin", "lin_bias", "fm", "dnn")}
    dy = dev(y)
    rc = lib.mi_sigmoid_ce_head(_p(d["lin"]), _p(d["lin_bias"]), _p(d["fm"]), _p(d["dnn"]), _p(dy), B, scale, out.ptr("logits"),
                                out.ptr("loss"), out.ptr("d"), out.ptr("dsum"), None if ws_null else _p(ws),
                                0 if ws_null else ws.numel(), _st())
    torch.cuda.synchronize()
    assert out.intact() and workspace_surroundings_intact(wbuf, ws)
    if expect_ok:
        _chk(rc, "mi_sigmoid_ce_head")
    return rc, out.host()


def _hold_head(got, x32, y, scale, what):
    l64, d64, _, _ = H.head64(x32, y, scale)
    s = float(F32(scale))
    if "logits" in got:
        assert np.array_equal(got["logits"].view(np.uint32), x32.view(np.uint32)), what
    if "d" in got:
        err = float(np.max(np.abs(got["d"] - d64))) / s
        print("HEAD %-58s max |d - d64| / scale %.3g (bar %.3g)" % (what, err, H.P_BAR + 2.0 ** -24))
        assert np.all(np.abs(got["d"] - d64) <= (H.P_BAR + 2.0 ** -24) * s), (what, err)
    if "loss" in got:
        assert np.isfinite(got["loss"][0]) and abs(got["loss"][0] - l64) <= H.TOL * abs(l64), (what, got["loss"][0], l64)
    if "dsum" in got:
        assert abs(got["dsum"][0] - d64.sum()) <= H.TOL * np.abs(d64).sum(), (what, got["dsum"][0], d64.sum())


def _same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize("B,which", [(B, w) for B in SMALL_B for w in H.LOGIT_SETS] + [(H.BIG, "wide")])
def test_head_against_fp64(lib, B, which):
    z, y = H.logits(which, B), H.labels("mixed", B, which)
    parts, x32 = H.components(z)
    for scale in (1.0 / B, 1.0):
        _, got = _head(lib, parts, y, B, scale)
        _hold_head(got, x32, y, scale, "head %s B=%d scale=%.3g" % (which, B, scale))
        _, again = _head(lib, parts, y, B, scale)
        assert _same_bits(got, again)                      # "bitwise reproducible" (head.hip)


@pytest.mark.parametrize("B", [257, 1025])
def test_head_every_subset_of_the_logit_parts(lib, B):
    z, y = H.logits("wide", B), H.labels("mixed", B, "wide")
    for r in (1, 2, 3):
        for subset in itertools.combinations(("lin", "fm", "dnn"), r):
            for bias in ((True, False) if "lin" in subset else (True,)):
                # (without lin the bias is still handed over: it must be ignored)
                parts, x32 = H.components(z, subset, bias="lin" in subset and bias)
                if "lin" not in subset:
                    parts["lin_bias"] = np.array([0.25], F32)
                _, got = _head(lib, parts, y, B, 1.0 / B)
                _hold_head(got, x32, y, 1.0 / B, "head B=%d parts=%s bias=%s" % (B, "+".join(subset), bias))


def test_head_every_legal_combination_of_outputs(lib):
    B = 1025
    z, y = H.logits("wide", B), H.labels("mixed", B, "wide")
    parts, x32 = H.components(z)
    scale = 1.0 / B
    _, full = _head(lib, parts, y, B, scale)
    _hold_head(full, x32, y, scale, "head B=1025 all outputs")
    for want, labelled, ws_null in ((("logits",), False, True), (("logits",), True, True), (("logits", "loss"), True, False),
                                    (("loss",), True, False), (("logits", "d"), True, True), (("d",), True, True),
                                    (("logits", "loss", "d"), True, False), (("d", "dsum"), True, False)):
        _, got = _head(lib, parts, y if labelled else None, B, scale, want=want, ws_null=ws_null)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k].view(np.uint32), full[k].view(np.uint32)), (want, k)


def test_head_refuses_what_it_cannot_do_and_writes_nothing(lib):
    B = 1025
    z, y = H.logits("normal", B), H.labels("mixed", B)
    parts, _ = H.components(z)
    all4 = ("logits", "loss", "d", "dsum")
    none = {"lin_bias": parts["lin_bias"]}

    def refused(rc, got):
        assert rc != 0 and all(np.isnan(v).all() for v in got.values())
        return rc

    refused(*_head(lib, parts, y, 0, 1.0, expect_ok=False))                                      # B > 0
    refused(*_head(lib, parts, y, -1, 1.0, expect_ok=False))
    refused(*_head(lib, none, y, B, 1.0, expect_ok=False))                                       # a logit component
    refused(*_head(lib, parts, None, B, 1.0, want=("logits", "loss"), expect_ok=False))          # loss needs labels
    refused(*_head(lib, parts, None, B, 1.0, want=("logits", "d"), expect_ok=False))             # so does the gradient
    refused(*_head(lib, parts, y, B, 1.0, want=("logits", "loss"), ws_null=True, expect_ok=False))   # the sums need a workspace
    refused(*_head(lib, parts, y, B, 1.0, want=("d", "dsum"), ws_null=True, expect_ok=False))
    refused(*_head(lib, parts, y, B, 1.0, want=("logits", "loss", "dsum"), expect_ok=False))     # d_logit_sum needs d_logit
    need = lib.mi_head_workspace_bytes(B)
    for want in (all4, ("loss",), ("d", "dsum")):
        assert refused(*_head(lib, parts, y, B, 1.0, want=want, ws_bytes=need - 1, expect_ok=False)) == MI_ERR_WORKSPACE
    # (one block writes no partials, but asks for the same workspace)
    assert refused(*_head(lib, {k: (v[:37] if k != "lin_bias" else v) for k, v in parts.items()}, y[:37], 37, 1.0, ws_bytes=need - 1,
                          expect_ok=False)) == MI_ERR_WORKSPACE


@pytest.mark.parametrize("lab", ["zeros", "ones"])
@pytest.mark.parametrize("B", [257, 1025, 4097])
def test_head_labels_of_one_class_on_saturated_logits(lib, B, lab):
    z, y = H.logits("wide", B), H.labels(lab, B, "wide")
    parts, x32 = H.components(z)
    assert np.abs(x32).max() == 1e4
    for scale in (1.0 / B, 1.0):
        _, got = _head(lib, parts, y, B, scale)
        _hold_head(got, x32, y, scale, "head wide labels=%s B=%d scale=%.3g" % (lab, B, scale))


# ---- mi_binary_predictions -------------------------------------------------------------------------------------------------------
def _predictions(lib, z, y=None, want=("p", "pr", "cls", "ul")):
    B = len(z)
    bufs = {"p": guarded_nan(B), "pr": guarded_nan(B, 2), "cls": _guarded(torch.int64, B), "ul": guarded_nan(B)}
    bufs = {k: v for k, v in bufs.items() if k in want}
    dz, dy = dev(z), dev(y)
    ptr = lambda k: _p(bufs[k][1]) if k in bufs else None
    _chk(lib.mi_binary_predictions(_p(dz), _p(dy), B, ptr("p"), ptr("pr"), ptr("cls"), ptr("ul"), _st()))
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs.values())
    return {k: v.cpu().numpy().copy() for k, (_, v) in bufs.items()}


@pytest.mark.parametrize("B", [0, 1, 256, 257, 4097])
def test_binary_predictions_against_fp64(lib, B):
    if B == 0:
        _chk(lib.mi_binary_predictions(None, None, 0, None, None, None, None, _st()))
        return
    z, y = H.logits("wide", B), H.labels("mixed", B, "wide")
    if B == 4097:
        assert all(((z == v) & (np.signbit(z) == np.signbit(v))).any() for v in H.WIDE_VALUES)
    g = _predictions(lib, z, y)
    _, _, per, sig = H.head64(z, y, 1.0)
    err = float(np.max(np.abs(g["p"] - sig)))
    print("HEAD logistic B=%-5d max |p - p64| %.3g = %.2f x 2^-24 (bar P_BAR = %.3g)" % (B, err, err * 2 ** 24, H.P_BAR))
    assert err <= H.P_BAR
    assert np.array_equal(g["pr"][:, 1].view(np.uint32), g["p"].view(np.uint32))
    assert np.array_equal(g["pr"][:, 0], F32(1) - g["p"])
    assert np.array_equal(g["cls"], (g["p"] > F32(0.5)).astype(np.int64)) and not g["cls"][z == 0].any()
    assert np.max(np.abs(g["ul"] - per) / (1 + per)) < 1e-6
    only = _predictions(lib, z, None, want=("p",))
    assert np.array_equal(only["p"].view(np.uint32), g["p"].view(np.uint32))


# ---- mi_eval_accumulate ----------------------------------------------------------------------------------------------------------
class _Counters:
    def __init__(self):
        self.hb, self.hist = _guarded(torch.int64, 2 * 201)
        self.cb, self.counts = _guarded(torch.int64, 8)
        self.sb, self.sums = _guarded(torch.float64, 4)

    def add(self, lib, z, y):
        dz, dy = dev(z), dev(y)
        _chk(lib.mi_eval_accumulate(_p(dz), _p(dy), len(z), _p(self.hist), _p(self.counts), _p(self.sums), _st()))
        torch.cuda.synchronize()
        assert guards_intact(self.hb) and guards_intact(self.cb) and guards_intact(self.sb)
        return self

    def host(self):
        return self.hist.cpu().numpy().reshape(2, 201).copy(), self.counts.cpu().numpy().copy(), self.sums.cpu().numpy().copy()


def _hold_given_p(lib, z, y, what):
    """the whole input: the counters of the logistic mi_binary_predictions reports, by the header's rule; returns that p"""
    p = _predictions(lib, z, None, want=("p",))["p"]
    hist, counts, sums = _Counters().add(lib, z, y).host()
    rh, rc = H.counters_from_p(p, y, H.thresholds64().astype(F32))
    assert np.array_equal(hist, rh) and np.array_equal(counts, rc), what
    assert hist[:, 0].sum() == 0 and hist[:, 200].sum() == 0, what
    _, _, s64, mag = H.eval64(z, y)
    assert sums[2] == float(np.asarray(y, np.int64).sum()) and sums[3] == 0
    assert abs(sums[0] - s64[0]) <= H.SUM_BAR * mag, (what, sums[0], s64[0])
    sp = p.astype(np.float64).sum()
    assert abs(sums[1] - sp) <= H.SUM_BAR * sp, (what, sums[1], sp)
    return p, hist


EVAL_CASES = [(B, w, lab) for B in SMALL_B for w in H.LOGIT_SETS for lab in H.LABEL_SETS] + [(H.BIG, "wide", "mixed")]


@pytest.mark.parametrize("B,which,lab", EVAL_CASES)
def test_eval_counters_equal_fp64_on_the_examples_not_near_a_threshold(lib, B, which, lab):
    z, y = H.logits(which, B), H.labels(lab, B, which)
    close = H.near(z)
    assert close.mean() <= H.NEAR_CAP
    z, y = z[~close], y[~close]                            # an input of its own: nothing is left out after the fact
    assert len(z) >= B - int(H.NEAR_CAP * B) and len(z) > 0
    hist, counts, sums = _Counters().add(lib, z, y).host()
    h64, c64, s64, mag = H.eval64(z, y)
    assert np.array_equal(hist, h64), np.argwhere(hist != h64)[:8].tolist()
    assert np.array_equal(counts, c64), (counts, c64)
    assert hist[:, 0].sum() == 0 and hist[:, 200].sum() == 0
    assert sums[2] == c64[1] and sums[3] == 0
    assert abs(sums[0] - s64[0]) <= H.SUM_BAR * mag, (sums[0], s64[0])
    if B == H.BIG:
        from mi355x_rec.metrics import metrics_from_counters
        from oracle.metrics import BinaryMetrics
        bm = BinaryMetrics()
        for i in range(0, len(z), 16384):
            bm.update(z[i:i + 16384], y[i:i + 16384])
        got, ref = metrics_from_counters(hist, counts, sums), bm.result()
        for k in ref:
            assert abs(got[k] - ref[k]) < 1e-9, (k, got[k], ref[k])


@pytest.mark.parametrize("B,which,lab", EVAL_CASES)
def test_eval_counters_follow_the_header_rule_on_the_reported_logistic(lib, B, which, lab):
    _hold_given_p(lib, H.logits(which, B), H.labels(lab, B, which), (B, which, lab))


def test_eval_midpoints_fill_every_bucket_once(lib):
    z = H.midpoints()
    for lab in (0, 1):
        y = np.full(199, lab, np.uint8)
        hist, counts, _ = _Counters().add(lib, z, y).host()
        assert np.array_equal(hist[lab, 1:200], np.ones(199, np.int64)) and hist[lab, 0] == 0 and hist[lab, 200] == 0
        assert hist[1 - lab].sum() == 0
        h64, c64, _, _ = H.eval64(z, y)                    # (logit 0 is p = 0.5 in every precision: class 0)
        assert np.array_equal(hist, h64) and np.array_equal(counts, c64)


def test_eval_a_logistic_equal_to_a_threshold_is_not_above_it(lib):
    z = np.concatenate([H.tie_sweep(j) for j in range(1, 199)])
    owner = np.repeat(np.arange(1, 199), 4001)
    assert len(z) < 800000
    y = (np.arange(len(z)) % 2).astype(np.uint8)
    p, hist = _hold_given_p(lib, z, y, "ties")
    th = H.thresholds64().astype(F32)
    tied = p == th[owner]
    per_j = np.bincount(owner[tied], minlength=199)
    print("HEAD ties on the device: j=99 %d, j=100 %d, j=198 %d; thresholds with a tie: %d; ties in all: %d"
          % (per_j[99], per_j[100], per_j[198], int((per_j > 0).sum()), int(tied.sum())))
    assert tied.any()                                      # (no tie: the test has lost its point and fails)
    # the tied examples alone, threshold by threshold: bucket j, not j + 1
    tz, ty, tj = z[tied], y[tied], owner[tied]
    hist_t, _, _ = _Counters().add(lib, tz, ty).host()
    ref = np.zeros((2, 201), np.int64)
    np.add.at(ref, (ty.astype(np.int64), tj), 1)
    assert np.array_equal(hist_t, ref), np.argwhere(hist_t != ref)[:8].tolist()


def test_eval_accumulates_across_calls_with_a_64_bit_carry(lib):
    B = 4097
    z, y = H.logits("wide", B), H.labels("mixed", B, "wide")
    whole = _Counters().add(lib, z, y).host()
    halves = _Counters().add(lib, z[:2000], y[:2000]).add(lib, z[2000:], y[2000:]).host()
    assert np.array_equal(whole[0], halves[0]) and np.array_equal(whole[1], halves[1])
    assert abs(whole[2][0] - halves[2][0]) <= H.SUM_BAR * abs(whole[2][0]) and whole[2][2] == halves[2][2]
    # a bin that starts at 2^32 - 1: the add carries into the high word; counts[7] is never written
    y_bin, k_bin = [int(v) for v in np.argwhere(whole[0] == whole[0].max())[0]]
    assert whole[0][y_bin, k_bin] > 1
    c = _Counters()
    c.hist[y_bin * 201 + k_bin] = 2 ** 32 - 1
    c.counts[0] = 2 ** 32 - 1
    c.counts[7] = 12345
    hist, counts, _ = c.add(lib, z[:2000], y[:2000]).add(lib, z[2000:], y[2000:]).host()
    ref = whole[0].copy()
    ref[y_bin, k_bin] += 2 ** 32 - 1
    assert np.array_equal(hist, ref)
    assert counts[0] == 2 ** 32 - 1 + B and counts[7] == 12345 and np.array_equal(counts[1:7], whole[1][1:7])
    for bad in ((None, y), (z, None)):
        c = _Counters()
        assert lib.mi_eval_accumulate(_p(dev(bad[0])), _p(dev(bad[1])), B, _p(c.hist), _p(c.counts), _p(c.sums), _st()) != 0
    assert lib.mi_eval_accumulate(_p(dev(z)), _p(dev(y)), 0, _p(c.hist), _p(c.counts), _p(c.sums), _st()) != 0
    torch.cuda.synchronize()
    assert not c.hist.any() and not c.counts.any()


# ---- mi_layer_stats ----------------------------------------------------------------------------------------------------------------
def _stats(lib, dx, n, ws_bytes=None):
    ob, out = guarded_nan(4)
    wbuf, ws = exact_workspace(lib.mi_layer_stats_workspace_bytes(n) if ws_bytes is None else ws_bytes)
    rc = lib.mi_layer_stats(_p(dx), n, _p(out), _p(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    assert guards_intact(ob) and workspace_surroundings_intact(wbuf, ws)
    return rc, out.cpu().numpy().copy()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4097, H.BIG])
def test_layer_stats_against_fp64(lib, n):
    worst = 0.0
    for name, x in H.stats_sets(n).items():
        for kind, v in (("as drawn", x), ("all negative", -np.abs(x) - 1), ("all zero", np.zeros(n, F32)), ("no zero", np.abs(x) + 1)):
            rc, g = _stats(lib, dev(v), n)
            _chk(rc)
            zf, mn, mx, mean = H.stats64(v)
            assert g[0].view(np.uint32) == zf.view(np.uint32), (name, kind, g[0], zf)
            assert g[1].view(np.uint32) == mn.view(np.uint32) or (g[1] == mn == 0), (name, kind, g[1], mn)
            assert g[2].view(np.uint32) == mx.view(np.uint32) or (g[2] == mx == 0), (name, kind, g[2], mx)
            mag = float(np.abs(v).mean(dtype=np.float64))
            assert abs(float(g[3]) - mean) <= 2e-6 * mag, (name, kind, g[3], mean)
            worst = max(worst, abs(float(g[3]) - mean) / mag if mag else 0.0)
            if kind == "all zero":
                assert g[0] == 1.0
            if kind in ("no zero", "all negative"):
                assert g[0] == 0.0
        if name == "relu":
            assert n < 64 or np.signbit(x[x == 0]).any()                  # -0.0 is there, and counted
        # the extremes, planted in turn at both ends and on both sides of a boundary between two blocks: among positive data,
        # and as the maximum of all-negative data (a running maximum that starts at 0 would report 0)
        neg = -np.abs(x) - 1
        for base, lo, hi in ((x, F32(-1e6), F32(1e6)), (neg, F32(-1e6), F32(-0.5))):
            d = dev(base)
            for pos in H.plant_positions(n):
                for val, slot in ((lo, 1), (hi, 2)):
                    keep = d[pos].clone()
                    d[pos] = float(val)
                    rc, g = _stats(lib, d, n)
                    _chk(rc)
                    assert g[slot] == val, (name, pos, slot, g, val)
                    d[pos] = keep
    print("HEAD layer_stats n=%-8d max |mean - mean64| / mean|x| %.3g (bar 2e-6)" % (n, worst))
    x = H.stats_sets(n)["normal"]
    rc, g = _stats(lib, dev(x), n, ws_bytes=lib.mi_layer_stats_workspace_bytes(n) - 1)
    assert rc == MI_ERR_WORKSPACE and np.isnan(g).all()


# ---- mi_colsum -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("M,N", [(1, 1), (1, 70), (511, 64), (512, 65), (513, 63), (3000, 70), (4097, 257)])
def test_colsum_against_fp64(lib, M, N, pad):
    rng = np.random.default_rng([M, N, pad])
    X = rng.standard_normal((M, N)).astype(F32)
    ld = N + pad
    xb = torch.full((M * ld,), float("nan"), device="cuda")           # (the padding columns are NaN: a read past N shows)
    xb.view(M, ld)[:, :N] = dev(X)
    ob, out = guarded_nan(N)
    need = lib.mi_colsum_workspace_bytes(M, N)
    wbuf, ws = exact_workspace(need)
    _chk(lib.mi_colsum(_p(xb), ld, M, N, _p(out), _p(ws), ws.numel(), _st()))
    torch.cuda.synchronize()
    assert guards_intact(ob) and workspace_surroundings_intact(wbuf, ws)
    ref = X.astype(np.float64).sum(0)
    err = np.abs(out.cpu().numpy() - ref) / np.abs(X).astype(np.float64).sum(0)
    assert np.all(err <= H.TOL), (M, N, pad, float(err.max()))
    ob, out = guarded_nan(N)
    wbuf, ws = exact_workspace(need - 1)
    assert lib.mi_colsum(_p(xb), ld, M, N, _p(out), _p(ws), ws.numel(), _st()) == MI_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and guards_intact(ob) and workspace_surroundings_intact(wbuf, ws)
    wbuf, ws = exact_workspace(need)                                                                     # (enough of it: ldx < N)
    assert lib.mi_colsum(_p(xb), N - 1, M, N, _p(out), _p(ws), ws.numel(), _st()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and guards_intact(ob) and workspace_surroundings_intact(wbuf, ws)


# ---- mi_layer_histogram ----------------------------------------------------------------------------------------------------------
def _hist_data(n, lim):
    """n values: every finite limit as fp32 (on, just under or just over it, as the fp64 limit rounds), the ends of the fp32
    range, denormals and -0.0 first; then test_hip_kernels.py's mixture"""
    rng = np.random.default_rng([n, 23])
    fin = lim[np.abs(lim) < 3e38]
    special = np.concatenate([fin.astype(F32), np.array([np.finfo(F32).max, -np.finfo(F32).max, 3e19, -3e19, 1e-45, -1e-45,
                                                         1e-40, -1e-40, -0.0, 0.0, 1e-13], F32)])
    m = max(n - len(special), 0)
    body = np.concatenate([np.maximum(rng.standard_normal(m - m // 64), 0), -np.abs(rng.standard_normal(m // 64)) * 1e-5]).astype(F32)
    x = np.concatenate([special, rng.permutation(body)])
    return rng.permutation(x)[:n] if n < len(special) else x


def _histogram(lib, x, lim, into=None, expect_ok=True):
    nl = len(lim)
    cb, counts = into[0] if into else _guarded(torch.int64, nl + 1)
    sb, sums = into[1] if into else _guarded(torch.float64, 2)
    dx, dl = dev(x), dev(lim)
    rc = lib.mi_layer_histogram(_p(dx), len(x), _p(dl), nl, _p(counts), _p(sums), _st())
    torch.cuda.synchronize()
    assert guards_intact(cb) and guards_intact(sb)
    if expect_ok:
        _chk(rc)
    return rc, counts.cpu().numpy().copy(), sums.cpu().numpy().copy(), ((cb, counts), (sb, sums))


def _hold_histogram(x, lim, counts, sums):
    x64 = x.astype(np.float64)
    ref = np.bincount(np.searchsorted(lim, x64, side="right"), minlength=len(lim) + 1)
    assert np.array_equal(counts, ref), np.flatnonzero(counts != ref)[:8].tolist()
    assert abs(sums[0] - x64.sum()) <= 1e-6 * np.abs(x64).sum()
    assert abs(sums[1] - (x64 ** 2).sum()) <= 1e-6 * (x64 ** 2).sum()


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 2048 * 1024 + 1])
def test_layer_histogram_against_searchsorted(lib, n):
    from mi355x_rec.metrics import histogram_limits
    lim = histogram_limits()
    if n == 0:
        cb, counts = _guarded(torch.int64, len(lim) + 1)
        _chk(lib.mi_layer_histogram(None, 0, None, len(lim), None, None, _st()))
        _chk(lib.mi_layer_histogram(None, 0, _p(dev(lim)), len(lim), _p(counts), None, _st()))
        torch.cuda.synchronize()
        assert not counts.any() and guards_intact(cb)
        return
    x = _hist_data(n, lim)
    assert len(x) == n and np.isfinite(x).all()
    if n >= 2047:
        on = np.isin(x.astype(np.float64), lim)
        assert on.sum() > 2 and (~on).sum() > 2 and np.signbit(x[x == 0]).any()      # values exactly on a limit, and -0.0
    _, counts, sums, _ = _histogram(lib, x, lim)
    _hold_histogram(x, lim, counts, sums)


def test_layer_histogram_limit_counts_and_accumulation(lib):
    from mi355x_rec.metrics import histogram_limits
    lim = histogram_limits()
    x = _hist_data(5000, lim)
    # two calls add into the same arrays
    _, _, _, into = _histogram(lib, x[:2049], lim)
    _, counts, sums, _ = _histogram(lib, x[2049:], lim, into=into)
    _hold_histogram(x, lim, counts, sums)
    # one limit and 2,048 of them: the ends of the accepted range; 0 and 2,049 are refused and nothing is written
    # (the linear limits are fp32 numbers, and every one of them is in the data: values exactly on a limit go above it)
    for lims in (np.array([0.0]), np.linspace(-4.0, 4.0, 2048).astype(F32).astype(np.float64)):
        v = np.concatenate([x[np.abs(x) < 10], lims.astype(F32)])
        assert np.all(np.diff(lims) > 0) if len(lims) > 1 else True
        _, counts, sums, _ = _histogram(lib, v, lims)
        _hold_histogram(v, lims, counts, sums)
    rc, counts, sums, _ = _histogram(lib, x, np.linspace(-4.0, 4.0, 2049), expect_ok=False)
    assert rc != 0 and not counts.any() and not sums.any()
    cb, c1 = _guarded(torch.int64, 2)
    assert lib.mi_layer_histogram(_p(dev(x)), len(x), _p(dev(lim)), 0, _p(c1), _p(c1), _st()) != 0
    torch.cuda.synchronize()
    assert not c1.any() and guards_intact(cb)
