"""CPU: the conditions test_hip_head.py rests on (tests/head_cases.py) — that the examples left out of the exact comparison
of the eval counters are few, that the inputs reach every bucket and every threshold, that the fp64 references agree with the
oracle, and that the numpy stand-ins of the head's entries pass the references the kernels are held to.

oracle.metrics.BinaryMetrics buckets and sums its own fp32 sigmoid, so it is compared with the fp64 references on the not-near
examples only (no near example is ever given to it: there its fp32 bucket and the fp64 one may differ by right), and its
prediction sum cannot agree with the fp64 one to 1e-12 as its loss sum does.  PRED_SUM_BAR(n) = P_BAR sqrt(n) holds the two
together: n roundings of either sign, none above P_BAR — a sum short of one example, or of the wrong examples, is off by the
order of 1, far outside it, where the worst case P_BAR n would hide an error of 0.25 at n = 2^20.  Beside it BinaryMetrics'
sum equals the fp64 sum of the numpy fp32 sigmoid (tests.cpu_kernels.sigmoid32) to 1e-12."""
import numpy as np
import pytest
import torch

from oracle import deepfm as O
from oracle.metrics import BinaryMetrics
from tests import head_cases as H
from tests.cpu_kernels import NumpyKernels, counters, sigmoid32, thresholds

F32 = np.float32
CPU_B = [1, 257, 1025, 4097]                     # the stand-ins: one block, two, several


def PRED_SUM_BAR(n):
    return H.P_BAR * np.sqrt(n)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("which", H.LOGIT_SETS)
@pytest.mark.parametrize("B", H.HEAD_B)
def test_share_of_near_examples_is_small(which, B):
    z = H.logits(which, B)
    share = float(H.near(z).mean())
    print("HEAD near share %-6s B=%-8d %.3g (cap %.2g)" % (which, B, share, H.NEAR_CAP))
    assert share <= H.NEAR_CAP
    if which == "wide" and B >= 4097:               # every fixed value is there, under both labels
        y = H.labels("mixed", B, "wide")
        for v in H.WIDE_VALUES:
            at = (z == v) & (np.signbit(z) == np.signbit(v))
            assert set(y[at].tolist()) == {0, 1}, float(v)


def test_near_marks_the_thresholds_and_a_half_only():
    th = H.thresholds64()
    on = np.log(th[1:199] / (1 - th[1:199])).astype(F32)
    assert H.near(on).all() and H.near(np.array([0.0, -0.0, 1e-30, -1e-30], F32)).all()
    # the middle of bucket 100 is p = 0.5, at the logit 0: a half in every precision, so its class is 0 everywhere
    mid = H.midpoints()
    assert np.flatnonzero(H.near(mid)).tolist() == [99] and mid[99] == 0 and sigmoid32(mid[99:100])[0] == F32(0.5)
    assert not H.near(np.array([88, -88, 104, -104, 1e4, -1e4, 17, -17], F32)).any()       # the outer thresholds do not count


def test_midpoints_fill_buckets_1_to_199_once_each():
    z = H.midpoints()
    assert len(z) == 199
    for hist in (H.eval64(z, np.zeros(199, np.uint8))[0], counters(z, np.zeros(199, np.uint8))[0]):
        assert np.array_equal(hist[0, 1:200], np.ones(199, np.int64)) and hist[0, 0] == 0 and hist[0, 200] == 0
        assert hist[1].sum() == 0


def test_tie_sweeps_contain_exact_ties_above_a_half():
    th = thresholds()
    assert np.array_equal(th.astype(np.float64), H.thresholds64())
    found = {}
    for j in range(1, 199):
        z = H.tie_sweep(j)
        assert len(z) == 4001
        p = sigmoid32(z)
        found[j] = int((p == th[j]).sum())
        assert p.min() < th[j] < p.max(), j                       # the sweep crosses its threshold
    print("HEAD ties per threshold (numpy fp32): j=99 %d, j=100 %d, j=198 %d; thresholds with a tie: %d; ties in all: %d"
          % (found[99], found[100], found[198], sum(v > 0 for v in found.values()), sum(found.values())))
    assert any(found[j] for j in range(100, 199))
    # a tie belongs to bucket j: the number of thresholds strictly below p
    z = H.tie_sweep(100)
    tied = sigmoid32(z) == th[100]
    assert tied.any() and counters(z[tied], np.ones(int(tied.sum()), np.uint8))[0][1, 100] == tied.sum()


@pytest.mark.parametrize("which", H.LOGIT_SETS)
@pytest.mark.parametrize("B", [4097, 65537])
def test_references_agree_with_the_oracle(which, B):
    z, y = H.logits(which, B), H.labels("mixed", B, which)
    keep = ~H.near(z)
    z, y = z[keep], y[keep]
    hist, counts, sums, _ = H.eval64(z, y)
    bm = BinaryMetrics()                                      # (its predictions are fp32: the not-near input)
    for i in range(0, len(z), 16384):
        bm.update(z[i:i + 16384], y[i:i + 16384])
    tail = np.cumsum(hist[:, ::-1], 1)[:, ::-1][:, 1:]        # examples above threshold j: buckets k > j
    assert np.array_equal(tail[1], bm.tp) and np.array_equal(tail[0], bm.fp)
    assert np.array_equal(hist[1].sum() - tail[1], bm.fn) and np.array_equal(hist[0].sum() - tail[0], bm.tn)
    assert counts.tolist() == [bm.n, bm.n_pos, bm.tp5 + bm.fp5, bm.n_correct, bm.tp5, bm.fp5, bm.fn5, 0]
    assert abs(sums[0] - bm.loss_sum) <= 1e-12 * abs(bm.loss_sum)
    assert abs(sums[1] - bm.pred_sum) <= PRED_SUM_BAR(len(z)) and sums[2] == bm.n_pos
    p32 = sigmoid32(z).astype(np.float64).sum()
    assert abs(p32 - bm.pred_sum) <= 1e-12 * p32
    # the head: oracle.deepfm.head's two reductions (2048 examples: the scale 1 / B is the same number in fp32 and fp64)
    x, yy = z[:2048], y[:2048]
    for red, scale in (("mean", 1.0 / 2048), ("sum", 1.0)):
        l, d, per, sig = O.head(x.astype(np.float64), yy, red)
        l64, d64, per64, sig64 = H.head64(x, yy, scale)
        assert abs(l - l64) <= 1e-12 * abs(l) and np.array_equal(d, d64) and np.array_equal(per, per64)
        assert np.array_equal(sig, sig64) and np.array_equal(sig, O.predictions(x.astype(np.float64))["logistic"])


@pytest.mark.parametrize("which", H.LOGIT_SETS)
@pytest.mark.parametrize("B", CPU_B)
def test_head_stand_in_passes_the_reference(which, B):
    k = NumpyKernels()
    z, y = H.logits(which, B), H.labels("mixed", B, which)
    parts, x32 = H.components(z)
    if which == "wide":
        fixed = np.isin(z, H.WIDE_VALUES)
        assert np.array_equal(x32[fixed], z[fixed] + F32(0))
    for scale in (1.0 / B, 1.0):
        logits, loss, dl, ds = torch.empty(B), torch.empty(1), torch.empty(B), torch.empty(1)
        k.mi_sigmoid_ce_head(_t(parts["lin"]), _t(parts["lin_bias"]), _t(parts["fm"]), _t(parts["dnn"]), _t(y), B, scale,
                             logits, loss, dl, ds, None, 0)
        assert np.array_equal(logits.numpy().view(np.uint32), x32.view(np.uint32))
        l64, d64, _, _ = H.head64(x32, y, scale)
        assert np.all(np.abs(dl.numpy() - d64) <= (H.P_BAR + 2.0 ** -24) * float(F32(scale)))
        assert np.isfinite(loss.item()) and abs(loss.item() - l64) <= H.TOL * abs(l64)
        assert abs(ds.item() - d64.sum()) <= H.TOL * np.abs(d64).sum()


@pytest.mark.parametrize("B", CPU_B)
def test_predictions_stand_in_passes_the_reference(B):
    k = NumpyKernels()
    z, y = H.logits("wide", B), H.labels("mixed", B, "wide")
    p, pr, cls, ul = torch.empty(B), torch.empty(B, 2), torch.empty(B, dtype=torch.int64), torch.empty(B)
    k.mi_binary_predictions(_t(z), _t(y), B, p, pr, cls, ul)
    _, _, per, sig = H.head64(z, y, 1.0)
    assert np.max(np.abs(p.numpy() - sig)) <= H.P_BAR
    assert np.array_equal(pr.numpy()[:, 1], p.numpy()) and np.array_equal(pr.numpy()[:, 0], F32(1) - p.numpy())
    assert np.array_equal(cls.numpy(), (p.numpy() > 0.5).astype(np.int64)) and not cls.numpy()[z == 0].any()
    assert np.max(np.abs(ul.numpy() - per) / (1 + per)) < 1e-6


@pytest.mark.parametrize("which,lab", [("normal", "mixed"), ("wide", "mixed"), ("wide", "zeros"), ("wide", "ones")])
@pytest.mark.parametrize("B", CPU_B)
def test_eval_stand_in_and_restatement_pass_the_reference(which, lab, B):
    z, y = H.logits(which, B), H.labels(lab, B, which)
    keep = ~H.near(z)
    z, y = z[keep], y[keep]
    assert len(z) >= B - int(H.NEAR_CAP * B) and len(z) > 0
    hist64, counts64, sums64, mag = H.eval64(z, y)
    hist, counts, sums = torch.zeros(2 * 201, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), torch.zeros(4, dtype=torch.float64)
    NumpyKernels().mi_eval_accumulate(_t(z), _t(y), len(z), hist, counts, sums)
    for h, c, s in ((hist.numpy().reshape(2, 201), counts.numpy(), sums.numpy()), counters(z, y)):
        assert np.array_equal(h, hist64) and np.array_equal(c, counts64)
        assert h[:, 0].sum() == 0 and h[:, 200].sum() == 0
        assert abs(s[0] - sums64[0]) <= H.SUM_BAR * mag and s[2] == sums64[2]
        assert abs(s[1] - sums64[1]) <= PRED_SUM_BAR(len(z))


@pytest.mark.parametrize("n", [1, 1025, 4097])
def test_layer_stats_stand_in_passes_the_reference(n):
    k = NumpyKernels()
    for name, x in H.stats_sets(n).items():
        for v in (x, -np.abs(x) - 1, np.zeros(n, F32), np.abs(x) + 1):          # (as drawn; all negative; all zero; no zero)
            out = torch.empty(4)
            k.mi_layer_stats(_t(v), n, out, None, 0)
            zf, mn, mx, mean = H.stats64(v)
            g = out.numpy()
            assert g[0].view(np.uint32) == zf.view(np.uint32) and g[1] == mn and g[2] == mx, (name, g, zf, mn, mx)
            assert abs(float(g[3]) - mean) <= 2e-6 * np.abs(v).mean(dtype=np.float64), (name, g[3], mean)
    r = H.stats_sets(4097)["relu"]
    assert np.signbit(r[r == 0]).any() and not np.signbit(r[r == 0]).all()
    assert H.partition(1024) == (1, 1024) and H.partition(1025) == (2, 513) and H.partition(H.BIG) == (1024, 1025)
    assert H.BIG - 1023 * 1025 == 2 and H.plant_positions(1025) == [0, 512, 513, 1024]
