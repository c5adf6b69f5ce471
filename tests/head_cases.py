"""Inputs and fp64 references for the entries of csrc/head.hip — mi_sigmoid_ce_head, mi_binary_predictions, mi_eval_accumulate,
mi_layer_stats, mi_layer_histogram — and mi_colsum: sizes around every block boundary of their launch plans, logits that
saturate, labels of one class, and the rules of include/mi355x_rec.h restated in fp64.  No GPU code and no fixtures; the CPU
half is test_head_cases_cpu.py, the GPU half test_hip_head.py.

The references take the loss, the gradient and the sigmoid from oracle.deepfm.head on fp64 logits, the thresholds from
oracle.metrics.auc_thresholds(), and nothing from tests.cpu_kernels.counters (an fp32 restatement of the kernel, which the
CPU module compares with these).

A kernel's fp32 sigmoid and the fp64 one can fall on different sides of a threshold only where the fp64 one lies within the
error of the fp32 evaluation of it.  P_BAR = 4 * 2^-24 is that error's bar: expf to 1 ulp of a value in (0, 1] (at most 2^-24
absolute), 1 + e and the division half an ulp each of values in [0.5, 2] (2^-24 and 2^-25) — under 3 * 2^-24 together.  near()
marks the examples within P_BAR of one of the 198 inner thresholds or of 0.5; the two outer thresholds, -1e-7 and
fp32(1 + 1e-7), are further than that from every p in [0, 1].  Counts are compared exactly on the examples that are not near."""
import numpy as np

from oracle import deepfm as O
from oracle.metrics import auc_thresholds

F32 = np.float32
TOL = 1e-5                       # test_hip_kernels.py's bar for the head's sums
P_BAR = 4 * 2.0 ** -24
NEAR_CAP = 0.01                  # the largest share of near examples a random logit set may have
SUM_BAR = 2e-10                  # fp64 sums of B <= 2^20 + 1 terms: B * 2^-53 for the order, a few ulp for exp and log1p

# 1024 | 1025: one block becomes two (per = 513); 2^20 + 1: the cap of 1,024 blocks (per = 1025, the last block holds 2)
HEAD_B = [1, 255, 256, 257, 1023, 1024, 1025, 4097, 2 ** 20 + 1]
BIG = 2 ** 20 + 1
LOGIT_SETS = ["normal", "wide"]
LABEL_SETS = ["mixed", "zeros", "ones"]

# the fixed values of the wide set, in an order that gives a short input a bit of everything; entry k of the 32-long
# pattern is value k % 16 with label (k % 2) ^ (k // 16): every value meets both labels, so that max(z, 0) - z y is large
# (z > 0 with y = 0, z < 0 with y = 1) and p - y cancels (the other way round)
WIDE_VALUES = np.array([17, -40, 88, -100, 104, -1e4, 0.0, 1e-30, -17, 40, -88, 100, -104, 1e4, -0.0, -1e-30], F32)
WIDE_STRIDE = 37                 # every 37th example is a fixed value: a quarter of them sit on p = 0.5 (0.7% of the input)


def kernel_blocks(n):
    """head.hip's blocks_for: one block of 256 threads per 1,024 elements, at most 1,024 blocks"""
    return int(min(max(-(-n // 1024), 1), 1024))


def partition(n):
    """(blocks, elements per block) of the head's and the layer statistics' partition: per = ceil(n / blocks)"""
    nb = kernel_blocks(n)
    return nb, -(-n // nb)


def _wide_positions(B):
    pos = np.arange(0, B, WIDE_STRIDE)
    k = np.arange(len(pos)) % 32
    return pos, k


def logits(which, B, seed=0):
    """fp32 logits of a set: "normal" N(0, 2); "wide" the same body with WIDE_VALUES every WIDE_STRIDE examples"""
    rng = np.random.default_rng([B, seed, 11])
    z = (rng.standard_normal(B) * 2).astype(F32)
    if which == "wide":
        pos, k = _wide_positions(B)
        z[pos] = WIDE_VALUES[k % 16]
    else:
        assert which == "normal", which
    return z


def labels(which, B, logit_set="normal", seed=0):
    """uint8 labels: "mixed" (0.3 positive; the wide set's fixed values labelled both ways), "zeros", "ones\""""
    if which == "zeros":
        return np.zeros(B, np.uint8)
    if which == "ones":
        return np.ones(B, np.uint8)
    assert which == "mixed", which
    rng = np.random.default_rng([B, seed, 13])
    y = (rng.random(B) < 0.3).astype(np.uint8)
    if logit_set == "wide":
        pos, k = _wide_positions(B)
        y[pos] = (k % 2) ^ (k // 16)
    return y


def midpoints():
    """199 fp32 logits whose fp64 sigmoid lies in the middle of buckets 1..199 (bucket k: th[k-1] < p <= th[k])"""
    p = (np.arange(1, 200) - 0.5) / 199.0
    return np.log(p / (1 - p)).astype(F32)


def components(z, subset=("lin", "fm", "dnn"), bias=True, seed=0):
    """The head's inputs for target logits z: {"lin", "lin_bias", "fm", "dnn"} (fp32; a part outside `subset` is None) and
    their sum x32 in the header's order, ((lin + bias) + fm) + dnn from 0, in numpy fp32 — the logits the entry must give bit
    for bit.  With all three parts x32 is z to a rounding; where z is one of WIDE_VALUES it is z exactly (lin = -bias, fm = 0)
    — but for -0.0, which no sum that starts at +0 gives.  The references are taken on x32."""
    B = len(z)
    rng = np.random.default_rng([B, seed, 17])
    b = F32(0.25)
    lin = (rng.standard_normal(B) * 0.5).astype(F32)
    fm = rng.standard_normal(B).astype(F32)
    fixed = np.isin(z, WIDE_VALUES)
    lin[fixed] = -b if bias else F32(0)
    fm[fixed] = 0
    head = (lin + (b if bias else F32(0))) + fm
    dnn = (z.astype(np.float64) - head).astype(F32)
    parts = {"lin": lin, "fm": fm, "dnn": dnn}
    x = np.zeros(B, F32)
    if "lin" in subset:
        x = x + (lin + (b if bias else F32(0)))
    if "fm" in subset:
        x = x + fm
    if "dnn" in subset:
        x = x + dnn
    out = {k: (v if k in subset else None) for k, v in parts.items()}
    out["lin_bias"] = np.array([b], F32) if bias else None
    assert x.dtype == F32
    return out, x


# ---- fp64 references ------------------------------------------------------------------------------------------------------------
def head64(x32, y, scale):
    """(loss, d_logit [B], per-example loss [B], sigmoid [B]) in fp64 of fp32 logits: oracle.deepfm.head's sum form, times the
    loss scale the entry is given — a float argument of the ABI, so the fp32 value of `scale`"""
    _, d, per, sig = O.head(np.asarray(x32, F32).astype(np.float64), np.asarray(y), "sum")
    s = float(F32(scale))
    return float(per.sum()) * s, d * s, per, sig


def sigmoid64(z):
    z = np.asarray(z, F32)
    return O.head(z.astype(np.float64), np.zeros(len(z), np.uint8), "sum")[3]


def thresholds64():
    """tf.metrics.auc's 200 thresholds: the fp32 values the predictions are compared with, as fp64"""
    th = auc_thresholds()
    assert th.dtype == F32 and len(th) == 200
    return th.astype(np.float64)


def counters_from_p(p, y, th):
    """hist [2, 201] and counts [8] (int64) as mi_eval_accumulate lays them out, of sigmoids p and thresholds th in one
    precision: bucket #{j : th[j] < p}, class p > 0.5"""
    y = np.asarray(y).astype(np.int64)
    k = np.searchsorted(th, p, side="left")
    hist = np.zeros((2, 201), np.int64)
    np.add.at(hist, (y, k), 1)
    cls = (p > 0.5).astype(np.int64)
    counts = np.array([len(y), y.sum(), cls.sum(), (cls == y).sum(), (cls & y).sum(), (cls & (1 - y)).sum(),
                       ((1 - cls) & y).sum(), 0], np.int64)
    return hist, counts


def eval64(z, y):
    """(hist [2, 201], counts [8], sums [3], sum of |loss terms|) of fp32 logits z: everything from the fp64 sigmoid"""
    _, _, per, sig = head64(z, y, 1.0)
    hist, counts = counters_from_p(sig, y, thresholds64())
    sums = np.array([per.sum(), sig.sum(), float(np.asarray(y, np.int64).sum())])
    return hist, counts, sums, float(np.abs(per).sum())


def near(z):
    """the examples whose fp64 sigmoid lies within P_BAR of an inner threshold (1..198) or of 0.5"""
    p = sigmoid64(z)
    t = np.sort(np.append(thresholds64()[1:199], 0.5))
    i = np.clip(np.searchsorted(t, p), 1, len(t) - 1)
    return np.minimum(np.abs(p - t[i - 1]), np.abs(p - t[i])) <= P_BAR


def tie_sweep(j):
    """the 4,001 consecutive fp32 values centred on fp32(logit(th[j])), ascending"""
    t = thresholds64()[j]
    c = np.array([np.log(t / (1 - t))], F32)
    bits = int(c.view(np.int32)[0])
    k = np.arange(-2000, 2001, dtype=np.int64)
    out = ((bits & 0x7FFFFFFF) + (k if bits >= 0 else -k)).astype(np.uint32) | np.uint32(bits & 0x80000000)
    out = out.view(F32)
    assert np.all(np.diff(out.astype(np.float64)) > 0) and out[2000] == c[0]
    return out


def stats64(x):
    """mi_layer_stats' four numbers: the zero fraction as float32(count / n) (-0.0 is a zero, as under tf.nn.zero_fraction),
    min and max exactly, the mean in fp64"""
    x = np.asarray(x, F32)
    return F32((x == 0).sum() / len(x)), x.min(), x.max(), float(x.astype(np.float64).mean())


def stats_sets(n, seed=0):
    """three inputs of n values: N(0, 1); 1000 + N(0, 1) (the bar on the mean becomes relative); relu output with -0.0 among
    its zeros"""
    rng = np.random.default_rng([n, seed, 19])
    a = rng.standard_normal(n).astype(F32)
    r = np.maximum(rng.standard_normal(n), 0).astype(F32)
    r[(r == 0) & (rng.random(n) < 0.3)] = -0.0
    return {"normal": a, "offset": (1000 + rng.standard_normal(n)).astype(F32), "relu": r}


def plant_positions(n):
    """where a planted extreme must be found: both ends, and both sides of the first boundary between two blocks"""
    nb, per = partition(n)
    pos = [0, n - 1]
    if nb > 1:
        pos += [per - 1, per]
    return sorted(set(pos))
