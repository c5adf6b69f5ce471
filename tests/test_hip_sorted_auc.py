"""-m gpu: the exact AUC / GAUC counts by sorting (mi_auc_sorted_counts, csrc/auc_sort.hip) through the entry itself, through
ExactAuc(method="sorted") and, end to end, through trainers.deep_fm --exact-auc --gauc-by.

Everything is integers and held to equality (torch.equal) with the brute force over all pairs on the header's key, a few
lines of numpy below, and on the same inputs with mi_auc_pair_counts.  The shapes are the smallest at which a radix sort and
a run count can go wrong: around the wave (64) and around the sort's tile of T keys (read from the source), a few tiles,
logits that land in one bin or differ in the lowest digit only, groups that straddle tiles, group ids that make a third
group digit live, ids outside [0, S)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import HipKernels
from mi355x_rec.exact_auc import ExactAuc
from tests.util import GUARD, ROOT, dev, exact_workspace, workspace_surroundings_intact

pytestmark = pytest.mark.gpu

F32 = np.float32
PATTERN = -0x5A5A5A5A5A5A5A5B


def _tile():
    src = open(os.path.join(ROOT, "recommender-tensorflow_amd", "csrc", "auc_sort.hip")).read()
    block, items = (int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("kBlock", "kItems"))
    assert re.search(r"constexpr int kTile = kBlock \* kItems;", src)
    return block * items


T = _tile()
assert 64 < T <= 4096


# ---- the reference ------------------------------------------------------------------------------------------------------
def key(z):
    """the header's key of fp32 logits: monotone bits, NaN -> 0, -0 as +0"""
    z = np.asarray(z, F32)
    u = z.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[z == 0] = 0x80000000
    k[np.isnan(z)] = 0
    return k


def brute(z, y, seg, S):
    """[S, 2] of one member: every (positive, negative) pair of a group compared; examples outside [0, S) take no part"""
    k = key(z).astype(np.int64)
    seg = np.asarray(seg, np.int64)
    ok = (seg >= 0) & (seg < S)
    pos, neg = np.flatnonzero(ok & (y != 0)), np.flatnonzero(ok & (y == 0))
    out = np.zeros((S, 2), np.int64)
    for c in range(0, len(pos), 1024):
        p = pos[c:c + 1024]
        same = seg[p][:, None] == seg[neg][None, :]
        np.add.at(out[:, 0], seg[p], ((k[p][:, None] > k[neg][None, :]) & same).sum(1))
        np.add.at(out[:, 1], seg[p], ((k[p][:, None] == k[neg][None, :]) & same).sum(1))
    return out


def reference(z, y, seg, S):
    """int64 [M, S, 2] of logits z [M, N]"""
    return torch.from_numpy(np.stack([brute(zm, y, seg, S) for zm in z]))


# ---- logits -------------------------------------------------------------------------------------------------------------
def tied(rng, M, N):
    """heavy ties: five values with +0 and -0 among them, and two NaN per member where there is room"""
    z = rng.choice(np.array([-1.5, -0.0, 0.0, 0.75, 3.0], F32), (M, N))
    if N >= 8:
        for m in range(M):
            z[m, rng.choice(N, 2, replace=False)] = np.nan
    return z


def all_equal(rng, M, N):
    return np.full((M, N), 0.375, F32)


def adjacent(rng, M, N):
    """N distinct neighbouring floats in random order: only the lowest digits of the key separate them"""
    bits = (np.uint32(0x3F800000) + np.arange(N, dtype=np.uint32))
    return np.stack([rng.permutation(bits) for _ in range(M)]).view(F32)


def extremes(rng, M, N):
    vals = np.array([np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 0.0, -0.0, 3e38, -3e38, 1.0, np.nan], F32)
    return rng.choice(vals, (M, N))


def mixed(rng, M, N):
    return rng.normal(0, 2, (M, N)).astype(F32)


KINDS = (tied, all_equal, adjacent, extremes, mixed)


# ---- calls --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k():
    return HipKernels()


def sorted_counts(k, z, y, groups, S, stride=None, into=None, lib=None):
    """z: host [M, N]; the members are laid out `stride` apart (NaN in between); groups: host int32 [N] or None (S = 1).
    The counts lie between guard bands and so does a workspace of exactly the bytes the library asks for.
    -> (the counts' whole buffer, int64 [M, S, 2] on the host)"""
    M, N = z.shape
    stride = stride or N
    flat = torch.full((M * stride,), float("nan"), device="cuda")
    flat.view(M, stride)[:, :N] = dev(z)
    if into is None:
        buf = torch.full((M * S * 2 + 2 * GUARD,), PATTERN, dtype=torch.int64, device="cuda")
        buf[GUARD:-GUARD] = 0
    else:
        buf = into
    out = buf[GUARD:-GUARD].view(M, S, 2)
    nbytes = int((lib or k.lib).mi_auc_sorted_workspace_bytes(N, S))
    assert nbytes >= 16 * N
    wbuf, ws = exact_workspace(nbytes)
    yd, gd = dev(np.ascontiguousarray(y, np.uint8)), (None if groups is None else dev(np.ascontiguousarray(groups, np.int32)))
    if lib is None:
        k.mi_auc_sorted_counts(flat, stride, M, yd, gd, S, N, out, ws, nbytes)
    else:
        _lib.check(lib.mi_auc_sorted_counts(_lib.ptr(flat), stride, M, _lib.ptr(yd), _lib.ptr(gd), S, N, _lib.ptr(out), _lib.ptr(ws),
                                            nbytes, _lib.cur_stream()), "mi_auc_sorted_counts")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())
    assert workspace_surroundings_intact(wbuf, ws)
    return buf, out.cpu()


def pair_counts(k, z, y, seg, S):
    """the same inputs through mi_auc_plan / mi_auc_pair_counts (every seg in [0, S)) -> int64 [M, S, 2] on the host"""
    M, N = z.shape
    seg = np.asarray(seg, np.int64)
    order = np.lexsort((y, seg)).astype(np.int32)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=S))]).astype(np.int64))
    neg = torch.from_numpy(np.bincount(seg[y == 0], minlength=S).astype(np.int64))
    nbytes = int(k.query("mi_auc_plan_bytes", _lib.ptr(off), _lib.ptr(neg), S, 0))
    table = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    plan = _lib.AucPlan()
    k.mi_auc_plan(off, neg, S, 0, table, nbytes, plan)
    out = torch.zeros(M, S, 2, dtype=torch.int64, device="cuda")
    k.mi_auc_pair_counts(plan, dev(z), N, M, dev(order), out)
    return out.cpu()


def labels(rng, N):
    return (rng.random(N) < 0.45).astype(np.uint8)


# ---- one group: sizes around the wave and the tile, every kind of logits ------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_one_group_of_N_examples(k, N):
    rng = np.random.default_rng(N)
    y = labels(rng, N)
    seg = np.zeros(N, np.int64)
    for kind in KINDS:
        z = kind(rng, 1, N)
        want = reference(z, y, seg, 1)
        _, got = sorted_counts(k, z, y, None, 1)
        assert torch.equal(got, want), kind.__name__
        assert torch.equal(pair_counts(k, z, y, seg, 1), want), kind.__name__
    if N >= T:
        assert int(want.sum()) > 0


@pytest.mark.parametrize("N", [1, 65, T + 1])
def test_label_edges(k, N):
    rng = np.random.default_rng(100 + N)
    z = tied(rng, 2, N)
    seg = np.zeros(N, np.int64)
    for only in (0, 1, 255):                                              # one class only: nothing is counted
        assert not bool(sorted_counts(k, z, np.full(N, only, np.uint8), None, 1)[1].any())
    if N > 1:
        for lone in (0, 1):                                               # one positive among negatives, and the reverse
            y = np.full(N, 1 - lone, np.uint8)
            y[N // 3] = lone
            assert torch.equal(sorted_counts(k, z, y, None, 1)[1], reference(z, y, seg, 1))
        y = labels(rng, N)
        y[y == 1] = rng.choice(np.array([1, 2, 255], np.uint8), int((y == 1).sum()))   # non-zero is positive
        assert torch.equal(sorted_counts(k, z, y, None, 1)[1], reference(z, y, seg, 1))


# ---- groups -------------------------------------------------------------------------------------------------------------
def test_one_example_per_group(k):
    N = T + 1
    rng = np.random.default_rng(7)
    seg = rng.permutation(N)
    _, got = sorted_counts(k, tied(rng, 1, N), labels(rng, N), seg, N)
    assert got.shape == (1, N, 2) and not bool(got.any())


def test_groups_of_1_to_130_straddle_the_tiles(k):
    rng = np.random.default_rng(40)
    sizes = np.array([1, 2, 3, 64, 65, 130, 3, 2, 65, 1] * 28)            # 9,408 examples: three tiles
    S = len(sizes)
    seg = np.repeat(np.arange(S), sizes)
    ends = np.cumsum(sizes)
    assert len(seg) > 2 * T and sum(1 for e, n in zip(ends, sizes) if (e - n) // T != (e - 1) // T) >= 2
    y = labels(rng, len(seg))
    y[seg == 3] = 1                                                       # 64 positives alone
    y[seg == 14] = 0                                                      # 65 negatives alone
    mix = rng.permutation(len(seg))
    y, seg = y[mix], seg[mix]
    z = np.concatenate([tied(rng, 1, len(seg)), mixed(rng, 1, len(seg))])
    want = reference(z, y, seg, S)
    assert int((want[:, :, 1] > 0).sum()) > S // 2
    assert torch.equal(sorted_counts(k, z, y, seg, S)[1], want)
    assert torch.equal(pair_counts(k, z, y, seg, S), want)


def test_sparse_group_ids_and_ids_outside_the_range_are_ignored(k):
    """ids up to 70,000 (a third 9-bit group digit is live, most groups are empty); a few ids outside [0, S): those
    examples take no part, and nothing is written outside counts (the guard bands: sorted_counts)"""
    N, S = 5000, 70000
    rng = np.random.default_rng(70)
    seg = rng.choice(rng.choice(S, 300, replace=False), N).astype(np.int64)
    seg[:2] = (S - 1, 0)
    y = labels(rng, N)
    z = tied(rng, 2, N)
    want = reference(z, y, seg, S)
    assert int(want.sum()) > 0 and bool(want[:, 2 ** 16:].any())
    assert torch.equal(sorted_counts(k, z, y, seg, S)[1], want)
    assert torch.equal(pair_counts(k, z, y, seg, S), want)
    bad = seg.copy()
    where = rng.choice(N, 9, replace=False)
    bad[where] = [-1, -5, S, S + 7, 2 ** 31 - 1, -2 ** 31, 2 ** 17, S, -1]
    want_bad = reference(z, y, bad, S)
    assert not torch.equal(want_bad, want)
    assert torch.equal(sorted_counts(k, z, y, bad, S)[1], want_bad)
    # and with one group: an id that is not 0 is outside
    one = np.zeros(N, np.int64)
    one[where] = [1, -1, 2, 5, 2 ** 31 - 1, -2 ** 31, 1, 1, 3]
    assert torch.equal(sorted_counts(k, z, y, one, 1)[1], reference(z, y, one, 1))


# ---- members, repeated calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,pad", [(1, 0), (1, 5), (3, 0), (3, 5)])
def test_members_at_a_stride_and_repeated_calls(k, M, pad):
    N = T + 77
    rng = np.random.default_rng(20 + M + pad)
    y, seg = labels(rng, N), rng.integers(0, 5, N)
    z = np.concatenate([tied(rng, 1, N), mixed(rng, M - 1, N)]) if M > 1 else tied(rng, 1, N)
    want = reference(z, y, seg, 5)
    buf, first = sorted_counts(k, z, y, seg, 5, stride=N + pad)
    assert torch.equal(first, want)
    assert torch.equal(sorted_counts(k, z, y, seg, 5, stride=N + pad)[1], first)      # two calls: equal bits
    _, second = sorted_counts(k, z, y, seg, 5, stride=N + pad, into=buf)               # into NON-zeroed counts: added again
    assert torch.equal(second, 2 * want)
    assert torch.equal(sorted_counts(k, z, y, None, 1, stride=N + pad)[1], reference(z, y, np.zeros(N, np.int64), 1))


# ---- refusals on the device's side: nothing launched, nothing written -----------------------------------------------------
def test_a_short_workspace_is_refused_and_counts_stay(k):
    lib = k.lib
    N = 300
    z = torch.zeros(2, N, device="cuda")
    y = torch.ones(N, dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 1, 2), 7, dtype=torch.int64, device="cuda")
    nbytes = int(lib.mi_auc_sorted_workspace_bytes(N, 1))
    wbuf, ws = exact_workspace(nbytes)
    rc = lib.mi_auc_sorted_counts(_lib.ptr(z), N, 2, _lib.ptr(y), None, 1, N, _lib.ptr(counts), _lib.ptr(ws), nbytes - 1,
                                  _lib.cur_stream())
    assert rc == -4 and "workspace of %d bytes, %d needed" % (nbytes - 1, nbytes) in lib.mi_last_error().decode()
    rc = lib.mi_auc_sorted_counts(_lib.ptr(z), N, 2, _lib.ptr(y), None, 1, N, _lib.ptr(counts), ws.data_ptr() + 8, nbytes,
                                  _lib.cur_stream())
    assert rc == -1 and "16-byte aligned" in lib.mi_last_error().decode()
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((wbuf == 0xA5).all())


# ---- the seam: no count depends on the digit width ------------------------------------------------------------------------
def test_no_count_depends_on_the_digit_width(k, monkeypatch):
    """the tools' build only (make -C recommender-tensorflow_amd/csrc tuning): MI_AUC_SORT_BITS caps the digit width"""
    path = os.path.join(ROOT, "tools", "probe", "libmi355x_rec_tuning.so")
    if not os.path.exists(path):
        pytest.skip("the tools' build of the library is not there (make -C recommender-tensorflow_amd/csrc tuning)")
    lib = C.CDLL(path)
    for name in ("mi_auc_sorted_workspace_bytes", "mi_auc_sorted_counts", "mi_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    N = T + 9
    rng = np.random.default_rng(5)
    y, seg = labels(rng, N), rng.integers(0, 700, N)
    z = np.concatenate([tied(rng, 1, N), adjacent(rng, 1, N)])
    want = reference(z, y, seg, 700)
    for bits in ("9", "8", "5", "3", "1"):
        monkeypatch.setenv("MI_AUC_SORT_BITS", bits)
        assert torch.equal(sorted_counts(k, z, y, seg, 700, lib=lib)[1], want), bits
        assert torch.equal(sorted_counts(k, z[:1], y, None, 1, lib=lib)[1], reference(z[:1], y, np.zeros(N, np.int64), 1)), bits


# ---- through the library --------------------------------------------------------------------------------------------------
def test_exact_auc_sorted_is_exact_auc_pairs():
    N = T + 300
    rng = np.random.default_rng(11)
    y = labels(rng, N)
    users = rng.choice(np.array(["u%03d" % i for i in range(90)]), N)
    z = dev(np.concatenate([tied(rng, 2, N), mixed(rng, 1, N)]))
    a, b = ExactAuc(y, users, device="cuda"), ExactAuc(y, users, device="cuda", method="sorted")
    assert torch.equal(a.counts(z), b.counts(z)) and torch.equal(a.counts(z, grouped=True), b.counts(z, grouped=True))
    assert torch.equal(a.counts(z[1]), b.counts(z[1]))
    assert a.metrics(z) == b.metrics(z) and list(a.group_values) == list(b.group_values)
    _, vals = np.unique(users, return_inverse=True)
    assert torch.equal(b.counts(z, grouped=True).cpu(), reference(z.cpu().numpy(), y, vals.reshape(-1), 90))


def test_deep_fm_reports_the_exact_auc_of_its_evaluation(tmp_path, monkeypatch, capsys):
    """trainers.deep_fm --synthetic 400 --train-steps 20 --exact-auc --gauc-by user_id: auc_exact and gauc are the brute
    force on the logits the evaluation handed to the accumulator"""
    from mi355x_rec import exact_auc
    from trainers import deep_fm
    seen = []
    add = exact_auc.StreamingExactAuc.add

    def recording(self, logits, labels, groups=None):
        seen.append((logits.detach().cpu().numpy().reshape(-1).copy(), labels.detach().cpu().numpy().reshape(-1).copy(),
                     np.asarray(groups).reshape(-1).copy()))
        return add(self, logits, labels, groups)
    monkeypatch.setattr(exact_auc.StreamingExactAuc, "add", recording)
    from trainers import _cli, ml_100k
    opt = ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")
    est = deep_fm.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(
        ["--synthetic", "400", "--train-steps", "20", "--exact-auc", "--gauc-by", "user_id", "--job-dir", str(tmp_path / "job")]))
    out = capsys.readouterr().out
    assert all(" %s = " % name in out for name in ("auc", "auc_exact", "auc_exact_pairs", "gauc", "gauc_groups"))
    del seen[:]
    metrics = est.evaluate(ml_100k.get_input_fn("synthetic:1500:2", "eval", 256))    # users meet again: groups with both classes
    assert len(seen) == 6 and {"auc", "auc_exact", "auc_exact_pairs", "gauc", "gauc_groups"} <= set(metrics)
    z, y, g = (np.concatenate(c) for c in zip(*seen))
    y = (y != 0).astype(np.uint8)
    P, Q = int(y.sum()), int((1 - y).sum())
    gt, eq = brute(z, y, np.zeros(len(z), np.int64), 1)[0]
    assert metrics["auc_exact_pairs"] == P * Q and metrics["auc_exact"] == (2 * int(gt) + int(eq)) / (2 * P * Q)
    values, seg = np.unique(g, return_inverse=True)
    by = brute(z, y, seg.reshape(-1), len(values))
    num = den = 0.0
    n = 0
    for s in range(len(values)):
        p, q = int(y[seg == s].sum()), int((1 - y[seg == s]).sum())
        if p and q:
            num += (p + q) * ((2 * int(by[s, 0]) + int(by[s, 1])) / (2 * p * q))
            den += p + q
            n += 1
    assert n >= 20 and metrics["gauc_groups"] == n and metrics["gauc"] == pytest.approx(num / den, rel=1e-14, abs=0)
