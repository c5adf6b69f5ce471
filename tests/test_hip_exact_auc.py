"""-m gpu: the pair counts of the exact AUC / GAUC for every member in ONE launch (mi_auc_plan / mi_auc_pair_counts,
auc_pair_counts_k in csrc/auc.hip) through the entries themselves, and through mi355x_rec.exact_auc.ExactAuc and
FusedPopulation.evaluate(exact=...).

Everything is integers and held to equality (torch.equal) with the brute force over all pairs on the header's key, a few
lines of numpy below.  The shapes are the smallest at which the kernel can go wrong: around the tile of 64 positives, around
the run of C negatives (the seam set to 64 and 128 so that items split on both axes at a few hundred examples), segments of
1 to 130 examples that straddle tile boundaries, members read at a stride."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import HipKernels
from mi355x_rec.exact_auc import ExactAuc
from mi355x_rec.population import FusedPopulation
from tests.cases import _hip_engine
from tests.util import GUARD, _fresh_ids, dev

pytestmark = pytest.mark.gpu

F32 = np.float32
PATTERN = -0x5A5A5A5A5A5A5A5B


# ---- the reference ------------------------------------------------------------------------------------------------------
def key(z):
    """the header's key of fp32 logits: monotone bits, NaN -> 0, -0 as +0"""
    z = np.asarray(z, F32)
    u = z.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[z == 0] = 0x80000000
    k[np.isnan(z)] = 0
    return k


def brute(z, y):
    p, n = key(z[y == 1])[:, None], key(z[y == 0])[None, :]
    return [int((p > n).sum()), int((p == n).sum())]


def reference(z, y, seg, S):
    """int64 [M, S, 2] of logits z [M, N]"""
    return torch.tensor([[brute(zm[seg == s], y[seg == s]) for s in range(S)] for zm in z], dtype=torch.int64).reshape(len(z), S, 2)


def tied_logits(rng, M, N):
    """heavy ties: five values with +0 and -0 among them, and two NaN per member where there is room"""
    z = rng.choice(np.array([-1.5, -0.0, 0.0, 0.75, 3.0], F32), (M, N))
    if N >= 8:
        for m in range(M):
            z[m, rng.choice(N, 2, replace=False)] = np.nan
    return z


def layout(rng, y, seg, S):
    """order (a real permutation: the examples of a segment's class in random order), seg_off, seg_neg"""
    perm = rng.permutation(len(y))
    order = perm[np.lexsort((y[perm], seg[perm]))].astype(np.int32)
    sizes = np.bincount(seg, minlength=S)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    neg = np.bincount(seg[y == 0], minlength=S).astype(np.int64)
    return order, torch.from_numpy(off), torch.from_numpy(neg)


class Raw:
    """one evaluation set planned through the binding"""

    def __init__(self, k, order, off, neg, run=0):
        self.k, self.S, self.N = k, len(neg), int(off[-1])
        self.off, self.neg = off, neg
        self.order = dev(order)
        nbytes = int(k.query("mi_auc_plan_bytes", _lib.ptr(off), _lib.ptr(neg), self.S, run))
        assert nbytes >= 32 and nbytes % 32 == 0
        self.table = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.plan = _lib.AucPlan()
        k.mi_auc_plan(off, neg, self.S, run, self.table, nbytes, self.plan)
        assert self.plan.N == self.N and self.plan.n_segments == self.S and 32 * max(self.plan.n_items, 1) == nbytes

    def counts(self, z, stride=None, into=None):
        """z: host [M, N]; the members are laid out `stride` apart (NaN in between); int64 [M, S, 2] between guard bands"""
        M = len(z)
        stride = stride or self.N
        flat = torch.full((M * stride,), float("nan"), device="cuda")
        flat.view(M, stride)[:, :self.N] = dev(z)
        if into is None:
            buf = torch.full((M * self.S * 2 + 2 * GUARD,), PATTERN, dtype=torch.int64, device="cuda")
            buf[GUARD:-GUARD] = 0
        else:
            buf = into
        out = buf[GUARD:-GUARD].view(M, self.S, 2)
        self.k.mi_auc_pair_counts(self.plan, flat, stride, M, self.order, out)
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())
        return buf, out.cpu()


def one_segment(rng, P, Q):
    """labels of P positives and Q negatives in random order, one segment"""
    y = np.zeros(P + Q, np.uint8)
    y[rng.choice(P + Q, P, replace=False)] = 1
    return y, np.zeros(P + Q, np.int64)


@pytest.fixture(scope="module")
def k():
    return HipKernels()


# ---- exact equality -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,pad", [(1, 0), (1, 5), (3, 0), (3, 5)])
def test_members_and_strides(k, M, pad):
    rng = np.random.default_rng(20 + M + pad)
    y, seg = one_segment(rng, 140, 117)                                   # N = 257
    raw = Raw(k, *layout(rng, y, seg, 1))
    z = tied_logits(rng, M, 257)
    _, got = raw.counts(z, stride=257 + pad)
    assert torch.equal(got, reference(z, y, seg, 1))
    assert not np.array_equal(raw.order.cpu().numpy(), np.arange(257))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_one_segment_of_N_examples(k, N):
    rng = np.random.default_rng(N)
    y = (rng.random(N) < 0.5).astype(np.uint8)
    raw = Raw(k, *layout(rng, y, np.zeros(N, np.int64), 1))
    for z in (tied_logits(rng, 2, N), rng.normal(0, 1, (2, N)).astype(F32)):
        _, got = raw.counts(z)
        assert torch.equal(got, reference(z, y, np.zeros(N, np.int64), 1))
    # one class only: no items, nothing is counted
    for only in (0, 1):
        y1 = np.full(N, only, np.uint8)
        raw = Raw(k, *layout(rng, y1, np.zeros(N, np.int64), 1))
        assert raw.plan.n_items == 0 and not bool(raw.counts(tied_logits(rng, 2, N))[1].any())


@pytest.mark.parametrize("P", [63, 65, 127, 129])
def test_positives_around_the_tile(k, P):
    rng = np.random.default_rng(P)
    y, seg = one_segment(rng, P, 50)
    raw = Raw(k, *layout(rng, y, seg, 1))
    assert raw.plan.n_items == -(-P // 64)
    z = tied_logits(rng, 2, P + 50)
    assert torch.equal(raw.counts(z)[1], reference(z, y, seg, 1))


@pytest.mark.parametrize("C_", [64, 128])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_negatives_around_the_run(k, C_, d):
    """C - 1, C and C + 1 negatives against 130 positives: the items split on both axes"""
    rng = np.random.default_rng(C_ + d)
    Q = C_ + d
    y, seg = one_segment(rng, 130, Q)
    raw = Raw(k, *layout(rng, y, seg, 1), run=C_)
    assert raw.plan.n_items == 3 * (2 if d == 1 else 1)
    z = tied_logits(rng, 2, 130 + Q)
    assert torch.equal(raw.counts(z)[1], reference(z, y, seg, 1))


def _forty_segments(rng):
    sizes = np.array([1, 2, 3, 64, 65, 130, 3, 2, 65, 1] * 4)
    seg = np.repeat(np.arange(40), sizes)
    y = (rng.random(len(seg)) < 0.45).astype(np.uint8)
    y[seg == 3] = 1                                                       # 64 positives alone
    y[seg == 14] = 0                                                      # 65 negatives alone
    mix = rng.permutation(len(seg))
    return y[mix], seg[mix], sizes


def test_forty_segments_of_mixed_sizes(k):
    rng = np.random.default_rng(40)
    y, seg, sizes = _forty_segments(rng)
    order, off, neg = layout(rng, y, seg, 40)
    assert any(off[s] // 64 != (off[s + 1] - 1) // 64 and 1 < sizes[s] <= 65 for s in range(40))  # small segments straddle multiples of 64
    pos = np.diff(off.numpy()) - neg.numpy()
    assert ((pos == 0) | (neg.numpy() == 0)).sum() >= 6                   # one-class segments (the singletons among them)
    z = np.concatenate([tied_logits(rng, 2, len(y)), rng.normal(0, 1, (1, len(y))).astype(F32)])
    want = reference(z, y, seg, 40)
    for run in (0, 64):
        raw = Raw(k, order, off, neg, run=run)
        buf, got = raw.counts(z, stride=len(y) + 5)
        assert torch.equal(got, want), run


# ---- determinism --------------------------------------------------------------------------------------------------------
def test_counts_do_not_depend_on_the_seam_and_a_second_call_adds_again(k):
    rng = np.random.default_rng(9)
    y, seg = one_segment(rng, 200, 300)
    order, off, neg = layout(rng, y, seg, 1)
    z = tied_logits(rng, 3, 500)
    want = reference(z, y, seg, 1)
    raws = {run: Raw(k, order, off, neg, run=run) for run in (0, 64, 128)}
    assert [raws[r].plan.n_items for r in (0, 64, 128)] == [4, 4 * 5, 4 * 3]
    for raw in raws.values():
        buf, first = raw.counts(z)
        assert torch.equal(first, want)
        assert torch.equal(raw.counts(z)[1], first)                       # twice from zeroed buffers
        _, second = raw.counts(z, into=buf)                               # into NON-zeroed counts: the same numbers again
        assert torch.equal(second, 2 * want)


# ---- refusals: decided on the host, nothing launched, nothing written ---------------------------------------------------
def test_refusals_leave_counts_untouched(k):
    lib = k.lib
    rng = np.random.default_rng(2)
    y, seg = one_segment(rng, 6, 4)
    raw = Raw(k, *layout(rng, y, seg, 1))
    z = torch.zeros(3, 10, device="cuda")
    counts = torch.full((3, 1, 2), 7, dtype=torch.int64, device="cuda")
    err = lambda: lib.mi_last_error().decode()
    stream = _lib.cur_stream()

    def refused(match, p=None, stride=10, M=3, **nulls):
        a = dict(z=z, order=raw.order, counts=counts)
        a.update(nulls)
        p = raw.plan if p is None else p
        rc = lib.mi_auc_pair_counts(C.byref(p) if p is not False else None, _lib.ptr(a["z"]), stride, M, _lib.ptr(a["order"]),
                                    _lib.ptr(a["counts"]), stream)
        assert rc == -1 and match in err(), (rc, err())
    forged = _lib.AucPlan(raw.table.data_ptr(), 0x1234, 10, 1, 1)
    refused("plan (not written by mi_auc_plan)", p=forged)
    refused("plan (not written by mi_auc_plan)", p=_lib.AucPlan())
    refused("plan (not written by mi_auc_plan)", p=False)
    for name in ("z", "order", "counts"):
        refused("logits / order / counts", **{name: None})
    refused("0 members (1 to 1024)", M=0)
    refused("1025 members (1 to 1024)", M=1025)
    refused("member_stride=9 below N=10", stride=9)
    # the plan's refusals: neither the device table nor the plan is written
    table = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)

    def plan_refused(status, match, off, neg, S, run=0, tab=table, nbytes=4096):
        p = _lib.AucPlan()
        rc = lib.mi_auc_plan(_lib.ptr(off), _lib.ptr(neg), S, run, _lib.ptr(tab), nbytes, C.byref(p), stream)
        assert rc == status and match in err(), (rc, err())
        assert p.magic == 0 and p.device_table is None
    ok_off, ok_neg = i64(0, 10), i64(4)
    plan_refused(-1, "seg_off / seg_neg", None, ok_neg, 1)
    plan_refused(-1, "seg_off / seg_neg", ok_off, None, 1)
    plan_refused(-1, "auc_plan: device_table", ok_off, ok_neg, 1, tab=None)
    plan_refused(-1, "0 segments (at least 1)", ok_off, ok_neg, 0)
    plan_refused(-1, "seg_off[0]=1", i64(1, 10), ok_neg, 1)
    plan_refused(-1, "seg_off[2]=5 after seg_off[1]=6", i64(0, 6, 5), i64(1, 0), 2)
    plan_refused(-1, "seg_neg[0]=11 negatives in a segment of 10", ok_off, i64(11), 1)
    plan_refused(-1, "N=0 examples", i64(0, 0), i64(0), 1)
    plan_refused(-1, "N=2147483648 examples", i64(0, 2 ** 31), i64(5), 1)
    plan_refused(-4, "device table of 16 bytes, 32 needed", ok_off, ok_neg, 1, nbytes=16)
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((table == 0xA5).all())


# ---- through the library ------------------------------------------------------------------------------------------------
def test_evaluate_with_exact_is_the_host_formula_on_the_evaluations_logits():
    vocab, N, B = [9, 13, 5], 83, 16
    members = []
    for j in range(3):
        m = _hip_engine(vocab, 4, [8])
        g = torch.Generator(device="cuda")
        g.manual_seed(50 + j)
        m.init_variables(g, lin_scale=0.3)
        members.append(m)
    pop = FusedPopulation(members)
    rng = np.random.default_rng(83)
    ids, y = dev(_fresh_ids(rng, vocab, N)), dev((rng.random(N) < 0.4).astype(np.uint8))
    groups = rng.integers(0, 7, N)
    plain, logits = pop.evaluate(ids, y, batch_size=B, return_logits=True)
    z, yh = logits.cpu().numpy(), y.cpu().numpy()
    ex = ExactAuc(y, groups, device="cuda")
    both = pop.evaluate(ids, y, batch_size=B, exact=ex)
    assert torch.equal(ex.counts(logits), reference(z, yh, np.zeros(N, np.int64), 1).cuda())
    assert torch.equal(ex.counts(logits, grouped=True), reference(z, yh, groups, 7).cuda())
    P, Q = int(yh.sum()), int((1 - yh).sum())
    for i in range(3):
        assert set(both[i]) == set(plain[i]) | {"auc_exact", "auc_exact_pairs", "gauc", "gauc_groups"}
        assert {key_: both[i][key_] for key_ in plain[i]} == plain[i]
        gt, eq = brute(z[i], yh)
        assert both[i]["auc_exact"] == (2 * gt + eq) / (2 * P * Q) and both[i]["auc_exact_pairs"] == P * Q
        num = den = 0.0
        n = 0
        for s in range(7):
            ys = yh[groups == s]
            p, q = int(ys.sum()), int((1 - ys).sum())
            if p and q:
                gt, eq = brute(z[i][groups == s], ys)
                num += (p + q) * ((2 * gt + eq) / (2 * p * q))
                den += p + q
                n += 1
        assert n >= 5 and both[i]["gauc_groups"] == n and both[i]["gauc"] == pytest.approx(num / den, rel=1e-14, abs=0)
    assert pop.evaluate(ids, y, batch_size=B) == plain                    # exact=None: today's keys and values


def test_sweep_counts_its_members_and_its_ensemble(tmp_path):
    """trainers.sweep --exact-auc --gauc-by on the device: the ensemble's numbers are the brute force on its mean logit"""
    from mi355x_rec.predictor import EnsemblePredictor
    from trainers import ml_100k, sweep
    job = str(tmp_path / "sweep")
    sweep.train_and_evaluate(sweep.make_parser().parse_args(
        ["--synthetic", "2000", "--train-steps", "40", "--learning-rate", "0.003", "0.03", "--seeds", "2", "--eval-every", "20",
         "--gauc-by", "gender", "--select", "auc_exact", "--ensemble", "2", "--job-dir", job]))
    doc = json.load(open(os.path.join(job, "sweep.json")))
    rows = doc["members"]
    exacts = [r["metrics"]["auc_exact"] for r in rows]
    assert len(rows) == 4 and exacts == sorted(exacts, reverse=True) and all(r["metrics"]["gauc_groups"] == 2 for r in rows)
    cols, _ = ml_100k._read_csv("synthetic:200:2")                        # the sweep's test file
    y = (cols["rating"] >= 5).astype(np.uint8)
    P, Q = int(y.sum()), int((1 - y).sum())
    assert all(r["metrics"]["auc_exact_pairs"] == P * Q for r in rows)
    ens = EnsemblePredictor.from_sweep(job, top=2)
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    z = ens({k: v for k, v in cols.items() if k in recv})["logits"][:, 0].astype(F32)
    gt, eq = brute(z, y)
    got = doc["ensemble"]["metrics"]
    assert got["auc_exact"] == (2 * gt + eq) / (2 * P * Q) and got["auc_exact_pairs"] == P * Q
    num = den = 0.0
    for v in np.unique(cols["gender"]):
        sel = cols["gender"] == v
        p, q = int(y[sel].sum()), int((1 - y[sel]).sum())
        gt, eq = brute(z[sel], y[sel])
        num += (p + q) * ((2 * gt + eq) / (2 * p * q))
        den += p + q
    assert got["gauc_groups"] == 2 and got["gauc"] == pytest.approx(num / den, rel=1e-14, abs=0)
