"""CPU: tests/rows_sort_cases.py itself — the plan table, every reference against a brute-force Python loop and against the
numpy stand-ins of tests/cpu_kernels.py (the routing chain exactly as parallel._route calls it), and the generated key sets
against what their patterns promise."""
import numpy as np
import pytest
import torch

from tests import rows_sort_cases as RC
from tests.cpu_kernels import NumpyKernels

I32 = torch.int32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_the_key_ranges_select_the_nine_plans():
    want = {1: (1, 1), 2: (1, 1), 512: (1, 9), 513: (2, 5), 2 ** 18: (2, 9), 2 ** 18 + 1: (3, 7), 2 ** 27: (3, 9),
            2 ** 27 + 1: (4, 7), 2 ** 31 - 1: (4, 8)}
    assert dict(RC.KEY_RANGES) == want and len(RC.KEY_RANGES) == 9
    for R, p in RC.KEY_RANGES:
        assert RC.plan(R) == p, (R, RC.plan(R), p)
        bits = max(1, int(np.ceil(np.log2(R))))            # the issue's formula, in floating point (exact at these R)
        passes = -(-bits // 9)
        assert p == (passes, -(-bits // passes))
    # the ranges the older tests run, for the record: 1x3, 1x4, 1x9, 2x7, 2x8, 3x9
    assert [RC.plan(R) for R in (7, 10, 300, 4106, 65536, 26_000_000)] == [(1, 3), (1, 4), (1, 9), (2, 7), (2, 8), (3, 9)]
    assert RC.SIZES == [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 12289]


@pytest.mark.parametrize("R", [r for r, _ in RC.KEY_RANGES])
def test_every_key_set_honours_its_range_and_its_pattern(R):
    rng = np.random.default_rng(R % 1000)
    for n in RC.SIZES:
        pats = RC.patterns_for(n, R)
        assert pats[:2] == ["uniform", "constant"]
        assert (len(pats) > 2) == (n in RC.ALL_PATTERNS_AT) and ("distinct" in pats) == (n in RC.ALL_PATTERNS_AT and R >= n)
        for pat in pats:
            k = RC.keys(pat, n, R, rng)
            assert k.dtype == np.int32 and k.shape == (n,) and k.min() >= 0 and int(k.max()) <= R - 1
            U = len(np.unique(k))
            if pat == "uniform" and n >= 2:
                assert k[0] == R - 1 and k[n - 1] == 0
            if pat == "constant":
                assert U == 1 and k[0] == R - 1
            if pat in ("descending", "ascending"):
                d = np.diff(k.astype(np.int64))
                assert np.all(d <= 0) if pat == "descending" else np.all(d >= 0)
                assert not R >= n or U == n                 # strictly monotonic where the range has n keys
                assert 0 in k
            if pat == "mod3":
                assert U == min(3, R, n) and np.array_equal(k[:3], np.minimum(np.arange(3), R - 1)[:n])
            if pat == "distinct":
                assert U == n and 0 in k and R - 1 in k
                assert not np.all(np.diff(k.astype(np.int64)) > 0)          # shuffled


def _brute_sort(rows):
    n = len(rows)
    order = sorted(range(n), key=lambda i: (int(rows[i]), i))
    uniq, seg, slot = [], [], [0] * n
    for k, e in enumerate(order):
        if k == 0 or rows[e] != rows[order[k - 1]]:
            uniq.append(int(rows[e]))
            seg.append(k)
        slot[e] = len(uniq) - 1
    return order, uniq, seg + [n], slot


@pytest.mark.parametrize("n", [1, 2, 65, 200])
@pytest.mark.parametrize("R", [1, 2, 513, 2 ** 31 - 1])
def test_sort_reference_against_a_loop_and_the_stand_ins(n, R):
    rng = np.random.default_rng([n, R % 997])
    k = NumpyKernels()
    for pat in RC.PATTERNS:
        if pat == "distinct" and R < n:
            continue
        rows = RC.keys(pat, n, R, rng)
        ref = RC.sort_reference(rows)
        order, uniq, seg, slot = _brute_sort(rows)
        assert ref.sorted_entry.tolist() == order and ref.uniq.tolist() == uniq and ref.seg_start.tolist() == seg
        assert ref.slot_of_entry.tolist() == slot and ref.U == len(uniq)
        assert all(a.dtype == np.int32 for a in (ref.sorted_entry, ref.uniq, ref.seg_start, ref.slot_of_entry))
        se, uq, sg, sl = (torch.full((n + 1,), RC.FILL, dtype=I32) for _ in range(4))
        nu = torch.full((1,), RC.FILL, dtype=I32)
        k.mi_sort_unique_rows_slots(_t(rows), n, R, se, uq, sg, nu, sl, None, 0)
        U = int(nu[0])
        assert U == ref.U and np.array_equal(se.numpy()[:n], ref.sorted_entry) and np.array_equal(uq.numpy()[:U], ref.uniq)
        assert np.array_equal(sg.numpy()[:U + 1], ref.seg_start) and np.array_equal(sl.numpy()[:n], ref.slot_of_entry)
        se2 = torch.full((n,), RC.FILL, dtype=I32)
        k.mi_sort_unique_rows(_t(rows), n, R, se2, None, None, None, None, 0)
        assert np.array_equal(se2.numpy(), ref.sorted_entry)


def _brute_route(rows, world, self_rank, epc):
    n = len(rows)
    triples = []
    for i in range(n):
        r = int(rows[i])
        owner = r % world
        if self_rank < 0:
            pos = owner
        elif owner == self_rank:
            pos = world - 1
        else:
            pos = owner - 1 if owner > self_rank else owner
        triples.append((i // epc if epc > 0 else 0, pos, r // world))
    req = sorted(set(triples))
    index = {t: u for u, t in enumerate(req)}
    chunks = -(-n // epc) if epc > 0 else 1
    counts = [0] * (chunks * world)
    for c, p, _ in req:
        counts[c * world + p] += 1
    order = sorted(range(n), key=lambda i: (triples[i], i))
    return [index[t] for t in triples], [t[2] for t in req], counts, order


@pytest.mark.parametrize("world", RC.ROUTE_WORLDS)
def test_route_reference_against_a_loop_and_the_chain_of_stand_ins(world):
    """n <= 200; one chunk (epc = 0, as parallel._route passes it), chunks that divide n, and a short last chunk"""
    rng = np.random.default_rng(world)
    k = NumpyKernels()
    R = 211
    Rl = (R + world - 1) // world
    ran = 0
    for self_rank in RC.route_ranks(world):
        for n, epc in ((1, 0), (7, 0), (200, 0), (200, 100), (200, 50), (199, 67), (10, 3)):
            rows = rng.integers(0, R, n).astype(np.int32)
            rows[n // 2] = rows[0]
            ref = RC.route_reference(rows, world, self_rank, epc, Rl)
            slot, send, counts, order = _brute_route(rows, world, self_rank, epc)
            assert ref.slot.tolist() == slot and ref.send_rows.tolist() == send and ref.counts.tolist() == counts
            assert ref.sorted_entry.tolist() == order and ref.U == len(send) == sum(counts)
            assert ref.chunks == (-(-n // epc) if epc else 1)
            # the chain as parallel._route runs it
            n_groups = ref.chunks * world
            key = torch.full((n,), RC.FILL, dtype=I32)
            k.mi_shard_keys(_t(rows), n, world, epc, Rl, self_rank, key)
            se, uq, sg, sl = (torch.full((n + 1,), RC.FILL, dtype=I32) for _ in range(4))
            nu = torch.zeros(1, dtype=I32)
            k.mi_sort_unique_rows_slots(key, n, n_groups * Rl, se, uq, sg, nu, sl, None, 0)
            send_t = torch.full((n,), RC.FILL, dtype=I32)
            counts_t = torch.full((n_groups,), 12345, dtype=I32)
            k.mi_route_requests(uq, nu, n, Rl, n_groups, send_t, counts_t)
            U = int(nu[0])
            assert U == ref.U and np.array_equal(sl.numpy()[:n], ref.slot) and np.array_equal(send_t.numpy()[:U], ref.send_rows)
            assert np.array_equal(counts_t.numpy(), ref.counts) and np.array_equal(se.numpy()[:n], ref.sorted_entry)
            assert bool((send_t[U:] == RC.FILL).all())
            ran += 1
    assert ran == 7 * len(RC.route_ranks(world))


def test_route_cases_hold_what_the_issue_lists():
    assert [RC.route_ranks(w) for w in RC.ROUTE_WORLDS] == [[-1, 0], [-1, 0, 1], [-1, 0, 1, 2], [-1, 0, 4, 7]]
    assert all(RC.ROUTE_R % w for w in RC.ROUTE_WORLDS if w > 1)
    for world in RC.ROUTE_WORLDS:
        cases = RC.route_cases(world)
        assert {c[1] for c in cases} == set(RC.ROUTE_SIZES)
        assert {c[3] for c in cases if c[1] in (1024, 8200) and c[1] % max(c[2], 1) == 0} == {1, 2, 4}
        assert any(c[2] and c[1] % c[2] for c in cases), "no short last chunk"
        assert len(cases) == len(RC.route_ranks(world)) * (1 + 3 + 1 + 1 + 3 + 2)
    rows = RC.route_rows(4097, np.random.default_rng(0))
    assert rows.min() == 0 and rows.max() == RC.ROUTE_R - 1 and len(np.unique(rows)) < 4097


@pytest.mark.parametrize("stride", RC.GAP_STRIDES)
@pytest.mark.parametrize("n_max", [1, 9, 200])
def test_gap_reference_against_a_loop_and_the_stand_in(n_max, stride):
    rng = np.random.default_rng([n_max, stride])
    rows, stamps = RC.gap_case(n_max, stride, rng)
    assert rows.dtype == np.int32 and np.all(np.diff(rows) > 0) and stamps.dtype == np.int32
    if n_max >= len(RC.GAP_STAMPS):
        assert set(stamps[rows.astype(np.int64) * stride].tolist()) == set(RC.GAP_STAMPS)
    step_to = RC.GAP_STEP_TO
    k = NumpyKernels()
    for U in RC.gap_us(n_max):
        key = []
        for i in range(U):
            s = int(stamps[int(rows[i]) * stride])
            key.append(min(step_to - s, 62) if 0 < s < step_to else 0)
        want = [int(rows[i]) for i in sorted(range(U), key=lambda i: (key[i], i))]
        assert RC.gap_reference(rows, U, stamps, stride, step_to).tolist() == want
        if U >= len(RC.GAP_STAMPS):
            assert set(key) == {0, 1, 61, 62}               # 62, 63, 64 and 1,000 steps all clamp to 62
        out = torch.full((n_max,), RC.FILL, dtype=I32)
        last = _t(stamps).as_strided((len(stamps) // stride,), (stride,))
        k.mi_catchup_rows_by_gap(_t(rows), _t(np.array([U], np.int32)), last, n_max, step_to, stride, out, None, 0)
        assert out.numpy()[:U].tolist() == want


@pytest.mark.parametrize("B,vocabs", [(16, [1, 5]), (200, [7, 40000, 3]), (64, [2 ** 30])])
def test_fields_reference_against_a_loop(B, vocabs):
    rng = np.random.default_rng(B)
    ids = RC.field_ids(B, vocabs, rng)
    off = RC.field_offsets(vocabs)
    F = len(vocabs)
    for f, v in enumerate(vocabs):
        assert ids[:, f].min() == 0 and ids[:, f].max() == v - 1
    assert off.tolist() == [sum(vocabs[:f]) for f in range(F)]
    se, uq, sg = [], [], []
    for f in range(F):
        order = sorted(range(B), key=lambda b: (int(ids[b, f]), b))
        for k, b in enumerate(order):
            se.append(b * F + f)
            if k == 0 or ids[b, f] != ids[order[k - 1], f]:
                uq.append(int(off[f]) + int(ids[b, f]))
                sg.append(f * B + k)
    sg.append(B * F)
    got = RC.fields_reference(ids, off)
    assert got[0].tolist() == se and got[1].tolist() == uq and got[2].tolist() == sg
    assert RC.field_vocabs(512) == [512, 512] and RC.field_vocabs(2 ** 30) == [2 ** 30, 1000]
