"""-m gpu: the rows sort, the routing helpers, the gap sort and the untaken branches of the per-field sort (csrc/sort.hip,
csrc/radix.h) against the host references of tests/rows_sort_cases.py, bit for bit over the defined ranges.

Every output sits between 64-element guard bands of -7; the workspace is exactly the advertised size, 256-aligned, inside a
0xA5-patterned buffer with 256 guard bytes on each side; after every call the guards and the input's bits are checked.  Only
the defined ranges are compared: sorted_entry[0..n), uniq_rows[0..U), seg_start[0..U], num_uniq, slot_of_entry[0..n).

a  one test per key range of KEY_RANGES (every digit plan from 1 x 1 to 4 x 8), all SIZES, the three forms of the entry; one
   workspace per size, so every call after a size's first runs on words an earlier sort left behind
b  one workspace sized for 12,289 keys reused for smaller sorts, whose layouts carve it differently
c  mi_shard_keys -> mi_sort_unique_rows_slots -> mi_route_requests (and mi_segment_slots) against a reference made of
   (chunk, place, local row) tuples
d  the routing helpers' edges: the int32 key limit, no request, one request, one group, the last group, a group boundary
   between two workgroups
e  mi_catchup_rows_by_gap, with its argument and with a registered step state
f  mi_sort_unique_fields where no test went: vocabularies of 9, 27, 28, 29 and 30 bits, 256 and 257 tiles per field, more
   than 4,096 tiles
What was found, the case counts and the wall times: profiles/rows_sort_edges.md."""
import numpy as np
import pytest
import torch

from tests import rows_sort_cases as RC
from tests.util import _chk, _p, _st, dev

pytestmark = pytest.mark.gpu

GUARD, FILL, INT32_MAX = RC.GUARD, RC.FILL, RC.INT32_MAX
WS_GUARD = 256


def _banded(m):
    """(whole buffer, the m elements between its guard bands), all FILL"""
    buf = torch.full((m + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + m]


def _bands_intact(buf):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


def _workspace(nbytes):
    """(whole buffer, exactly nbytes of it, 256-aligned), all 0xA5"""
    buf = torch.full((nbytes + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = buf[WS_GUARD:WS_GUARD + nbytes]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == nbytes
    return buf, ws


def _ws_guards_intact(buf):
    return bool((buf[:WS_GUARD] == 0xA5).all()) and bool((buf[-WS_GUARD:] == 0xA5).all())


class Out:
    """one call's outputs: the device views se, uq, sg, nu, sl and bufs, the banded buffers they lie in"""


def _run(lib, rows, R, form, ws=None):
    """One call of the rows sort on host keys `rows`: form "full" (mi_sort_unique_rows), "perm" (uniq_rows = NULL) or "slots"
    (mi_sort_unique_rows_slots).  ws: (buffer, view) of an earlier call to run on; else a fresh exact one.  Asserts the guards
    and the input's bits; returns the outputs."""
    n = len(rows)
    d_rows = dev(rows)
    o = Out()
    o.bufs = [_banded(m) for m in (n, n, n + 1, 1, n)]
    o.se, o.uq, o.sg, o.nu, o.sl = (v for _, v in o.bufs)
    nbytes = int(lib.mi_sort_unique_workspace_bytes(n))
    wbuf, wv = ws if ws is not None else _workspace(nbytes)
    assert wv.numel() >= nbytes
    if form == "full":
        rc = lib.mi_sort_unique_rows(_p(d_rows), n, R, _p(o.se), _p(o.uq), _p(o.sg), _p(o.nu), _p(wv), wv.numel(), _st())
    elif form == "perm":
        rc = lib.mi_sort_unique_rows(_p(d_rows), n, R, _p(o.se), None, _p(o.sg), _p(o.nu), _p(wv), wv.numel(), _st())
    else:
        rc = lib.mi_sort_unique_rows_slots(_p(d_rows), n, R, _p(o.se), _p(o.uq), _p(o.sg), _p(o.nu), _p(o.sl), _p(wv), wv.numel(), _st())
    _chk(rc)
    torch.cuda.synchronize()
    for b, _ in o.bufs:
        assert _bands_intact(b), "write outside an output"
    assert _ws_guards_intact(wbuf), "write outside the workspace"
    assert np.array_equal(d_rows.cpu().numpy(), rows), "the input was written"
    return o


def _check(o, ref, form, what):
    n = len(ref.sorted_entry)
    assert np.array_equal(o.se.cpu().numpy(), ref.sorted_entry), what
    if form == "perm":                                      # nothing else is written
        for t in (o.uq, o.sg, o.nu, o.sl):
            assert bool((t == FILL).all()), what
        return
    U = int(o.nu.item())
    assert U == ref.U, (what, U, ref.U)
    assert np.array_equal(o.uq.cpu().numpy()[:U], ref.uniq), what
    assert np.array_equal(o.sg.cpu().numpy()[:U + 1], ref.seg_start), what
    if form == "slots":
        assert np.array_equal(o.sl.cpu().numpy()[:n], ref.slot_of_entry), what
    else:
        assert bool((o.sl == FILL).all()), what


FORMS = ("full", "perm", "slots")


# ---- a. the rows sort, plan by plan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,plan", RC.KEY_RANGES, ids=["R%d_%dx%d" % (r, p[0], p[1]) for r, p in RC.KEY_RANGES])
def test_rows_sort_under_every_digit_plan(lib, R, plan):
    """every size, its patterns, the three forms — all calls of a size on ONE workspace, patterned before the first: each later
    call (another pattern, another form) finds what the one before left"""
    assert RC.plan(R) == plan
    rng = np.random.default_rng(R % 100_003)
    calls = 0
    for n in RC.SIZES:
        ws = _workspace(int(lib.mi_sort_unique_workspace_bytes(n)))
        for pat in RC.patterns_for(n, R):
            rows = RC.keys(pat, n, R, rng)
            ref = RC.sort_reference(rows)
            for form in FORMS:
                _check(_run(lib, rows, R, form, ws), ref, form, (n, pat, form))
                calls += 1
    # two patterns at 13 sizes, all six at four (five where the range cannot hold n distinct keys), three forms each
    assert calls == 3 * (2 * (len(RC.SIZES) - 4) + sum(6 if R >= n else 5 for n in RC.ALL_PATTERNS_AT))


# ---- b. one dirty workspace across sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_rows_sort_on_a_workspace_other_sizes_left_dirty(lib, form):
    """the layout depends on n: a workspace sized for 12,289 keys holds, for a smaller sort, another sort's keys where its
    histograms and head counts go"""
    ws = _workspace(int(lib.mi_sort_unique_workspace_bytes(12289)))
    rng = np.random.default_rng(12289)
    for n, R, pat in ((12289, INT32_MAX, "uniform"), (1025, 513, "uniform"), (4097, 2, "uniform")):
        rows = RC.keys(pat, n, R, rng)
        _check(_run(lib, rows, R, form, ws), RC.sort_reference(rows), form, (n, R))


# ---- c. the routing chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", RC.ROUTE_WORLDS)
def test_routing_chain_against_tuples(lib, world):
    Rl = (RC.ROUTE_R + world - 1) // world
    rng = np.random.default_rng(world)
    cases = RC.route_cases(world)
    short = 0
    for self_rank, n, epc, chunks in cases:
        rows = RC.route_rows(n, rng)
        ref = RC.route_reference(rows, world, self_rank, epc, Rl)
        assert ref.chunks == chunks
        n_groups = chunks * world
        short += bool(epc and n % epc)
        what = (world, self_rank, n, epc)
        d_rows = dev(rows)
        kbuf, keys = _banded(n)
        _chk(lib.mi_shard_keys(_p(d_rows), n, world, epc, Rl, self_rank, _p(keys), _st()))
        assert _bands_intact(kbuf) and np.array_equal(d_rows.cpu().numpy(), rows), what
        h_keys = keys.cpu().numpy()
        assert h_keys.min() >= 0 and int(h_keys.max()) < n_groups * Rl, what
        o = _run(lib, h_keys, n_groups * Rl, "slots")
        U = int(o.nu.item())
        assert U == ref.U, what
        assert np.array_equal(o.se.cpu().numpy(), ref.sorted_entry), what
        assert np.array_equal(o.sl.cpu().numpy(), ref.slot), what
        o.uq[U:] = INT32_MAX                                # past U: not to be looked at
        sbuf, send = _banded(n)
        cbuf, counts = _banded(n_groups)
        counts.fill_(12345)                                 # the entry zeroes them itself
        _chk(lib.mi_route_requests(_p(o.uq), _p(o.nu), n, Rl, n_groups, _p(send), _p(counts), _st()))
        assert _bands_intact(sbuf) and _bands_intact(cbuf), what
        h_send, h_counts = send.cpu().numpy(), counts.cpu().numpy()
        assert np.array_equal(h_send[:U], ref.send_rows) and np.all(h_send[U:] == FILL), what
        assert np.array_equal(h_counts, ref.counts) and int(h_counts.sum()) == U, what
        lbuf, slot2 = _banded(n)
        _chk(lib.mi_segment_slots(_p(o.sg), _p(o.se), _p(o.nu), n, _p(slot2), _st()))
        assert _bands_intact(lbuf) and np.array_equal(slot2.cpu().numpy(), ref.slot), what
    assert short == 2 * len(RC.route_ranks(world)) and len(cases) == 11 * len(RC.route_ranks(world))


# ---- d. the routing helpers' edges --------------------------------------------------------------------------------------------------
def test_shard_keys_at_the_int32_key_limit(lib):
    """chunks x world x rows_per_rank == INT32_MAX is accepted (one rank, one chunk: the key is the row) and its keys sort under
    num_rows_total = INT32_MAX; 2 chunks x 1 rank x 2^30 rows per rank = 2^31 is refused and writes nothing"""
    n = 4097
    rng = np.random.default_rng(31)
    rows = rng.integers(0, INT32_MAX, n).astype(np.int32)
    rows[5], rows[n - 5], rows[n // 2] = 0, INT32_MAX - 1, INT32_MAX - 1
    d_rows = dev(rows)
    kbuf, keys = _banded(n)
    _chk(lib.mi_shard_keys(_p(d_rows), n, 1, 0, INT32_MAX, 0, _p(keys), _st()))
    assert _bands_intact(kbuf) and np.array_equal(keys.cpu().numpy(), rows)
    ref = RC.sort_reference(rows)
    for form in FORMS:
        _check(_run(lib, keys.cpu().numpy(), INT32_MAX, form), ref, form, form)
    kbuf, keys = _banded(8)
    assert lib.mi_shard_keys(_p(d_rows), 8, 1, 4, 2 ** 30, -1, _p(keys), _st()) != 0
    torch.cuda.synchronize()
    assert bool((kbuf == FILL).all())


def _route(lib, groups, locals_, Rl, n_groups, n_max, U=None):
    """mi_route_requests on the sorted distinct requests (group, local row): (send_rows [n_max], counts [n_groups]) as numpy"""
    groups, locals_ = np.asarray(groups, np.int64), np.asarray(locals_, np.int64)
    U = len(groups) if U is None else U
    k = groups * Rl + locals_
    assert np.all(np.diff(k) > 0) and (len(k) == 0 or k[-1] <= INT32_MAX) and len(k) <= n_max
    buf = np.full(n_max, INT32_MAX, np.int32)
    buf[:len(k)] = k
    sbuf, send = _banded(n_max)
    cbuf, counts = _banded(n_groups)
    counts.fill_(12345)
    d_keys, d_nu = dev(buf), dev(np.array([U], np.int32))
    _chk(lib.mi_route_requests(_p(d_keys), _p(d_nu), n_max, Rl, n_groups, _p(send), _p(counts), _st()))
    torch.cuda.synchronize()
    assert _bands_intact(sbuf) and _bands_intact(cbuf)
    return send.cpu().numpy(), counts.cpu().numpy()


def test_route_requests_edges(lib):
    # no request at all, n_max = 300: counts zeroed, send_rows untouched
    send, counts = _route(lib, [], [], 1000, 6, 300)
    assert np.all(counts == 0) and np.all(send == FILL)
    # ... and with keys in the buffer that *num_uniq == 0 hides
    send, counts = _route(lib, [0, 1, 2], [5, 6, 7], 1000, 6, 300, U=0)
    assert np.all(counts == 0) and np.all(send == FILL)
    # one request, in a middle group
    send, counts = _route(lib, [2], [999], 1000, 4, 300)
    assert counts.tolist() == [0, 0, 1, 0] and send[0] == 999 and np.all(send[1:] == FILL)
    # one group
    loc = np.arange(0, 900, 3)
    send, counts = _route(lib, np.zeros(300, int), loc, 1000, 1, 300)
    assert counts.tolist() == [300] and np.array_equal(send, loc)
    # every request in the last of 64 groups
    loc = np.arange(0, 1000, 2)
    send, counts = _route(lib, np.full(500, 63), loc, 1000, 64, 777)
    assert counts.tolist() == [0] * 63 + [500] and np.array_equal(send[:500], loc) and np.all(send[500:] == FILL)
    # a group boundary exactly between u = 255 and u = 256: the two threads that see it sit in different workgroups
    g = np.r_[np.full(256, 3), np.full(256, 4)]
    loc = np.r_[np.arange(256) + 744, np.arange(256)]
    send, counts = _route(lib, g, loc, 1000, 8, 512)
    assert counts.tolist() == [0, 0, 0, 256, 256, 0, 0, 0] and np.array_equal(send, loc)


# ---- e. the catch-up's order ----------------------------------------------------------------------------------------------------------
def _gap(lib, rows, U, stamps, stride, step_to, n_max):
    d_rows, d_stamps, d_nu = dev(rows), dev(stamps), dev(np.array([U], np.int32))
    obuf, out = _banded(n_max)
    nbytes = int(lib.mi_sort_unique_workspace_bytes(n_max))
    wbuf, ws = _workspace(nbytes)
    _chk(lib.mi_catchup_rows_by_gap(_p(d_rows), _p(d_nu), _p(d_stamps), n_max, step_to, stride, _p(out), _p(ws), nbytes, _st()))
    torch.cuda.synchronize()
    assert _bands_intact(obuf), "write outside rows_out"
    assert _ws_guards_intact(wbuf), "write outside the workspace"
    assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_stamps.cpu().numpy(), stamps)
    return out.cpu().numpy()


@pytest.mark.parametrize("n_max", RC.GAP_NMAX)
def test_catchup_rows_by_gap_with_its_argument_and_with_a_step_state(lib, n_max):
    """rows_out[0..U) = the first U rows in the stable order of their staleness key; then once more with a registered step
    state (step = step_to + 1) and the ARGUMENT 0, which must not matter"""
    step_to = RC.GAP_STEP_TO
    calls = 0
    for stride in RC.GAP_STRIDES:
        rows, stamps = RC.gap_case(n_max, stride, np.random.default_rng([n_max, stride]))
        for U in RC.gap_us(n_max):
            ref = RC.gap_reference(rows, U, stamps, stride, step_to)
            assert np.array_equal(_gap(lib, rows, U, stamps, stride, step_to, n_max)[:U], ref), (n_max, U, stride)
            state = torch.zeros(16, dtype=torch.uint8, device="cuda")
            state.view(torch.int32)[0] = step_to + 1
            _chk(lib.mi_set_step_state(_p(state)))
            try:
                got = _gap(lib, rows, U, stamps, stride, 0, n_max)
            finally:
                _chk(lib.mi_set_step_state(None))
            assert np.array_equal(got[:U], ref), (n_max, U, stride, "step state")
            calls += 2
    assert calls == 2 * 2 * len(RC.gap_us(n_max))


# ---- f. the per-field sort where no test went -----------------------------------------------------------------------------------------
def _fields(lib, d_ids, d_off, B, F, max_vocab, beside, expect_ok=True):
    n = B * F
    bufs = [_banded(m) for m in (n, n, n + 1, 1)]
    se, uq, sg, nu = (v for _, v in bufs)
    nbytes = int(lib.mi_sort_unique_fields_workspace_bytes(B, F))
    wbuf, ws = _workspace(nbytes)
    rc = lib.mi_sort_unique_fields(_p(d_ids), _p(d_off), B, F, max_vocab, _p(se), _p(uq), _p(sg), _p(nu), _p(ws), nbytes, beside, _st())
    torch.cuda.synchronize()
    if not expect_ok:
        assert rc != 0
        assert all(bool((b == FILL).all()) for b, _ in bufs), "a refused call wrote an output"
        assert bool((wbuf == 0xA5).all()), "a refused call wrote the workspace"
        return None
    _chk(rc)
    assert all(_bands_intact(b) for b, _ in bufs), "write outside an output"
    assert _ws_guards_intact(wbuf), "write outside the workspace"
    U = int(nu.item())
    assert 0 < U <= n
    return se.cpu().numpy(), uq[:U].cpu().numpy(), sg[:U + 1].cpu().numpy()


def _fields_case(lib, B, vocabs, max_vocab, forms, seed):
    ids = RC.field_ids(B, vocabs, np.random.default_rng(seed))
    off = RC.field_offsets(vocabs)
    d_ids, d_off = dev(ids), dev(off)
    ref = RC.fields_reference(ids, off)
    got = [_fields(lib, d_ids, d_off, B, len(vocabs), max_vocab, beside) for beside in forms]
    for beside, g in zip(forms, got):
        for a, b, name in zip(g, ref, ("sorted_entry", "uniq_rows", "seg_start")):
            assert np.array_equal(a, b), (name, "beside = %d" % beside)
    for g in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(g, got[0]))
    assert np.array_equal(d_ids.cpu().numpy(), ids)          # read in place, never written


@pytest.mark.parametrize("max_vocab", RC.FIELD_MAX_VOCABS)
def test_sort_unique_fields_up_to_the_vocabulary_limit(lib, max_vocab):
    """9, 27, 28, 29 and 30 bits: one launch per pass plans 7-bit digits up to 28 bits (2, 4 and 4 passes) and 8-bit digits
    above (4 passes), the short launches 9-bit digits — both forms sort everything the range check admits"""
    _fields_case(lib, 4096, RC.field_vocabs(max_vocab), max_vocab, (0, 1), max_vocab % 1009)


@pytest.mark.parametrize("beside", [0, 1])
def test_sort_unique_fields_refuses_a_vocabulary_above_2_to_the_30(lib, beside):
    vocabs = RC.field_vocabs(2 ** 30)
    ids = RC.field_ids(4096, vocabs, np.random.default_rng(30))
    d_ids, d_off = dev(ids), dev(RC.field_offsets(vocabs))
    assert _fields(lib, d_ids, d_off, 4096, 2, 2 ** 30 + 1, beside, expect_ok=False) is None


def test_sort_unique_fields_256_tiles_per_field_wait_for_each_other(lib):
    """beside = 0 at the largest field whose tiles exchange their counts inside one launch"""
    _fields_case(lib, 1_048_576, [1000, 1000], 1000, (0,), 256)


def test_sort_unique_fields_257_tiles_per_field_take_the_short_launches(lib):
    """beside = 0 one tile above that: the short launches, silently"""
    _fields_case(lib, 1_052_672, [1000], 1000, (0,), 257)


def test_sort_unique_fields_above_4096_tiles_scans_the_head_counts(lib):
    """4,160 tiles (F = 64 fields of 65 tiles): compact_k with segments behind scan_small_k, not compact_fields_k; both forms
    (65 tiles per field: beside = 0 is the one-launch-per-pass form, whose compaction waits on 4,159 tiles before the last)"""
    _fields_case(lib, 266_240, [1000] * 64, 1000, (0, 1), 4160)
