"""-m gpu: mi_sort_unique_fields(beside = 1) — the short launches that run beside the catch-up: pairs staged in LDS and
written in runs, offsets a tile derives itself, pass 0 reading ids [B][F] in place, the head scan folded into the compaction
— against a host reference (numpy stable argsort per field, np.unique) and against the beside = 0 form of the same input,
bit for bit over the defined ranges: sorted_entry[0..n), uniq_rows[0..U), seg_start[0..U], num_uniq.

Shapes: B = 1, 2 and 3 tiles of 4,096 per field (the "tiles before me" sums have 0, 1 and 2 terms), F = 1, 3, 26.
Vocabularies: 1 (one bin holds the whole tile; stability), 2, 128 | 129 (one | two passes of 7-bit digits), 16,385 (third
pass), 1,000,000, and a mixed list under one shared max_vocab."""
import numpy as np
import pytest
import torch

from tests.util import _chk, _p, _st, dev

pytestmark = pytest.mark.gpu

MIXED = [1_000_000, 2, 129, 16_385, 1, 128]
GUARD = 64
FILL = -7


def _vocabs(kind, F):
    return [MIXED[f % len(MIXED)] for f in range(F)] if kind == "mixed" else [kind] * F


def _ids(pattern, B, vs, rng):
    b = np.arange(B)
    cols = []
    for v in vs:
        if pattern == "uniform":
            c = rng.integers(0, v, B)
        elif pattern == "descending":                      # strictly descending where the vocabulary has B ids
            c = ((B - 1 - b) * v) // B
        elif pattern == "zipf":
            c = np.minimum(rng.zipf(1.05, B) - 1, v - 1)
        else:                                              # long equal runs across wave and tile boundaries once sorted
            c = np.minimum(b % 3, v - 1)
        cols.append(c)
    return np.stack(cols, 1).astype(np.int32)


def _host(ids, off):
    B, F = ids.shape
    se, uq, sg = [], [], []
    for f in range(F):
        order = np.argsort(ids[:, f], kind="stable")
        se.append(order * F + f)
        u, first = np.unique(ids[order, f], return_index=True)
        uq.append(off[f] + u)
        sg.append(f * B + first)
    sg.append(np.array([B * F]))
    return np.concatenate(se).astype(np.int32), np.concatenate(uq).astype(np.int32), np.concatenate(sg).astype(np.int32)


def _run(lib, d_ids, d_off, B, F, max_vocab, beside):
    """the four outputs between guard bands, the workspace of exactly the advertised size inside a patterned buffer"""
    n = B * F
    outs = [torch.full((m + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda") for m in (n, n, n + 1, 1)]
    se, uq, sg, nu = (o[GUARD:-GUARD] for o in outs)
    nbytes = int(lib.mi_sort_unique_fields_workspace_bytes(B, F))
    buf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = buf[256:256 + nbytes]
    assert ws.data_ptr() % 256 == 0
    _chk(lib.mi_sort_unique_fields(_p(d_ids), _p(d_off), B, F, max_vocab, _p(se), _p(uq), _p(sg), _p(nu), _p(ws), nbytes, beside, _st()))
    for o in outs:
        assert bool((o[:GUARD] == FILL).all()) and bool((o[-GUARD:] == FILL).all()), "write outside an output"
    assert bool((buf[:256] == 0xA5).all()) and bool((buf[256 + nbytes:] == 0xA5).all()), "write outside the workspace"
    U = int(nu.item())
    assert 0 < U <= n
    return se.cpu().numpy(), uq[:U].cpu().numpy(), sg[:U + 1].cpu().numpy(), U


@pytest.mark.parametrize("pattern", ["uniform", "descending", "zipf", "mod3"])
@pytest.mark.parametrize("kind", [1, 2, 128, 129, 16_385, 1_000_000, "mixed"])
@pytest.mark.parametrize("F", [1, 3, 26])
@pytest.mark.parametrize("B", [4096, 8192, 12288])
def test_sort_unique_fields_beside_is_the_stable_sort_per_field(lib, B, F, kind, pattern):
    rng = np.random.default_rng([B, F, MIXED.index(kind) if kind in MIXED else 99])
    vs = _vocabs(kind, F)
    ids = _ids(pattern, B, vs, rng)
    off = np.zeros(F, np.int64); off[1:] = np.cumsum(vs)[:-1]
    d_ids, d_off = dev(ids), dev(off)
    ref_se, ref_uq, ref_sg = _host(ids, off)
    got = _run(lib, d_ids, d_off, B, F, max(vs), 1)
    assert got[3] == len(ref_uq)
    assert np.array_equal(got[0], ref_se)
    assert np.array_equal(got[1], ref_uq) and np.array_equal(got[2], ref_sg)
    other = _run(lib, d_ids, d_off, B, F, max(vs), 0)
    assert got[3] == other[3]
    for a, b in zip(got[:3], other[:3]):
        assert np.array_equal(a, b)
    assert torch.equal(d_ids, dev(ids))                    # the ids are read in place, never written


def test_sort_unique_fields_where_bin_scan_makes_the_offsets(lib):
    """nbins x tiles per field above 4,096: the short launches no longer derive a tile's offsets from the raw counts —
    bin_scan_k turns hist into offsets per (field, digit), with segments and seg_len = B, and scatter_runs_k reads them.
    The smallest such shape: B = 9 tiles, vocabulary 200,000 = 18 bits = 2 passes of 9 -> 512 x 9 = 4,608 ints.  Both
    fields uniform, then the second given a single id; both forms, against the host reference."""
    B, F, V = 36_864, 2, 200_000
    rng = np.random.default_rng(36_864)
    ids = _ids("uniform", B, [V, V], rng)
    off = np.array([0, V], np.int64)
    d_off = dev(off)
    for single in (False, True):
        if single:
            ids[:, 1] = 123_456
        d_ids = dev(ids)
        ref_se, ref_uq, ref_sg = _host(ids, off)
        for beside in (0, 1):
            se, uq, sg, U = _run(lib, d_ids, d_off, B, F, V, beside)
            assert U == len(ref_uq)
            assert np.array_equal(se, ref_se)
            assert np.array_equal(uq, ref_uq) and np.array_equal(sg, ref_sg)
        assert torch.equal(d_ids, dev(ids))
