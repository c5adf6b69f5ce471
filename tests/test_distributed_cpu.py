"""world_size-2 gloo tests (CPU) of the multi-rank step in mi355x_rec/parallel.py: the REAL routing /
all-to-all / all-reduce plumbing with numpy stand-ins for the device kernels (tests/cpu_kernels.py).

Parity statement: an N-rank synchronous step equals a 1-rank step on the concatenated
batch — mean loss over the global batch, dense gradients summed, sparse gradients dedup-summed at
the row's owner.  The 1-rank side here is the oracle."""
import numpy as np
import pytest
import torch

from tests.cases import DISTRIBUTED_CASES, _problem, _run_ranks, check_against_big_batch

@pytest.mark.parametrize("cfg", DISTRIBUTED_CASES)
def test_two_rank_step_equals_big_batch(cfg):
    check_against_big_batch(cfg, _run_ranks(cfg, 2), 2)


def test_next_batch_routed_ahead_equals_big_batch():
    """the routing of batch t + 1 (sorts, count exchange, split sizes to the host) is started during step t
    when its ids are announced — the plan is picked up by the next call (every step but the first), results are those of
    the plain sequence; an evaluation in between drops a plan made ahead instead of overwriting its buffers."""
    cfg = ([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 4, (True, True, True), 2, dict(announce=True))
    res = _run_ranks(cfg, 2)
    check_against_big_batch(cfg, res, 2)
    assert all(res[r][1]["route_ahead_hits"] == 3 for r in range(2)), [res[r][1]["route_ahead_hits"] for r in range(2)]


@pytest.mark.parametrize("cfg", [
    ([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 3, (True, True, True), 4, dict(chunk_compute=False, announce=True)),
    ([11, 5, 9], 4, [12], 16, 2, "Adam", 0.001, 2, (True, True, True), 2, dict(chunk_compute=False)),          # numeric columns
    ([7, 6, 5], 4, [], 16, 0, "Ftrl", 0.1, 2, (True, False, False), 2, dict(chunk_compute=False)),              # wide part only
    ([9, 13, 5, 6], 8, [16, 8], 16, 3, "Adagrad", 0.05, 2, (True, False, True), 2,
     dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum", chunk_compute=False))])
def test_chunked_exchanges_one_forward_equals_big_batch(cfg):
    """RowShard(chunk_compute=False) — rounds 3-5's default from 8 ranks on (since the rehearsal of profiles/r05_sim_ranks.md an option): the exchanges and the embedding-side kernels run per
    chunk (every chunk's rows served at once, a chunk's embedding kernels behind its own exchange), the MLP once on the
    whole batch, the gradient exchange started from inside the backward (after the input layer's data gradient)."""
    check_against_big_batch(cfg, _run_ranks(cfg, 2), 2)


def test_four_rank_chunked_exchanges_one_forward():
    cfg = ([9, 13, 5, 6], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(chunk_compute=False))
    check_against_big_batch(cfg, _run_ranks(cfg, 4), 4)


@pytest.mark.parametrize("cfg", [
    ([19, 23, 17, 29], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(announce=True)),
    # BASELINE config 4's model (Wide&Deep, raw numeric columns, Ftrl + Adagrad, SUM loss) — its 8-GPU form
    ([19, 23, 17, 29], 8, [16, 8], 16, 3, "Adagrad", 0.05, 3, (True, False, True), 2,
     dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum", announce=True))])
def test_eight_rank_default_step_equals_big_batch(cfg):
    """world 8, as the driver's 8-GPU bench runs it: RowShard's defaults from 8 ranks on (chunked exchanges, one MLP pass),
    two chunks, the next batch announced (routing and owner-side sort ahead, on the second communicator) — every rank asks
    7 peers and itself, its own requests last in every chunk."""
    res = _run_ranks(cfg, 8)
    check_against_big_batch(cfg, res, 8)
    assert all(res[r][1]["route_ahead_hits"] == 2 for r in range(8))
    assert all(res[r][1]["exchange"]["requests_to_self"] <= res[r][1]["exchange"]["requests_sent"] for r in range(8))


@pytest.mark.parametrize("cfg,world", [
    (([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 4, (True, True, True), 2, dict(announce=True, route_ahead=False)), 2),
    (([9, 13, 5, 6], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(chunk_compute=False, announce=True, route_ahead=False)), 4),
    (([19, 23, 17, 29], 8, [16, 8], 16, 3, "Adagrad", 0.05, 3, (True, False, True), 2,
      dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum", announce=True, route_ahead=False)), 8)])
def test_single_communicator_step_equals_big_batch(cfg, world):
    """RowShard(route_ahead=False): the whole step on ONE communicator — no second process group is created; an announced
    next batch is still prepared ahead, with every collective (count exchange, id exchange) on the one communicator in
    program order and only local work (the request sort, the owners' sort) on the side stream (parallel._ahead_in_order) —
    same results; world 2, 4 (chunked exchanges, one MLP pass) and 8 (config 4's model with the 8-rank defaults)."""
    res = _run_ranks(cfg, world)
    check_against_big_batch(cfg, res, world)
    steps = cfg[7]
    assert all(res[r][1]["route_ahead_hits"] == steps - 1 and not res[r][1]["second_communicator"] for r in range(world))


@pytest.mark.parametrize("cfg,world", [
    (([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(announce=True)), 2),
    (([9, 13, 5, 6], 8, [16, 8], 16, 3, "Adagrad", 0.05, 2, (True, False, True), 2,
      dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum", chunk_compute=False)), 2),
    (([9, 13, 5, 6], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(chunk_compute=False)), 4)])
def test_rows_and_wide_weights_exchange_equals_big_batch(cfg, world):
    """A model with an embedding and a wide part: a request's row and its wide weight (and their gradients) travel as two
    arrays, one collective each per chunk and direction.  Same results as the big-batch step."""
    check_against_big_batch(cfg, _run_ranks(cfg, world), world)


def test_packed_exchange_is_refused():
    """RowShard(packed=True), the record exchange that lost its one-rank A/B (profiles/r04_sharded_one_rank.md), is gone."""
    from mi355x_rec.parallel import RowShard
    with pytest.raises(ValueError, match="packed exchange was removed"):
        RowShard(0, 2, packed=True)


def test_four_rank_pipelined_step_equals_big_batch():
    """world 4 (keys chunk * 4 + owner, 4-way splits, some empty): the pipelined step in 2 chunks"""
    cfg = ([9, 13, 5, 6], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2)
    check_against_big_batch(cfg, _run_ranks(cfg, 4), 4)


@pytest.mark.parametrize("world, chunks", [(2, None), (2, 2), (4, None)])
def test_column_subsets_and_per_column_dimensions_on_n_ranks(world, chunks):
    """VERDICT r3 (missing 1): DNNLinearCombinedClassifier with linear_feature_columns != dnn_feature_columns, embedding
    columns of different dimensions and numeric columns that only one part reads (linear_deep.py:32-39 passes two
    independent lists) used to refuse on N GPUs.  Same model as tests/test_canned_parity.py's single-GPU case: Ftrl on the
    linear scope, Adagrad on the dnn scope, SUM loss; N ranks against the oracle on the concatenated batch."""
    cfg = ([9, 13, 5, 6, 7, 11], 8, [16, 8], 16, 3, "Adagrad", 0.05, 3, (True, False, True), chunks,
           dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum", field_dims=[8, 4, 8, 0, 4, 8],
                wide_fields=[True, False, True, True, False, True], deep_numeric=[True, False, True],
                wide_numeric=[True, True, False]))
    res = _run_ranks(cfg, world)
    check_against_big_batch(cfg, res, world)
    for r in range(world):                               # columns of no variable stayed zero through the training
        t = res[r][1]["table"]
        off = np.concatenate([[0], np.cumsum(cfg[0])])
        f_of = np.searchsorted(off, np.arange(off[-1])[r::world], side="right") - 1
        for f, d in enumerate(cfg[10]["field_dims"]):
            assert float(np.abs(t[f_of == f][:, d:]).sum()) == 0.0


def test_skewed_ids_cross_the_link_once_per_distinct_row():
    """VERDICT r1 (7a/7c): rows and gradients travel per DISTINCT row of a chunk, not per (example, field) entry.
    Zipf-like ids, world 2, two chunks: results equal the big-batch oracle, and every rank sends exactly as many
    requests as its batch has distinct (chunk, row) pairs — far fewer than entries."""
    vocab = [50, 40, 30]
    cfg = (vocab, 8, [16, 8], 64, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(zipf=True))
    res = _run_ranks(cfg, 2)
    check_against_big_batch(cfg, res, 2)
    p, ids, x, y = _problem(cfg, 2)                     # the eval batch the workers ran last (one chunk)
    off = np.concatenate([[0], np.cumsum(vocab)])[:-1]
    for r in range(2):
        ex = res[r][1]["exchange"]
        rows = ids[r * 64:(r + 1) * 64].astype(np.int64) + off[None, :]
        assert ex["entries"] == 64 * 3
        assert ex["requests_sent"] == len(np.unique(rows))
    # the hot rows dominate: a small fraction of the entries travels
    assert sum(res[r][1]["exchange"]["requests_sent"] for r in range(2)) < 0.8 * 2 * 64 * 3


def test_row_shard_layout():
    from mi355x_rec.parallel import RowShard
    R = 11
    assert [RowShard(r, 4).local_rows(R) for r in range(4)] == [3, 3, 3, 2]
    with pytest.raises(ValueError):
        RowShard(4, 4)


def test_sharded_initialisers_respect_column_dimensions():
    """init_variables on a rank of N: a column of dimension d has values in its first d columns only, a column outside
    linear_feature_columns zero linear weights — located through the rank's own rows (row r lives on rank r % N at r // N)."""
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    from mi355x_rec.parallel import RowShard
    from tests.cpu_kernels import NumpyKernels
    vocab, dims, wide, world = [9, 13, 5, 6], [8, 4, 0, 8], [True, False, True, True], 3
    off = np.concatenate([[0], np.cumsum(vocab)])
    for rank in range(world):
        m = DeepFM(vocab, n_numeric=0, embedding_size=8, hidden_units=[8], use_linear=True, use_mf=False, use_dnn=True,
                   optimizer=OptimizerSpec("Adagrad", 0.05), device="cpu", shard=RowShard(rank, world), numeric="raw",
                   field_dims=dims, wide_fields=wide, _kernels=NumpyKernels())
        g = torch.Generator(); g.manual_seed(3)
        m.init_variables(g, lin_scale=0.05)
        f_of = np.searchsorted(off, np.arange(off[-1])[rank::world], side="right") - 1
        t, lw = m.table.numpy(), m.lin_w.numpy()
        assert t.shape[0] == len(f_of)
        for f, (d, on) in enumerate(zip(dims, wide)):
            rows = f_of == f
            assert [m._field_rows(f)[1] - m._field_rows(f)[0]] == [int(rows.sum())]
            assert float(np.abs(t[rows][:, d:]).sum()) == 0.0 and (d == 0 or np.all(np.abs(t[rows][:, :d]).sum(1) > 0))
            assert (float(np.abs(lw[rows]).sum()) > 0) == on
