"""world_size-2 gloo tests (CPU) of the multi-rank step in mi355x_rec/parallel.py: the REAL routing /
all-to-all / all-reduce plumbing with numpy stand-ins for the device kernels (tests/cpu_kernels.py).

Parity statement: an N-rank synchronous step equals a 1-rank step on the concatenated
batch — mean loss over the global batch, dense gradients summed, sparse gradients dedup-summed at
the row's owner.  The 1-rank side here is the oracle."""
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.util import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, cfg, out_q, device="cpu", backend="gloo"):
    try:
        for p in (ROOT, os.path.join(ROOT, "recommender-tensorflow_amd")):
            if p not in sys.path:
                sys.path.insert(0, p)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        if device != "cpu":
            torch.cuda.set_device(0)
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend, rank=rank, world_size=world)
        from mi355x_rec.engine import DeepFM, OptimizerSpec
        from mi355x_rec.parallel import RowShard
        kernels = None                              # None -> HipKernels (the shipped binding)
        if device == "cpu":
            from tests.cpu_kernels import NumpyKernels
            kernels = NumpyKernels()
        vocab, E, hidden, B, nn, opt_name, lr, steps, flags = cfg[:9]
        chunks = cfg[9] if len(cfg) > 9 else None       # pipeline depth of the step (None: by batch size, 1 here)
        extra = cfg[10] if len(cfg) > 10 else {}        # numeric="raw", lin_opt=(name, lr), reduction="sum": the canned W&D
        p, ids, x, y = _problem(cfg, world)
        lin_opt = OptimizerSpec(*extra["lin_opt"]) if "lin_opt" in extra else None
        m = DeepFM(vocab, n_numeric=nn, embedding_size=E, hidden_units=hidden, use_linear=flags[0], use_mf=flags[1],
                   use_dnn=flags[2], optimizer=OptimizerSpec(opt_name, lr), device=device, shard=RowShard(rank, world, chunks=chunks, chunk_compute=extra.get("chunk_compute"),
                                                                                     route_ahead=extra.get("route_ahead"),
                                                                                     sim_links=extra.get("sim_links")),
                   numeric=extra.get("numeric", "embed"), linear_optimizer=lin_opt, reduction=extra.get("reduction", "mean"),
                   _kernels=kernels, **_subsets(extra))
        m.load_oracle_params(p)
        rng = np.random.default_rng(5)
        losses = []
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
        sl = slice(rank * B, (rank + 1) * B)
        drawn = []
        for _ in range(steps):
            ids_s = _draw_ids(rng, vocab, B * world, extra)
            ids_s[1] = ids_s[0]
            ids_s[B % len(ids_s)] = ids_s[0]         # the same rows requested from both ranks
            drawn.append(t(ids_s[sl]))
        for s_i in range(steps):
            # extra["announce"]: the next step's ids are handed over with this step's (parallel._route_ahead)
            nxt = drawn[s_i + 1] if (extra.get("announce") and s_i + 1 < steps) else None
            loss, logits = m.train_step(drawn[s_i], t(y[sl]), t(None if x is None else x[sl]), next_ids=nxt)
            tot = loss.detach().cpu().clone() if backend == "gloo" else loss.clone()
            dist.all_reduce(tot)
            losses.append((float(tot.item()), logits.cpu().numpy().copy()))
        ev_loss, ev_logits = m.loss(t(ids[rank * B:(rank + 1) * B]), t(y[rank * B:(rank + 1) * B]),
                                    t(None if x is None else x[rank * B:(rank + 1) * B]))
        exported = m.export_numpy()
        exported["exchange"] = dict(m.last_exchange)            # of the eval step: one chunk
        exported["route_ahead_hits"] = getattr(m, "route_ahead_hits", 0)
        exported["second_communicator"] = m.shard.comm.ahead_group is not None
        out_q.put((rank, "ok", losses, exported, ev_logits.cpu().numpy().copy()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:                                  # surface the traceback in the parent
        out_q.put((rank, "error", traceback.format_exc(), None, None))


def _subsets(extra):
    """the canned Wide&Deep's column subsets (engine.DeepFM field_dims / wide_fields / deep_numeric / wide_numeric)"""
    return {k: extra[k] for k in ("field_dims", "wide_fields", "deep_numeric", "wide_numeric") if k in extra}


def _draw_ids(rng, vocab, n, extra):
    """a step's ids: uniform, or (extra["zipf"]) heavily skewed — most entries of a field hit a few hot rows"""
    if extra.get("zipf"):
        return np.stack([np.minimum(rng.geometric(0.35, n) - 1, v - 1) for v in vocab], 1).astype(np.int32)
    return np.stack([rng.integers(0, v, n) for v in vocab], 1).astype(np.int32)


def _problem(cfg, world):
    vocab, E, hidden, B, nn, opt_name, lr, steps, flags = cfg[:9]
    extra = cfg[10] if len(cfg) > 10 else {}
    if extra.get("numeric") == "raw":
        rng = np.random.default_rng(11)
        sub = _subsets(extra)
        p = O.init_params(rng, vocab, E, hidden, n_numeric=nn, dtype=np.float32, lin_scale=0.05, use_dnn=flags[2], numeric="raw",
                          **{k: v for k, v in sub.items() if k != "wide_numeric"})
        if "wide_numeric" in sub:
            p.lin_num[~np.asarray(sub["wide_numeric"], bool)] = 0
        ids = np.stack([rng.integers(0, v, B * world) for v in vocab], 1).astype(np.int32)
        x = rng.standard_normal((B * world, nn)).astype(np.float32)
        y = (rng.random(B * world) < 0.3).astype(np.uint8)
        return p, ids, x, y
    return make_problem(11, vocab, E, hidden, B * world, n_numeric=nn, use_dnn=flags[2])


def _run(cfg, world=2, device="cpu", backend="gloo"):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, cfg, q, device, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        rank, status, a, b, c = q.get(timeout=240)
        assert status == "ok", a
        res[rank] = (a, b, c)
    for p in procs:
        p.join(timeout=60)
    return res


CASES = [
    ([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 3, (True, True, True)),
    ([11, 5, 9], 4, [12], 16, 2, "Adam", 0.001, 2, (True, True, True)),          # numeric columns
    ([7, 6, 5], 4, [8], 16, 0, "Adagrad", 0.05, 2, (True, False, True)),          # no FM, Adagrad
    ([7, 6, 5], 4, [], 16, 0, "Ftrl", 0.1, 2, (True, False, False)),              # wide part only
    # the pipelined form: the local batch in 4 / 2 chunks, row and gradient exchanges per chunk
    ([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 3, (True, True, True), 4),
    ([11, 5, 9], 4, [12], 16, 2, "Adam", 0.001, 2, (True, True, True), 2),
    ([7, 6, 5], 4, [], 16, 0, "Ftrl", 0.1, 2, (True, False, False), 2),
    # BASELINE config 4's model: Wide&Deep with raw numeric columns, Adagrad on the deep part + Ftrl on the
    # wide part, SUM loss (trainers/linear_deep.py:32-39), data-parallel over 2 ranks, 2 chunks
    ([9, 13, 5, 6], 8, [16, 8], 16, 3, "Adagrad", 0.05, 2, (True, False, True), 2,
     dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum")),
]


@pytest.mark.parametrize("cfg", CASES)
def test_two_rank_step_equals_big_batch(cfg):
    check_against_big_batch(cfg, _run(cfg, 2), 2)


def test_next_batch_routed_ahead_equals_big_batch():
    """the routing of batch t + 1 (sorts, count exchange, split sizes to the host) is started during step t
    when its ids are announced — the plan is picked up by the next call (every step but the first), results are those of
    the plain sequence; an evaluation in between drops a plan made ahead instead of overwriting its buffers."""
    cfg = ([9, 13, 5, 6], 8, [16, 8], 32, 0, "Adam", 0.001, 4, (True, True, True), 2, dict(announce=True))
    res = _run(cfg, 2)
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
    check_against_big_batch(cfg, _run(cfg, 2), 2)


def test_four_rank_chunked_exchanges_one_forward():
    cfg = ([9, 13, 5, 6], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(chunk_compute=False))
    check_against_big_batch(cfg, _run(cfg, 4), 4)


@pytest.mark.parametrize("cfg", [
    ([19, 23, 17, 29], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2, dict(announce=True)),
    # BASELINE config 4's model (Wide&Deep, raw numeric columns, Ftrl + Adagrad, SUM loss) — its 8-GPU form
    ([19, 23, 17, 29], 8, [16, 8], 16, 3, "Adagrad", 0.05, 3, (True, False, True), 2,
     dict(numeric="raw", lin_opt=("Ftrl", 0.2), reduction="sum", announce=True))])
def test_eight_rank_default_step_equals_big_batch(cfg):
    """world 8, as the driver's 8-GPU bench runs it: RowShard's defaults from 8 ranks on (chunked exchanges, one MLP pass),
    two chunks, the next batch announced (routing and owner-side sort ahead, on the second communicator) — every rank asks
    7 peers and itself, its own requests last in every chunk."""
    res = _run(cfg, 8)
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
    res = _run(cfg, world)
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
    check_against_big_batch(cfg, _run(cfg, world), world)


def test_packed_exchange_is_refused():
    """RowShard(packed=True), the record exchange that lost its one-rank A/B (profiles/r04_sharded_one_rank.md), is gone."""
    from mi355x_rec.parallel import RowShard
    with pytest.raises(ValueError, match="packed exchange was removed"):
        RowShard(0, 2, packed=True)


def test_four_rank_pipelined_step_equals_big_batch():
    """world 4 (keys chunk * 4 + owner, 4-way splits, some empty): the pipelined step in 2 chunks"""
    cfg = ([9, 13, 5, 6], 8, [16, 8], 16, 0, "Adam", 0.001, 3, (True, True, True), 2)
    check_against_big_batch(cfg, _run(cfg, 4), 4)


def check_against_big_batch(cfg, res, world, tol=1.0):
    vocab, E, hidden, B, nn, opt_name, lr, steps, flags = cfg[:9]
    extra = cfg[10] if len(cfg) > 10 else {}
    numeric, red = extra.get("numeric", "embed"), extra.get("reduction", "mean")
    sub = {k: v for k, v in _subsets(extra).items() if k != "field_dims"}
    # 1-rank reference: the oracle on the concatenated batch
    p, ids, x, y = _problem(cfg, world)
    st = O.TrainState(p, OO.Hyper(opt_name, lr), OO.Hyper(*extra["lin_opt"]) if "lin_opt" in extra else None)
    rng = np.random.default_rng(5)
    for s in range(steps):
        ids_s = _draw_ids(rng, vocab, B * world, extra)
        ids_s[1] = ids_s[0]
        ids_s[B % len(ids_s)] = ids_s[0]
        lo, logit_o = O.train_step(p, st, ids_s, y, x, *flags, reduction=red, numeric=numeric, **sub)
        for r in range(world):
            tot, logits = res[r][0][s]
            assert abs(tot - float(lo)) < tol * (1e-5 * abs(float(lo)) + 1e-7)
            assert np.allclose(logits, logit_o[r * B:(r + 1) * B], rtol=1e-4 * tol, atol=2e-6 * tol)
    tab = np.concatenate([np.pad(a, ((0, 0), (0, E - a.shape[1]))) for a in p.emb], 0)      # (narrower columns: zero pad)
    lw = np.concatenate(p.lin_w, 0)
    # (a column outside linear_feature_columns owns no linear weight: its slots exist, are written and never read)
    owned = np.concatenate([np.full(v, on) for v, on in zip(vocab, extra.get("wide_fields") or [True] * len(vocab))])
    for r in range(world):
        g = res[r][1]
        if g["table"] is not None:
            assert np.max(np.abs(g["table"] - tab[r::world])) < 2e-6 * tol          # this rank's rows only
        if g["lin_w_local"] is not None:
            assert np.max(np.abs(g["lin_w_local"] - lw[r::world])[owned[r::world]]) < 2e-6 * tol
        for i, (k, b) in enumerate(g["mlp"]):
            assert np.max(np.abs(k - p.mlp[i][0])) < 2e-6 * tol and np.max(np.abs(b - p.mlp[i][1])) < 2e-6 * tol
        assert abs(g["lin_bias"][0] - p.lin_bias[0]) < 2e-6 * tol
    # replicated dense variables stay bitwise identical across ranks
    for i in range(len(res[0][1]["mlp"])):
        for r in range(1, world):
            assert np.array_equal(res[0][1]["mlp"][i][0], res[r][1]["mlp"][i][0])
    # sharded eval forward agrees with the oracle forward on the updated variables
    c = O.forward(p, ids, x, *flags, numeric=numeric, **sub)
    for r in range(world):
        assert np.allclose(res[r][2], c["logits"][r * B:(r + 1) * B], rtol=1e-4 * tol, atol=2e-6 * tol)


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
    res = _run(cfg, world)
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
    res = _run(cfg, 2)
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
