"""Case lists that more than one test module parametrises over, and the helpers that build the engines, populations and
multi-rank runs of those cases.  The lists are in the order the test ids were first given in: append, never reorder.
pytest does not rewrite the assertions of this module: every assert here carries its message."""
import os
import socket
import sys
import traceback

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.util import ROOT, make_problem

ML100K_VOCAB = [2, 2, 7, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 2000, 2, 2, 50, 8, 2, 2, 2, 2, 1000, 2, 2, 1000]  # sorted order
VOCAB26 = [30 + 7 * i for i in range(26)]


# ---- single engines ---------------------------------------------------------------------------------------------------------
def _hip_engine(vocab, E, hidden, n_numeric=0, **kw):
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    opt = kw.pop("optimizer", OptimizerSpec("Adam", 0.001))
    kw.setdefault("catchup", "exact")       # (the library's default is "bounded": the tests that mean it say so)
    return DeepFM(vocab, n_numeric=n_numeric, embedding_size=E, hidden_units=hidden, optimizer=opt, **kw)


def _numpy_engine(vocab, E, hidden, k=None, lr=0.001, **kw):
    """an Adam engine on the CPU over the numpy stand-ins `k` (its own instance when None)"""
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    from tests.cpu_kernels import NumpyKernels
    return DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=kw.pop("optimizer", OptimizerSpec("Adam", lr)),
                  device="cpu", _kernels=k if k is not None else NumpyKernels(), **kw)


# ---- optimizers away from TF's defaults: (name, learning rate, constructor arguments of OO.Hyper and OptimizerSpec alike) --------
# Every term of the apply rules that vanishes at the defaults is switched on by one of them: Adam's betas and epsilon, the
# accumulators' initial value, Ftrl's l1 clip and 2 * l2, RMSProp's momentum and decay.
OPTIMIZER_HPARAM_SETS = [
    ("Adam", 0.001, dict(beta1=0.5, beta2=0.9, epsilon=1e-3)),
    ("Adagrad", 0.05, dict(initial_accumulator_value=1e-3)),
    ("Ftrl", 0.05, dict(l1=0.01, l2=0.0)),
    ("Ftrl", 0.05, dict(l1=0.0, l2=0.1)),
    ("Ftrl", 0.05, dict(l1=0.01, l2=0.1, initial_accumulator_value=1.0)),
    ("RMSProp", 0.05, dict(decay=0.99, momentum=0.9, epsilon=1e-6)),
]
OPTIMIZER_HPARAM_IDS = ["%s %s" % (n, " ".join("%s=%g" % kv for kv in kw.items())) for n, _, kw in OPTIMIZER_HPARAM_SETS]


def ftrl_gradients(rng, shape, rows=None):
    """Gradients under which both branches of Ftrl's l1 clip occur in every step: the variables of even rows (`rows`: the row
    each gradient goes to; None: its own index) get gradients of 1e-4 — their `linear` stays inside [-l1, l1] for
    l1 = 0.01 over a few steps, the weight is exactly 0 — those of odd rows gradients of order 1."""
    g = rng.standard_normal(shape).astype(np.float32)
    g[(np.arange(shape if np.isscalar(shape) else shape[0]) if rows is None else rows) % 2 == 0] *= np.float32(1e-4)
    return g


# ---- the one-launch train step ------------------------------------------------------------------------------------------------
# Cases whose oracle trajectory keeps every hidden pre-activation at least 1e-6 away from 0 over the five steps (the
# margin found on the CPU is in the comment; the test asserts it), so that no relu decision can depend on summation order.
TRAJECTORIES = [
    (ML100K_VOCAB, 4, [16, 16], 32, 300),                    # trainers.deep_fm's defaults: 3.1e-4
    (ML100K_VOCAB, 4, [16, 16], 1, 301),                     # 1.0e-2
    (ML100K_VOCAB, 4, [16, 16], 128, 305),                   # 3.4e-5
    (ML100K_VOCAB, 16, [64, 64, 32], 32, 308),               # the top of the envelope: 2.3e-5
    ([9, 13, 5, 6], 8, [16, 8], 64, 301),                    # 7.2e-5
    ([50, 30, 20, 40, 11, 7], 16, [64, 32], 96, 307),        # 2.1e-5
]


FLAGS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, False, True),
         (False, True, True)]


# ---- pair scoring: the model and size cases of test_hip_rank (test_hip_serve takes the models) ----------------------------------
RANK_CASES = [
    # (E, hidden, activation, flags (linear, mf, dnn), U, I)
    (4, [16, 16], "relu", (True, True, True), 37, 1682),
    (4, [16, 16], "relu", (True, True, True), 1, 70001),
    (64, [512, 256, 128], "relu", (True, True, True), 37, 5),
    (64, [512, 256, 128], "tanh", (True, True, True), 1, 33),
    (64, [24, 8], "tanh", (True, True, True), 33, 45),
    (4, [24, 8], "sigmoid", (True, True, True), 5, 1),
    (4, [16, 16], "identity", (True, True, True), 40, 70),
    (64, [], "relu", (True, True, True), 37, 40),
    (4, [], "relu", (True, True, True), 3, 7),
    (64, [64, 32], "sigmoid", (True, True, True), 35, 66),
    (4, [16, 16], "relu", (False, True, True), 20, 30),
    (4, [16, 16], "relu", (True, False, True), 20, 30),
    (4, [16, 16], "relu", (True, True, False), 20, 30),
    (4, [16, 16], "relu", (True, False, False), 20, 30),
    (64, [128], "relu", (False, False, True), 9, 50),
    # MFMA widths that are not multiples of 32, and the <2,2> / <4,4> register tilings
    (64, [512, 200, 48], "relu", (True, True, True), 35, 41),
    (16, [96, 64], "tanh", (True, True, True), 33, 70),
    (16, [128, 100, 40], "sigmoid", (True, True, True), 34, 67),
    (8, [40, 33, 1], "relu", (True, True, True), 3, 29),
]


# ---- the population ---------------------------------------------------------------------------------------------------------
STATE = ("t_rec", "lin_state", "dense", "d_s0", "d_s1", "last_step")


def _spec(E=4, hidden=(16, 16), lr=0.001, beta2=0.999, **kw):
    return dict(E=E, hidden=list(hidden), lr=lr, beta2=beta2, kw=kw)


# the mixed list of the bit tests: members differ in everything a fused step accepts
MIXED = ([_spec(), _spec(16, [64, 64, 32]), _spec(8, [32]), _spec(12, [32, 16])] +
         [_spec(8, [16, 8], use_linear=ul, use_mf=um, use_dnn=ud) for ul, um, ud in FLAGS] +
         [_spec(8, [16, 8], activation=a) for a in ("relu", "sigmoid", "tanh", None)] +
         [_spec(4, [16, 16], dropout=d, seed=11 + i) for i, d in enumerate((0.0, 0.1, 0.25))] +
         [_spec(4, [16, 16], lr=lr) for lr in (0.001, 0.003, 0.01)] +
         [_spec(8, [32, 16], beta2=0.99, dropout=0.1, seed=5), _spec(4, [16], reduction="sum"),
          _spec(16, [64, 32], lr=0.005, dropout=0.25, activation="tanh", seed=77)])


def _spec_engine(spec, vocab=ML100K_VOCAB):
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    return DeepFM(vocab, embedding_size=spec["E"], hidden_units=spec["hidden"], catchup="exact",
                  optimizer=OptimizerSpec("Adam", spec["lr"], beta2=spec["beta2"]), **spec["kw"])


def _fresh(specs, vocab=ML100K_VOCAB):
    """engines of `specs` with variables drawn per member, and the state_dicts they start from"""
    out = []
    for i, s in enumerate(specs):
        m = _spec_engine(s, vocab)
        g = torch.Generator(device="cuda")
        g.manual_seed(100 + i)
        m.init_variables(g, lin_scale=0.05)
        out.append(m)
    return out, [m.state_dict() for m in out]


def _clones(specs, sds, vocab=ML100K_VOCAB):
    out = []
    for s, sd in zip(specs, sds):
        m = _spec_engine(s, vocab)
        m.load_state_dict(sd)
        out.append(m)
    return out


def _same_state(a, b):
    for name in STATE:
        x, z = getattr(a, name), getattr(b, name)
        if x is None and z is None:
            continue
        if not torch.equal(x, z):
            return name
    return None


def _population(engines, sweep_blocks=0):
    from mi355x_rec.population import FusedPopulation
    pop = FusedPopulation(engines)
    pop.SWEEP_BLOCKS = sweep_blocks
    return pop


# (seed of make_problem, E, hidden, learning rate): every hidden pre-activation of the oracle stays >= 1e-6 from 0 over the
# five steps on the batches of default_rng(300) (found on the CPU: 3.1e-4, 2.2e-5, 2.0e-5, 7.9e-5, 1.1e-4, 1.8e-5; asserted)
ORACLE_MEMBERS = [(300, 4, [16, 16], 0.001), (301, 4, [16, 16], 0.01), (308, 16, [64, 64, 32], 0.001), (302, 8, [32], 0.003),
                  (304, 4, [16, 16], 0.003), (305, 12, [32, 16], 0.001)]


def _sweep_args(job, *extra):
    from trainers import sweep
    return sweep.make_parser().parse_args(["--synthetic", "300", "--job-dir", str(job), "--batch-size", "16", "--device", "cpu",
                                           "--hidden-units", "8", "8"] + list(extra))


# ---- the multi-rank step: (vocab, E, hidden, B per rank, numeric columns, optimizer, lr, steps, part flags[, chunks[, extra]]) --
DISTRIBUTED_CASES = [
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


def _run_ranks(cfg, world=2, device="cpu", backend="gloo"):
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
            assert abs(tot - float(lo)) < tol * (1e-5 * abs(float(lo)) + 1e-7), ("loss", s, r, tot, float(lo))
            assert np.allclose(logits, logit_o[r * B:(r + 1) * B], rtol=1e-4 * tol, atol=2e-6 * tol), ("logits", s, r)
    tab = np.concatenate([np.pad(a, ((0, 0), (0, E - a.shape[1]))) for a in p.emb], 0)      # (narrower columns: zero pad)
    lw = np.concatenate(p.lin_w, 0)
    # (a column outside linear_feature_columns owns no linear weight: its slots exist, are written and never read)
    owned = np.concatenate([np.full(v, on) for v, on in zip(vocab, extra.get("wide_fields") or [True] * len(vocab))])
    for r in range(world):
        g = res[r][1]
        if g["table"] is not None:
            assert np.max(np.abs(g["table"] - tab[r::world])) < 2e-6 * tol, ("table", r)     # this rank's rows only
        if g["lin_w_local"] is not None:
            assert np.max(np.abs(g["lin_w_local"] - lw[r::world])[owned[r::world]]) < 2e-6 * tol, ("lin_w", r)
        for i, (k, b) in enumerate(g["mlp"]):
            assert np.max(np.abs(k - p.mlp[i][0])) < 2e-6 * tol and np.max(np.abs(b - p.mlp[i][1])) < 2e-6 * tol, ("mlp", r, i)
        assert abs(g["lin_bias"][0] - p.lin_bias[0]) < 2e-6 * tol, ("lin_bias", r, float(g["lin_bias"][0]), float(p.lin_bias[0]))
    # replicated dense variables stay bitwise identical across ranks
    for i in range(len(res[0][1]["mlp"])):
        for r in range(1, world):
            assert np.array_equal(res[0][1]["mlp"][i][0], res[r][1]["mlp"][i][0]), ("kernel %d differs between ranks 0 and" % i, r)
    # sharded eval forward agrees with the oracle forward on the updated variables
    c = O.forward(p, ids, x, *flags, numeric=numeric, **sub)
    for r in range(world):
        assert np.allclose(res[r][2], c["logits"][r * B:(r + 1) * B], rtol=1e-4 * tol, atol=2e-6 * tol), ("eval logits", r)
