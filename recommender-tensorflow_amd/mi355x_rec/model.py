"""Glue between the Estimator-style surface and the engine: runs one batch in TRAIN / EVAL / PREDICT
mode and returns an EstimatorSpec.  Shared by ``trainers.deep_fm.model_fn`` and the canned
classifiers (``canned.py``).  Reference: the tail of model_fn, ``trainers/deep_fm.py:117-125``
(``head.create_estimator_spec``; the prediction / metric keys are those of SURVEY A.5)."""
import numpy as np
import torch

from . import _lib
from .dataset import DeviceBatch, materialise_group
from .estimator import EstimatorSpec, ModeKeys
from .feature_column import FieldPlan
from .metrics import metrics_from_counters


GRAPH_AUTO_MAX_BATCH = 1024      # from here on nothing in a step is launch-bound (bench.py: the replay is 1-6 % behind eager at B = 65536)


def binary_predictions(logits, kernels):
    """logits [B] -> the head's PREDICT dict (same keys as the TF head): mi_binary_predictions."""
    x = logits.reshape(-1).contiguous()
    B = x.numel()
    p = torch.empty(B, 1, dtype=torch.float32, device=x.device)
    prob = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    cls = torch.empty(B, 1, dtype=torch.int64, device=x.device)
    kernels.mi_binary_predictions(x, None, B, p, prob, cls, None)
    return {"logits": x.reshape(-1, 1), "logistic": p, "probabilities": prob, "class_ids": cls, "classes": cls}


class _EvalCounters:
    def __init__(self, device):
        self.hist = torch.zeros(2 * 201, dtype=torch.int64, device=device)
        self.counts = torch.zeros(8, dtype=torch.int64, device=device)
        self.sums = torch.zeros(4, dtype=torch.float64, device=device)
        self.batch_losses = []

    def reset(self):
        self.hist.zero_(); self.counts.zero_(); self.sums.zero_()
        self.batch_losses = []


def split_sides(plan, query_features, candidate_features):
    """The plan's columns (categorical fields 0..F-1, numeric column j as F + j) on the query side: those whose source
    key is in query_features.  A key in both dicts or in neither is an error."""
    qf = []
    for i, c in enumerate(list(plan.categorical) + list(plan.numeric)):
        inq, inc = c.key in query_features, c.key in candidate_features
        if inq == inc:
            raise ValueError("column %r: its key %r is in %s of the two feature dicts" % (c.name, c.key, "both" if inq else "neither"))
        if inq:
            qf.append(i)
    return qf


def side_inputs(plan, fields, features, device):
    """ids int32 [n, Fx] and numeric values float32 [n, nx] (or None) of one side's columns, ascending field order."""
    if plan.device_mode == "on":         # the side's raw columns to the device, its ids made there (device_transform.py)
        return plan.on_device(device, fields=fields).transform(features)
    F = len(plan.categorical)
    cat = [plan.categorical[f] for f in fields if f < F]
    num = [plan.numeric[f - F] for f in fields if f >= F]
    cols = []
    for c in cat:
        v = np.asarray(c.transform(features))
        if v.size and (v.min() < 0 or v.max() >= c.num_buckets):
            raise ValueError("column %r produced an id outside [0, %d)" % (c.name, c.num_buckets))
        cols.append(v.reshape(-1))
    n = len(cols[0]) if cols else len(num[0].values(features))
    ids = np.ascontiguousarray(np.stack(cols, 1) if cols else np.zeros((n, 0)), np.int32)
    x = np.ascontiguousarray(np.stack([c.values(features) for c in num], 1), np.float32) if num else None
    return torch.from_numpy(ids).to(device), (torch.from_numpy(x).to(device) if x is not None else None)


def recommend_sides(plan, eng, query_features, candidate_features, k, exclude):
    """The engine's top_k on the two sides' raw features and the head's logistic on the result, as numpy: logits [U, k],
    probabilities [U, k], indices [U, k].  Estimator.recommend (a checkpoint) and Predictor.recommend (an export) both
    end here."""
    qf = split_sides(plan, query_features, candidate_features)
    cf = [f for f in range(len(plan.categorical) + len(plan.numeric)) if f not in qf]
    q_ids, q_x = side_inputs(plan, qf, query_features, eng.device)
    c_ids, c_x = side_inputs(plan, cf, candidate_features, eng.device)
    score, idx = eng.top_k(q_ids, c_ids, qf, k, q_x, c_x, exclude=exclude)
    pr = binary_predictions(score.reshape(-1).contiguous(), eng.k)
    return {"logits": score.cpu().numpy(), "probabilities": pr["logistic"].reshape(score.shape).cpu().numpy(),
            "indices": idx.cpu().numpy()}


def rank_targets_sides(plan, engines, query_features, candidate_features, targets, exclude, say=None):
    """The exact ranks of named target candidates on the two sides' raw features, for every engine by its own logit, as
    numpy int32 [M, U, Tmax] (-1: padding, not a candidate, or excluded): ONE engine.target_ranks_group call for the engines
    inside mi_pair_target_ranks' scope (256 a call), DeepFM.target_ranks one by one for the others — say(text) is told so.
    Both sides' ids are transformed once.  Estimator.rank_targets, Predictor.rank_targets and FusedPopulation.rank_targets
    end here."""
    from .engine import target_ranks_group
    qf = split_sides(plan, query_features, candidate_features)
    cf = [f for f in range(len(plan.categorical) + len(plan.numeric)) if f not in qf]
    dev = engines[0].device
    q_ids, q_x = side_inputs(plan, qf, query_features, dev)
    c_ids, c_x = side_inputs(plan, cf, candidate_features, dev)
    inside = [i for i, e in enumerate(engines) if e._top_k_group_limit() is None]
    out = [None] * len(engines)
    for lo in range(0, len(inside), _lib.PAIR_TOPK_GROUP_MAX_MEMBERS):
        who = inside[lo:lo + _lib.PAIR_TOPK_GROUP_MAX_MEMBERS]
        r = target_ranks_group([engines[i] for i in who], q_ids, c_ids, qf, targets, q_x, c_x, exclude=exclude).cpu().numpy()
        for j, i in enumerate(who):
            out[i] = r[j]
    for i, e in enumerate(engines):
        if out[i] is None:
            if say is not None:
                say("member %d: the model has %s: ranked on its own (DeepFM.target_ranks, mode auto)" % (i, e._top_k_group_limit()))
            out[i] = e.target_ranks(q_ids, c_ids, qf, targets, q_x, c_x, exclude=exclude).cpu().numpy()
    return np.stack(out)


def recommend_batch(query_features, candidate_features, k, exclude, params):
    """Estimator.recommend's body: recommend_sides on the estimator's plan and engine."""
    store = params["_store"]
    return recommend_sides(store["plan"], store["engine"], query_features, candidate_features, k, exclude)


def run_batch(features, labels, mode, params, make_engine):
    """make_engine(plan, device) -> engine.DeepFM; called once, the result lives in params['_store']."""
    store = params.setdefault("_store", {})
    if "engine" not in store:
        plan = FieldPlan(params.get("categorical_columns", []), params.get("numeric_columns", []))
        device = params.get("device", "cuda")
        plan.set_device_mode(params.get("device_transform", "off"))
        store["plan"] = plan
        shard = params.get("_shard")           # parallel.RowShard of a multi-GPU launch (trainers/_cli.py), else None
        dd = params.get("device_dataset", "off")
        if dd not in ("off", "on"):
            raise ValueError("device_dataset must be 'off' or 'on'")
        if shard is not None and (dd == "on" or isinstance(features, DeviceBatch)):
            raise ValueError("device_dataset=on: one GPU only — a RowShard run takes the plain input pipeline")
        eng = store["engine"] = make_engine(plan, device, shard) if shard is not None else make_engine(plan, device)
        gen = torch.Generator(device=eng.device)
        gen.manual_seed(int(params.get("seed", 0)) + (0 if shard is None else 7919 * shard.rank))
        eng.init_variables(gen)                # TF initialisers; a checkpoint restore overrides
        if shard is not None:
            from .parallel import broadcast_dense
            broadcast_dense(eng)               # the replicated MLP starts identical on every rank
        store["counters"] = None
    if mode == "_build":
        return None
    plan, eng = store["plan"], store["engine"]
    dev = eng.device
    ahead = params.get("_ahead")
    # params["device_transform"] = "on": the batch's raw columns go to the device and become ids there in one launch
    # (mi_ids_transform), bit for bit the host transform's; "off" (the default): the host transform and a copy of its ids
    on_device = plan.device_mode == "on"
    if ahead is not None and mode == ModeKeys.TRAIN and ahead.get("features") is features:
        # small batches (Estimator.train groups them): the id transforms of a whole group of batches were done in one
        # call and copied to the device once; this batch is rows lo..hi of the group
        g = ahead["group"]
        if "ids" not in g and "handles" in g:
            # a dataset on the device: the group's rows are formed there in one launch, the batches are views of them
            (g["ids"], g["x"], g["y"]), g["status"] = materialise_group(g["handles"], plan, eng)
        elif "ids" not in g:
            if on_device:
                g["ids"], g["x"] = plan.on_device(dev, eng.k).transform(g["features"])
            else:
                ids_np, x_np = plan.transform(g["features"])
                g["ids"] = torch.from_numpy(ids_np).to(dev)
                g["x"] = torch.from_numpy(x_np).to(dev) if x_np is not None else None
            g["y"] = torch.from_numpy(np.ascontiguousarray(np.asarray(g["labels"]).reshape(-1)).astype(np.uint8)).to(dev)
        if g.get("status") is not None:
            g.pop("status").raise_if_bad()
        lo, hi = ahead["rows"]
        ids, y = g["ids"][lo:hi], g["y"][lo:hi]
        x = g["x"][lo:hi] if g["x"] is not None else None
    else:
        def stage(f, l):
            """(ids, x, y, status): status is None on the host transform, which has checked its ids; the device transform's
            is looked at when the batch is used (TransformStatus.raise_if_bad: it waits for its own status copy only).  A
            handle of a dataset on the device (dataset.py) is materialised there: one launch, or views of the resident arrays"""
            if isinstance(f, DeviceBatch):
                return f.materialise(plan, eng)
            y_ = None
            if l is not None:
                y_ = torch.from_numpy(np.ascontiguousarray(np.asarray(l).reshape(-1)).astype(np.uint8)).to(dev)
            if on_device:
                ids_, x_, st = plan.on_device(dev, eng.k).transform(f, check=False)
                return (ids_, x_, y_), st
            ids_np, x_np = plan.transform(f)
            return (torch.from_numpy(ids_np).to(dev), torch.from_numpy(x_np).to(dev) if x_np is not None else None, y_), None
        staged = store.pop("staged", None)          # this batch, transformed and copied a step ago (Estimator._with_lookahead)
        if staged is not None and staged[0] is features and mode == ModeKeys.TRAIN:
            (ids, x, y), status = staged[1]
        else:
            (ids, x, y), status = stage(features, labels)
        if status is not None:
            status.raise_if_bad()

    # multi-GPU: a rank's loss is its SHARE of the global-batch mean (already divided by the global batch); times
    # world = the mean over its own examples — what is logged, and, with every rank evaluating the same batches,
    # the eval loss
    rescale = (lambda l: l * float(eng.shard.world)) if (eng.shard is not None and eng.reduction == "mean") else (lambda l: l)
    if mode == ModeKeys.TRAIN:
        # the whole step as ONE hipGraph launch — bit for bit the eager step (tests/test_hip_model.py) — where a step is
        # launch-bound: "auto" (the default) takes it for batches of <= GRAPH_AUTO_MAX_BATCH examples on a single GPU
        # (trainers.deep_fm at the reference's defaults, B = 32: 2-2.5x the eager rate), "on" / True always, "off" never
        # small models: the whole step as ONE kernel launch (engine.fused_train_step) — "off" (the default) never, "on"
        # whenever the model and batch are inside the kernel's scope (outside it: an error, not a fallback), "auto" where
        # it was measured to win.  A step whose layer summaries are recorded runs the layered path (the fused kernel
        # keeps no activations in memory); the next fused step carries on from it.
        fs = params.get("fused_step", "off")
        if fs not in ("off", "on", "auto"):
            raise ValueError("fused_step must be 'off', 'on' or 'auto'")
        if fs != "off":
            B = ids.shape[0]
            ok = eng.fused_step_ok(B)
            if fs == "on" and not ok:
                raise ValueError("fused_step=on: the model has %s" % eng._fused_step_limit(B))
            if ok and (fs == "on" or eng.fused_step_auto(B)) and not getattr(eng, "summaries_next", False):
                # (the batch's numeric features, where the model has numeric columns, go with it)
                loss, logits = eng.fused_train_step(ids, y, x) if x is not None else eng.fused_train_step(ids, y)
                return EstimatorSpec(mode, predictions=None, loss=rescale(loss), train_op=eng.step)
        hg = params.get("hip_graph", "auto")
        graph = hg in (True, "on") or (hg == "auto" and ids.shape[0] <= GRAPH_AUTO_MAX_BATCH)
        if getattr(eng, "summaries_next", False) and ids.shape[0] >= getattr(eng, "TOP_FUSED_MIN_BATCH", 1 << 62):
            graph = False         # (a captured large-batch step keeps the last hidden layer on the chip: this one is looked at)
        if graph and eng.device.type == "cuda" and hasattr(eng, "graph_ok") and eng.graph_ok():
            loss, logits = eng.graph_train_step(ids, y, x)
        else:
            # the next batch, if the train loop holds it (Estimator._with_lookahead: large batches, one GPU): transformed and
            # copied now — the GPU still runs the previous step — and announced to the engine
            la, nxt_ids = params.get("_lookahead"), None
            if la is not None and ahead is None and eng.shard is None:
                nxt = stage(la["features"], la["labels"])
                store["staged"] = (la["features"], nxt)
                if nxt[0][0].shape == ids.shape:
                    nxt_ids = nxt[0][0]
            loss, logits = eng.train_step(ids, y, x, next_ids=nxt_ids) if nxt_ids is not None else eng.train_step(ids, y, x)
        return EstimatorSpec(mode, predictions=None, loss=rescale(loss), train_op=eng.step)
    if mode == ModeKeys.EVAL:
        loss, logits = eng.loss(ids, y, x)
        loss = rescale(loss)
        if store["counters"] is None:
            store["counters"] = _EvalCounters(dev)
        ctr = store["counters"]
        fresh = store.pop("metrics_reset", False)
        if fresh:
            ctr.reset()
        eng.k.mi_eval_accumulate(logits, y, ids.shape[0], ctr.hist, ctr.counts, ctr.sums)
        ctr.batch_losses.append(loss.clone())
        # params["exact_auc"] / params["gauc_by"] (a raw feature key, the per-group AUC's groups; implies exact_auc): the
        # evaluation's logits are also kept and, in result(), sorted and counted — auc_exact, auc_exact_pairs, gauc,
        # gauc_groups beside the bucketed "auc".  On N ranks every rank evaluates the same batches: no collective.
        gauc_by = params.get("gauc_by")
        exact = None
        if params.get("exact_auc") or gauc_by:
            exact = store.get("exact_auc")
            if exact is None:
                from .exact_auc import StreamingExactAuc
                exact = store["exact_auc"] = StreamingExactAuc(dev, eng.k)
            if fresh:
                exact.reset()
            if gauc_by and gauc_by not in features:
                raise ValueError("gauc_by=%r: the batch has no such feature (it has %s)" % (gauc_by, ", ".join(sorted(features))))
            exact.add(logits, y, np.asarray(features[gauc_by]).reshape(-1) if gauc_by else None)

        def result():
            out = metrics_from_counters(ctr.hist.cpu().numpy(), ctr.counts.cpu().numpy(), ctr.sums.cpu().numpy())
            out["loss"] = float(torch.stack(ctr.batch_losses).mean())     # tf.metrics.mean over batch losses
            if exact is not None:
                out.update(exact.metrics())
            return out
        store["metrics_result"] = result
        return EstimatorSpec(mode, predictions=binary_predictions(logits, eng.k), loss=loss, eval_metric_ops=result)
    if mode == ModeKeys.PREDICT:
        logits = eng.predict_logits(ids, x)
        pr = binary_predictions(logits.clone(), eng.k)
        return EstimatorSpec(mode, predictions=pr, export_outputs={"predict": pr})
    raise ValueError("unknown mode %r" % (mode,))
