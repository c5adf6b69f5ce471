"""Serving an export: ``Predictor.from_export(dir)`` turns what ``LatestExporter`` wrote — ``signature.json`` and
``variables.pt`` — into a callable that maps raw receiver tensors to the head's PREDICT dict, with nothing else from
the training run in hand.  The last step of the reference's pipeline (``LatestExporter("exporter", serving_input_fn)``,
``scripts/mle_deploy.sh``: a SavedModel behind an online-prediction service).

Two paths score a batch:
  fused    ``DeepFM.predict_fused``: the whole model as one HIP launch (csrc/serve.hip), ids in, predictions out, with
           the id and output buffers kept per batch size (a call allocates nothing on the device);
  layered  ``DeepFM.predict_logits`` + ``model.binary_predictions``: the training engine's forward, one launch per stage.
``mode="auto"`` takes the path that measured faster (profiles/serve_latency.md; the constants below).

An ensemble — the best members of a ``trainers.sweep``, averaged — is served by ``EnsemblePredictor``: M exports over one
set of feature columns, ids transformed once, and in its fused mode ONE launch for all members and their mean
(``FusedGroup``: mi_predict_group, csrc/serve.hip)."""
import glob
import json
import os

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from .feature_column import FieldPlan, column_from_json
from .model import binary_predictions, rank_targets_sides, recommend_sides, side_inputs, split_sides

# mode="auto": the fused launch for batches up to FUSED_MAX_BATCH requests, as long as the MLP's weights — which every
# workgroup of 32 requests streams through one CU — stay below FUSED_MAX_WEIGHT_BYTES.  Both from the table in
# profiles/serve_latency.md (tools/serve_bench.py): at every measured point "auto" is the path that measured faster.
FUSED_MAX_BATCH = 4096
FUSED_MAX_WEIGHT_BYTES = 256 * 1024

OUTPUTS = ("logits", "logistic", "probabilities", "class_ids", "classes")


def _newest(export_dir):
    """export_dir itself when it holds a signature, else its newest <timestamp> sub-directory that does"""
    if os.path.exists(os.path.join(export_dir, "signature.json")):
        return export_dir
    subs = [d for d in glob.glob(os.path.join(export_dir, "*")) if os.path.exists(os.path.join(d, "signature.json"))]
    if not subs:
        raise FileNotFoundError("no export (signature.json) in %s or its sub-directories" % export_dir)
    num = lambda d: int(os.path.basename(d)) if os.path.basename(d).isdigit() else -1
    return max(subs, key=lambda d: (num(d), d))


class Predictor:
    """``predictor(features) -> dict`` of numpy arrays with the signature's outputs (logits, logistic, probabilities,
    class_ids, classes).  ``features`` maps the receiver names of the export's signature to equally long sequences of
    raw values; a receiver whose spec carries a default may be omitted."""

    def __init__(self, signature, plan, eng, mode="auto", device_transform="off"):
        if mode not in ("auto", "fused", "layered"):
            raise ValueError("mode must be 'auto', 'fused' or 'layered'")
        # device_transform="on": a request's raw columns go to the device and become ids there, written straight into the
        # per-B ids buffer (mi_ids_transform); recommend / rank_targets transform both sides there too
        plan.set_device_mode(device_transform)
        self.signature, self.plan, self.engine, self.mode = signature, plan, eng, mode
        self.receivers = {}
        for key, spec in signature["receiver_tensors"].items():
            parts = str(spec).split()
            default = None
            if "default" in parts:
                raw = parts[parts.index("default") + 1]
                default = raw if parts[0] == "string" else int(raw) if parts[0].startswith("int") else float(raw)
            self.receivers[key] = (parts[0], default)
        self._bufs = {}
        if mode == "fused" and not eng.fused_predict_ok():
            raise ValueError("mode='fused': the model has %s" % eng._fused_limit())

    @classmethod
    def from_export(cls, export_dir, device="cuda", mode="auto", device_transform="off"):
        """export_dir: one <timestamp> directory of an export, or the folder that holds them (``<job-dir>/export/exporter``:
        the newest is taken).  The columns and the FieldPlan are rebuilt from the signature's "model" entry, the engine from
        the `layout` table of variables.pt, WEIGHTS ONLY: it is built with the SGD spec, whose table is [R, E] records
        without slot columns and which has no dense slots, and the export's table, lin_w and dense are copied in.  For a
        model trained with Adam that is 8 R E bytes of table slots (two of the three columns of every [w | m | v] record)
        plus 8 P bytes of dense slots that are neither allocated nor read from disk into device memory — at config 3
        (26 M rows, E = 64) 13.3 GB of 20 GB."""
        d = _newest(export_dir)
        with open(os.path.join(d, "signature.json")) as f:
            sig = json.load(f)
        if "sharding" in sig:
            raise ValueError("%s is a row-sharded export (\"sharding\": %d files, %s): serving one needs the shards put "
                             "together again, which the predictor does not do" %
                             (d, sig["sharding"].get("world", 0), sig["sharding"].get("rule", "")))
        if "model" not in sig:
            raise ValueError("%s has no \"model\" entry in its signature: it was written before exports described their "
                             "model (feature columns, model kind, activation); export again from the job's checkpoint" % d)
        model = sig["model"]
        cats = [column_from_json(c) for c in model["categorical_columns"]]
        nums = [column_from_json(c) for c in model["numeric_columns"]]
        plan = FieldPlan(cats, nums)
        if [c.name for c in plan.categorical] != [c["name"] for c in model["categorical_columns"]]:
            raise ValueError("%s: the signature's categorical columns are not in field order" % d)
        sd = torch.load(os.path.join(d, "variables.pt"), weights_only=True, map_location="cpu")
        lay = sd["layout"]
        if lay.get("world", 1) != 1:
            raise ValueError("%s: variables.pt holds shard %d of %d" % (d, lay.get("rank", 0), lay["world"]))
        if list(lay["vocab_sizes"]) != list(plan.vocab_sizes) or lay["n_numeric"] != len(plan.numeric):
            raise ValueError("%s: the signature's columns (%s buckets, %d numeric) do not fit variables.pt (%s, %d)" %
                             (d, plan.vocab_sizes, len(plan.numeric), lay["vocab_sizes"], lay["n_numeric"]))
        use = lay["use"]
        eng = _engine.DeepFM(lay["vocab_sizes"], n_numeric=lay["n_numeric"], embedding_size=lay["embedding_size"],
                             hidden_units=lay["hidden_units"], use_linear=use[0], use_mf=use[1], use_dnn=use[2],
                             optimizer=_engine.OptimizerSpec("SGD"), reduction=model["engine"]["reduction"], device=device,
                             numeric=lay["numeric"], activation=model["engine"]["activation"], field_dims=lay.get("field_dims"),
                             wide_fields=lay.get("wide_fields"), deep_numeric=lay.get("deep_numeric"),
                             wide_numeric=lay.get("wide_numeric"))
        mine = eng._layout()
        canon = lambda v: json.loads(json.dumps(v))
        skip = ("optimizer", "linear_optimizer")
        bad = sorted(k for k in set(mine) | set(lay) if k not in skip and canon(mine.get(k)) != canon(lay.get(k)))
        if bad:
            raise ValueError("%s: variables.pt does not fit the model rebuilt from it: %s" % (d, "; ".join(
                "%s = %r in the export, %r here" % (k, lay.get(k), mine.get(k)) for k in bad)))
        for key in ("table", "lin_w", "dense"):
            dst = getattr(eng, key)
            if (dst is None) != (key not in sd):
                raise ValueError("%s: variables.pt %s %r, the model %s it" % (d, "lacks" if key not in sd else "holds", key,
                                                                             "has" if dst is not None else "does not have"))
            if dst is not None:
                if tuple(sd[key].shape) != tuple(dst.shape) or sd[key].dtype != dst.dtype:
                    raise ValueError("%s: %r is %s in the export, %s in the model" % (d, key, tuple(sd[key].shape), tuple(dst.shape)))
                dst.copy_(sd[key].to(eng.device))
        eng.step = eng._final_step = int(sd.get("step", 0))
        p = cls(sig, plan, eng, mode, device_transform)
        p.export_dir = d
        return p

    # ------------------------------------------------------------------ requests
    def _columns(self, features):
        """The receiver tensors as typed numpy columns of one length; defaults filled in."""
        for key in features:
            if key not in self.receivers:
                raise ValueError("unknown feature %r (the export's receivers: %s)" % (key, ", ".join(sorted(self.receivers))))
        n, first = None, None
        cols = {}
        for key, (dtype, default) in self.receivers.items():
            if key not in features:
                if default is None:
                    raise ValueError("feature %r is missing and its receiver has no default" % key)
                continue
            v = features[key]
            a = np.asarray(v, dtype=object) if dtype == "string" else np.asarray(v, dtype=np.dtype(dtype))
            a = a.reshape(-1)
            if n is None:
                n, first = len(a), key
            elif len(a) != n:
                raise ValueError("feature %r has %d values, %r has %d" % (key, len(a), first, n))
            cols[key] = a
        if n is None:
            raise ValueError("no features given")
        for key, (dtype, default) in self.receivers.items():
            if key not in cols:
                cols[key] = np.full(n, default, dtype=object if dtype == "string" else np.dtype(dtype))
        return cols, n

    def transform(self, features):
        """(ids int32 [B, F], x float32 [B, n_numeric] or None) of a request: the columns' own id transforms"""
        cols, _ = self._columns(features)
        return self.plan.transform(cols)

    def use_fused(self, B):
        if self.mode != "auto":
            return self.mode == "fused"
        eng = self.engine
        weights = 4 * sum(fan * h for (_, _, fan, h) in eng.layers)
        return eng.fused_predict_ok() and B <= FUSED_MAX_BATCH and weights <= FUSED_MAX_WEIGHT_BYTES

    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            if len(self._bufs) >= 64:                 # (a server sees a handful of batch sizes; a sweep does not pile them up)
                self._bufs.clear()
            eng, dev = self.engine, self.engine.device
            b = self._bufs[B] = {
                "ids": torch.empty(B, eng.F, dtype=torch.int32, device=dev),
                "x": torch.empty(B, eng.n_numeric, dtype=torch.float32, device=dev) if eng.n_numeric else None,
                "out": _engine.predict_buffers(B, dev)}
        return b

    def predict_ids(self, ids, x=None):
        """The PREDICT dict (numpy) of already transformed ids [B, F] int32 / x [B, n_numeric] float32 (numpy)."""
        eng = self.engine
        B = ids.shape[0]
        if B == 0:
            return {"logits": np.zeros((0, 1), np.float32), "logistic": np.zeros((0, 1), np.float32),
                    "probabilities": np.zeros((0, 2), np.float32), "class_ids": np.zeros((0, 1), np.int64),
                    "classes": np.zeros((0, 1), np.int64)}
        if self.use_fused(B):
            b = self._buffers(B)
            b["ids"].copy_(torch.from_numpy(ids))
            if b["x"] is not None:
                b["x"].copy_(torch.from_numpy(x))
            return self._predict_device(b["ids"], b["x"])
        dev = eng.device
        return self._predict_device(torch.from_numpy(ids).to(dev), torch.from_numpy(x).to(dev) if x is not None else None)

    def _predict_device(self, ids, x):
        """The PREDICT dict (numpy) of ids / x on the device (the fused path: the per-B buffers themselves)"""
        eng = self.engine
        if self.use_fused(ids.shape[0]):
            pr = eng.predict_fused(ids, x, out=self._buffers(ids.shape[0])["out"])
        else:
            pr = binary_predictions(eng.predict_logits(ids, x).clone(), eng.k)
        host = {k: pr[k].to("cpu", copy=True).numpy() for k in OUTPUTS[:4]}     # (copies: the device buffers are reused)
        host["classes"] = host["class_ids"]
        return host

    def _transform_on_device(self, features):
        """(ids, x) of a request on the device, or None for an empty one: the raw columns copied, the ids made there — into
        the per-B ids buffer where the fused path will read them"""
        cols, n = self._columns(features)
        if n == 0:
            return None
        dt = self.plan.on_device(self.engine.device, self.engine.k)
        if not self.use_fused(n):
            return dt.transform(cols)
        b = self._buffers(n)
        ids, x = dt.transform(cols, out=b["ids"])
        if b["x"] is not None:
            b["x"].copy_(x)
        return b["ids"], b["x"]

    def __call__(self, features):
        if self.plan.device_mode == "on":
            on_dev = self._transform_on_device(features)
            if on_dev is not None:
                return self._predict_device(*on_dev)
        ids, x = self.transform(features)
        return self.predict_ids(ids, x)

    # ------------------------------------------------------------------ top-K recommendation
    def recommend(self, query_features, candidate_features, k, exclude=None):
        """What Estimator.recommend does for a checkpoint, for this export: the k best candidates of every query by logit
        (DeepFM.top_k).  The two dicts map the columns' source keys to each side's raw values (a column belongs to the side
        whose dict holds its key; keys no column reads are ignored); exclude as DeepFM.top_k takes it.  Returns numpy
        arrays: logits [U, k], probabilities [U, k] (the head's logistic) and indices [U, k] (-1 / -inf / 0 past the
        eligible candidates)."""
        return recommend_sides(self.plan, self.engine, query_features, candidate_features, k, exclude)

    def rank_targets(self, query_features, candidate_features, targets, exclude=None):
        """What Estimator.rank_targets does for a checkpoint, for this export: the exact 0-based rank of named target
        candidates among all eligible candidates of their query (DeepFM.target_ranks), numpy int32 [U, Tmax], -1 where a
        target has no rank."""
        return rank_targets_sides(self.plan, [self.engine], query_features, candidate_features, targets, exclude)[0]


def host_top_k(scores, k, excl_off=None, excl_idx=None):
    """The selection rule of mi_pair_topk (include/mi355x_rec.h) on the host: per row of scores [U, I] the k best eligible
    candidates — score descending, equal scores by ascending index, NaN below every number, a -0 returned as +0 — padded
    with index -1 / score -inf.  excl_off / excl_idx: the excluded candidates per row as a CSR pair (numpy), or None."""
    U, I = scores.shape
    top_s = np.full((U, k), -np.inf, np.float32)
    top_i = np.full((U, k), -1, np.int32)
    for u in range(U):
        ok = np.arange(I)
        if excl_off is not None:
            ok = np.setdiff1d(ok, np.asarray(excl_idx[excl_off[u]:excl_off[u + 1]], np.int64))
        s = scores[u, ok]
        order = np.lexsort((ok, np.where(np.isnan(s), np.inf, -s)))[:k]
        top_s[u, :len(order)] = s[order] + np.float32(0.0)
        top_i[u, :len(order)] = ok[order]
    return top_s, top_i


# ---------------------------------------------------------------------- an ensemble of exports
def _serve_member(eng, keep_alive):
    """engine eng as a mi_serve_member_t (keep_alive: the host tables the struct points to)"""
    layer_off, widths, wide = eng._fused_tables()
    keep_alive += [layer_off, widths]
    m = _lib.ServeMember()
    _lib.set_ptrs(m, table=eng.table, lin_w=eng.lin_w, dense=eng.dense, layer_off=layer_off, widths=widths)
    m.table_stride, m.lin_stride, m.E, m.n_layers, m.activation = eng.ts, eng.ls, eng.E, len(eng.layers), eng.act
    m.use_linear, m.use_fm, m.use_dnn, m.numeric_raw = int(eng.use_linear), int(eng.use_mf), int(eng.use_dnn), int(eng.raw_numeric)
    m.lin_bias_off = eng.lin_bias_off
    m.num_emb_off = -1 if eng.num_emb_off is None else eng.num_emb_off
    m.lin_num_off = -1 if eng.lin_num_off is None else eng.lin_num_off
    m.wide_fields = wide
    return m


class FusedGroup:
    """M engines over one set of feature columns, scored and averaged in ONE launch (mi_predict_group): member i's logit is
    bit for bit its own predict_fused's, the ensemble's is (((z_0 + z_1) + ...) + z_{M-1}) / M in fp32.  The plan is made
    once, here; it holds the engines' pointers (a caller who REPLACES a member's tensors makes a new group)."""

    MAX_MEMBERS = _lib.PREDICT_GROUP_MAX_MEMBERS

    def __init__(self, engines):
        self.engines = _engine.check_members("FusedGroup", engines, self.MAX_MEMBERS,
                                             lambda e: "row-sharded tables" if e.shard is not None else e._fused_limit())
        self.M, lead = len(self.engines), self.engines[0]
        self.k, self.device, self.F, self.n_numeric = lead.k, lead.device, lead.F, lead.n_numeric
        self._keep = []
        members = (_lib.ServeMember * self.M)(*[_serve_member(e, self._keep) for e in self.engines])
        nbytes = int(self.k.query("mi_predict_group_plan_bytes", self.M))
        self.table = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        self.plan = _lib.ServeGroupPlan()
        self.k.mi_predict_group_plan(members, self.M, self.F, self.n_numeric, lead.field_off, self.table, self.plan)

    def buffers(self, B):
        """member_logits [M, B], the tickets (zero: every call leaves them zero) and the PREDICT dict for batches of B"""
        dev = self.device
        return {"member_logits": torch.empty(self.M, B, dtype=torch.float32, device=dev),
                "tickets": torch.zeros((B + 31) // 32, dtype=torch.int32, device=dev),
                "out": _engine.predict_buffers(B, dev)}

    def run(self, ids, x_num=None, bufs=None):
        """ids int32 [B, F] / x_num float32 [B, n_numeric] on the device -> bufs["out"] (device tensors, as
        DeepFM.predict_fused returns them); bufs["member_logits"] holds the members' own logits.  bufs: buffers(B), kept by
        the caller (None: made here)."""
        lead = self.engines[0]
        lead._prep(ids, None, x_num)
        B = ids.shape[0]
        if B < 1:
            raise ValueError("FusedGroup: no rows")
        for e in self.engines:
            e.finalize_rows()
        if bufs is None:
            bufs = self.buffers(B)
        out = bufs["out"]
        self.k.mi_predict_group(self.plan, self.M, ids, x_num, B, bufs["member_logits"], bufs["tickets"], out["logits"],
                                out["logistic"], out["probabilities"], out["class_ids"])
        return out


def _model_columns(sig):
    """the columns of a signature's "model" entry as the ids see them: everything but the embedding dimension"""
    strip = lambda c: {k: v for k, v in c.items() if k != "embedding_dimension"}
    m = sig["model"]
    return [strip(c) for c in m["categorical_columns"]], [strip(c) for c in m["numeric_columns"]]


def _layered_mean(engines, q_ids, c_ids, qf, k, q_x, c_x):
    """the members' mean pair score [U, I] on the device, member by member: every member's top_k(return_scores=True), a
    torch fp32 sum in member order and a division"""
    acc = None
    for e in engines:
        z = e.top_k(q_ids, c_ids, qf, k, q_x, c_x, return_scores=True)[2]
        acc = z.clone() if acc is None else acc + z
    return acc / torch.full_like(acc, float(len(engines)))


class EnsemblePredictor:
    """``ensemble(features) -> dict``: the mean logit of M Predictors over the same feature columns and what the head makes
    of it — the Predictor dict (logits, logistic, probabilities, class_ids, classes); ``return_members=True`` adds
    member_logits [M, B].  The request's ids are transformed ONCE (member 0's plan: the members' columns are equal), copied
    to the device once, and the outputs come back in one copy.

    mode: "fused"   all members and their mean in one launch (FusedGroup; every member within mi_predict_fused's limits);
          "layered" every member by its own Predictor's path, then a torch fp32 sum in member order, a division and
                    binary_predictions;
          "auto"    fused iff every member's own use_fused(B) says fused (the measured thresholds of profiles/
                    serve_latency.md; profiles/ensemble_latency.md has the ensemble's own table).
    device_transform: None leaves the switch as member 0 was made; "on" / "off" sets it ON MEMBER 0's PLAN, which the
    ensemble shares — a caller who still holds that Predictor sees it change too."""

    def __init__(self, predictors, mode="auto", device_transform=None):
        if mode not in ("auto", "fused", "layered"):
            raise ValueError("mode must be 'auto', 'fused' or 'layered'")
        self.members = list(predictors)
        if not self.members:
            raise ValueError("EnsemblePredictor: no members (an empty list of predictors)")
        if len(self.members) > FusedGroup.MAX_MEMBERS:
            raise ValueError("EnsemblePredictor: %d members (at most %d)" % (len(self.members), FusedGroup.MAX_MEMBERS))
        lead = self.members[0]
        cats0, nums0 = _model_columns(lead.signature)
        for i, p in enumerate(self.members[1:], 1):
            cats, nums = _model_columns(p.signature)
            for what, a, b in (("categorical", cats0, cats), ("numeric", nums0, nums)):
                if len(a) != len(b):
                    raise ValueError("EnsemblePredictor: member %d has %d %s columns, member 0 has %d" % (i, len(b), what, len(a)))
                for f, (ca, cb) in enumerate(zip(a, b)):
                    if ca != cb:
                        key = next(k for k in sorted(set(ca) | set(cb)) if ca.get(k) != cb.get(k))
                        raise ValueError("EnsemblePredictor: member %d differs from member 0 in %s column %d (%r): %s = %r "
                                         "against %r" % (i, what, f, ca.get("name"), key, cb.get(key), ca.get(key)))
            ra, rb = lead.signature["receiver_tensors"], p.signature["receiver_tensors"]
            if ra != rb:
                key = next(k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k))
                raise ValueError("EnsemblePredictor: member %d differs from member 0 in receiver %r: %r against %r" % (
                    i, key, rb.get(key), ra.get(key)))
            if p.engine.device != lead.engine.device:
                raise ValueError("EnsemblePredictor: member %d is on device %s, member 0 on %s" % (
                    i, p.engine.device, lead.engine.device))
        if mode == "fused":
            for i, p in enumerate(self.members):
                if not p.engine.fused_predict_ok():
                    raise ValueError("mode='fused': member %d: the model has %s" % (
                        i, p.engine._fused_limit() or "row-sharded tables"))
        self.mode, self.signature, self.plan, self.receivers = mode, lead.signature, lead.plan, lead.receivers
        if device_transform is not None:      # (None: as member 0 was made; "on" / "off": as Predictor takes it)
            self.plan.set_device_mode(device_transform)
        self.device, self.k = lead.engine.device, lead.engine.k
        self.export_dirs = [getattr(p, "export_dir", None) for p in self.members]
        self._group = None
        self._bufs = {}

    @classmethod
    def from_exports(cls, export_dirs, device="cuda", mode="auto", member_mode="auto", device_transform="off"):
        """One Predictor.from_export per directory (member_mode: the members' own mode, which "layered" and "auto" consult)"""
        return cls([Predictor.from_export(d, device=device, mode=member_mode) for d in export_dirs], mode=mode,
                   device_transform=device_transform)

    @classmethod
    def from_sweep(cls, job_dir, top, device="cuda", mode="auto", member_mode="auto", device_transform="off"):
        """The first `top` rows of <job_dir>/sweep.json — trainers.sweep ranked them best first — each from its export"""
        path = os.path.join(job_dir, "sweep.json")
        if not os.path.exists(path):
            raise FileNotFoundError("%s has no sweep.json: an ensemble is taken from the job directory of a trainers.sweep run" % job_dir)
        with open(path) as f:
            rows = json.load(f)["members"]
        if top < 1 or top > len(rows):
            raise ValueError("top=%d: the sweep in %s has %d members (1 <= top <= %d)" % (top, job_dir, len(rows), len(rows)))
        dirs = []
        for row in rows[:top]:
            d = row["export"]
            if not os.path.isdir(d):                    # (a sweep directory that was moved: the members lie inside it)
                d = os.path.join(job_dir, "member_%d" % row["member"], "export", "exporter")
            dirs.append(d)
        ens = cls.from_exports(dirs, device=device, mode=mode, member_mode=member_mode, device_transform=device_transform)
        ens.sweep_members = [row["member"] for row in rows[:top]]
        return ens

    # ------------------------------------------------------------------ requests
    def transform(self, features):
        return self.members[0].transform(features)

    def use_fused(self, B):
        if self.mode != "auto":
            return self.mode == "fused"
        return all(p.use_fused(B) for p in self.members)

    def _buffers(self, B):
        """Per batch size: ids / x on the device, the group's scratch (member logits, tickets) and ONE packed output buffer
        [logits B | logistic B | probabilities 2 B | class_ids B int64 | member_logits M B] whose views the launch writes
        and one copy brings to the host."""
        b = self._bufs.get(B)
        if b is None:
            if len(self._bufs) >= 64:
                self._bufs.clear()
            dev, M = self.device, len(self.members)
            eng = self.members[0].engine
            pack = torch.empty(24 * B + 4 * M * B, dtype=torch.uint8, device=dev)
            f32 = lambda lo, n, *shape: pack[lo:lo + 4 * n].view(torch.float32).view(*shape)
            cls = pack[16 * B:24 * B].view(torch.int64).view(B, 1)
            b = self._bufs[B] = {
                "ids": torch.empty(B, eng.F, dtype=torch.int32, device=dev),
                "x": torch.empty(B, eng.n_numeric, dtype=torch.float32, device=dev) if eng.n_numeric else None,
                "pack": pack, "member_logits": f32(24 * B, M * B, M, B),
                "tickets": torch.zeros((B + 31) // 32, dtype=torch.int32, device=dev),
                "out": {"logits": f32(0, B, B, 1), "logistic": f32(4 * B, B, B, 1), "probabilities": f32(8 * B, 2 * B, B, 2),
                        "class_ids": cls, "classes": cls}}
        return b

    def predict_ids(self, ids, x=None, return_members=False):
        """The PREDICT dict (numpy) of already transformed ids [B, F] int32 / x [B, n_numeric] float32 (numpy)."""
        B, M = ids.shape[0], len(self.members)
        if B == 0:
            host = {"logits": np.zeros((0, 1), np.float32), "logistic": np.zeros((0, 1), np.float32),
                    "probabilities": np.zeros((0, 2), np.float32), "class_ids": np.zeros((0, 1), np.int64),
                    "classes": np.zeros((0, 1), np.int64)}
            if return_members:
                host["member_logits"] = np.zeros((M, 0), np.float32)
            return host
        b = self._buffers(B)
        b["ids"].copy_(torch.from_numpy(ids))
        if b["x"] is not None:
            b["x"].copy_(torch.from_numpy(x))
        return self._predict_buffers(b, B, return_members)

    def _predict_buffers(self, b, B, return_members):
        """The PREDICT dict (numpy) of the ids / x that lie in the per-B buffers b"""
        M = len(self.members)
        if self.use_fused(B):
            if self._group is None:
                self._group = FusedGroup([p.engine for p in self.members])
            self._group.run(b["ids"], b["x"], b)
        else:
            acc = None
            for i, p in enumerate(self.members):
                eng = p.engine
                if p.use_fused(B):
                    z = eng.predict_fused(b["ids"], b["x"])["logits"].reshape(-1)
                else:
                    z = eng.predict_logits(b["ids"], b["x"]).reshape(-1)
                b["member_logits"][i].copy_(z)
                acc = z.clone() if acc is None else acc + z
            pr = binary_predictions(acc / torch.full_like(acc, float(M)), self.k)
            for key in OUTPUTS[:4]:
                b["out"][key].copy_(pr[key])
        n = 24 * B + (4 * M * B if return_members else 0)
        flat = b["pack"][:n].to("cpu", copy=True).numpy()                  # (a copy: the device buffer is reused)
        host = {"logits": flat[:4 * B].view(np.float32).reshape(B, 1), "logistic": flat[4 * B:8 * B].view(np.float32).reshape(B, 1),
                "probabilities": flat[8 * B:16 * B].view(np.float32).reshape(B, 2),
                "class_ids": flat[16 * B:24 * B].view(np.int64).reshape(B, 1)}
        host["classes"] = host["class_ids"]
        if return_members:
            host["member_logits"] = flat[24 * B:].view(np.float32).reshape(M, B)
        return host

    def __call__(self, features, return_members=False):
        if self.plan.device_mode == "on":
            lead = self.members[0]
            cols, n = lead._columns(features)
            if n:
                b = self._buffers(n)
                _, x = self.plan.on_device(self.device, self.k).transform(cols, out=b["ids"])
                if b["x"] is not None:
                    b["x"].copy_(x)
                return self._predict_buffers(b, n, return_members)
        ids, x = self.transform(features)
        return self.predict_ids(ids, x, return_members=return_members)

    # ------------------------------------------------------------------ top-K recommendation
    def rank_fused_limit(self):
        """(member, text) of the first member outside mi_pair_topk_group's scope, or None when the group launch can rank"""
        for i, p in enumerate(self.members):
            why = p.engine._top_k_group_limit()
            if why is not None:
                return i, why
        return None

    def recommend(self, query_features, candidate_features, k, exclude=None, mode=None, return_scores=False):
        """Predictor.recommend for the ensemble: the k best candidates of every query by the MEAN logit of the members.
        Both sides' ids are transformed once (member 0's plan) and the exclusions built once; the per-side precompute runs
        once per member with the member's own kernels.

        mode (None: the ensemble's own):
          "fused"   one pair scoring and selection launch for all members (engine.top_k_group: mi_pair_topk_group);
                    ValueError naming the member and the limit when a member is outside that kernel's scope;
          "layered" every member's top_k(return_scores=True), a torch fp32 sum in member order, a division, and the
                    header's selection rule on the host (host_top_k) — the fallback, not the hot path;
          "auto"    fused iff every member is inside the kernel's scope.
        Returns numpy arrays: logits [U, k] (the mean logit), probabilities [U, k], indices [U, k]; return_scores adds
        scores [U, I], every pair's mean logit."""
        mode = self.mode if mode is None else mode
        if mode not in ("auto", "fused", "layered"):
            raise ValueError("mode must be 'auto', 'fused' or 'layered'")
        limit = self.rank_fused_limit()
        if mode == "fused" and limit is not None:
            raise ValueError("mode='fused': member %d: the model has %s" % limit)
        fused = mode == "fused" or (mode == "auto" and limit is None)
        plan, lead = self.plan, self.members[0].engine
        qf = split_sides(plan, query_features, candidate_features)
        cf = [f for f in range(len(plan.categorical) + len(plan.numeric)) if f not in qf]
        q_ids, q_x = side_inputs(plan, qf, query_features, self.device)
        c_ids, c_x = side_inputs(plan, cf, candidate_features, self.device)
        engines = [p.engine for p in self.members]
        if fused:
            out = _engine.top_k_group(engines, q_ids, c_ids, qf, k, q_x, c_x, exclude=exclude, return_scores=return_scores)
            score, idx = out[0], out[1]
            scores = out[2].cpu().numpy() if return_scores else None
        else:
            _, U, I, k = lead._top_k_check(q_ids, c_ids, qf, k, q_x, c_x)
            off, ix = lead._top_k_exclusions(exclude, U, I) if exclude is not None else (None, None)
            scores = _layered_mean(engines, q_ids, c_ids, qf, k, q_x, c_x).cpu().numpy()
            top_s, top_i = host_top_k(scores, k, None if off is None else off.cpu().numpy(),
                                      None if ix is None else ix.cpu().numpy())
            score, idx = torch.from_numpy(top_s).to(self.device), torch.from_numpy(top_i).to(self.device)
        pr = binary_predictions(score.reshape(-1).contiguous(), self.k)
        host = {"logits": score.cpu().numpy(), "probabilities": pr["logistic"].reshape(score.shape).cpu().numpy(),
                "indices": idx.cpu().numpy()}
        if return_scores:
            host["scores"] = scores
        return host

    def rank_targets(self, query_features, candidate_features, targets, exclude=None, mode=None, return_scores=False):
        """Predictor.rank_targets for the ensemble: the exact 0-based rank of named target candidates among all eligible
        candidates of their query by the MEAN logit of the members — the position a target would take in recommend's list
        were k unbounded.  targets and exclude as DeepFM.target_ranks takes them; the two feature dicts and mode as
        recommend takes them:
          "fused"   one scoring and counting launch for all members per 64 target columns (engine.target_ranks_mean:
                    mi_pair_target_ranks_mean); ValueError naming the member and the limit when a member is outside that
                    kernel's scope;
          "layered" the mean matrix as recommend's layered branch makes it, and the keys counted by torch comparisons on
                    the device (engine.ranks_from_scores) — the fallback, not the hot path;
          "auto"    fused iff every member is inside the kernel's scope.
        Returns numpy int32 [U, Tmax], -1 where a target has no rank; return_scores adds the targets' mean logits float32
        [U, Tmax] (NaN there)."""
        mode = self.mode if mode is None else mode
        if mode not in ("auto", "fused", "layered"):
            raise ValueError("mode must be 'auto', 'fused' or 'layered'")
        limit = self.rank_fused_limit()
        if mode == "fused" and limit is not None:
            raise ValueError("mode='fused': member %d: the model has %s" % limit)
        plan, lead = self.plan, self.members[0].engine
        qf = split_sides(plan, query_features, candidate_features)
        cf = [f for f in range(len(plan.categorical) + len(plan.numeric)) if f not in qf]
        q_ids, q_x = side_inputs(plan, qf, query_features, self.device)
        c_ids, c_x = side_inputs(plan, cf, candidate_features, self.device)
        engines = [p.engine for p in self.members]
        if mode == "fused" or (mode == "auto" and limit is None):
            out = _engine.target_ranks_mean(engines, q_ids, c_ids, qf, targets, q_x, c_x, exclude=exclude,
                                            return_scores=return_scores)
            ranks, scores = out if return_scores else (out, None)
        else:
            _, U, I, _ = lead._top_k_check(q_ids, c_ids, qf, 1, q_x, c_x)
            tg = torch.from_numpy(_engine.dense_targets(targets, U, I)).to(self.device).long()
            excl = lead._top_k_exclusions(exclude, U, I) if exclude is not None else None
            ranks, scores = _engine.ranks_from_scores(_layered_mean(engines, q_ids, c_ids, qf, 1, q_x, c_x), tg, excl)
        ranks = ranks.cpu().numpy()
        return (ranks, scores.cpu().numpy()) if return_scores else ranks
