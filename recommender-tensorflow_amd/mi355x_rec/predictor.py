"""Serving an export: ``Predictor.from_export(dir)`` turns what ``LatestExporter`` wrote — ``signature.json`` and
``variables.pt`` — into a callable that maps raw receiver tensors to the head's PREDICT dict, with nothing else from
the training run in hand.  The last step of the reference's pipeline (``LatestExporter("exporter", serving_input_fn)``,
``scripts/mle_deploy.sh``: a SavedModel behind an online-prediction service).

Two paths score a batch:
  fused    ``DeepFM.predict_fused``: the whole model as one HIP launch (csrc/serve.hip), ids in, predictions out, with
           the id and output buffers kept per batch size (a call allocates nothing on the device);
  layered  ``DeepFM.predict_logits`` + ``model.binary_predictions``: the training engine's forward, one launch per stage.
``mode="auto"`` takes the path that measured faster (profiles/serve_latency.md; the constants below)."""
import glob
import json
import os

import numpy as np
import torch

from . import engine as _engine
from .feature_column import FieldPlan, column_from_json
from .model import binary_predictions

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

    def __init__(self, signature, plan, eng, mode="auto"):
        if mode not in ("auto", "fused", "layered"):
            raise ValueError("mode must be 'auto', 'fused' or 'layered'")
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
    def from_export(cls, export_dir, device="cuda", mode="auto"):
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
        p = cls(sig, plan, eng, mode)
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
            cls = torch.empty(B, 1, dtype=torch.int64, device=dev)
            b = self._bufs[B] = {
                "ids": torch.empty(B, eng.F, dtype=torch.int32, device=dev),
                "x": torch.empty(B, eng.n_numeric, dtype=torch.float32, device=dev) if eng.n_numeric else None,
                "out": {"logits": torch.empty(B, 1, dtype=torch.float32, device=dev),
                        "logistic": torch.empty(B, 1, dtype=torch.float32, device=dev),
                        "probabilities": torch.empty(B, 2, dtype=torch.float32, device=dev), "class_ids": cls, "classes": cls}}
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
            pr = eng.predict_fused(b["ids"], b["x"], out=b["out"])
        else:
            dev = eng.device
            logits = eng.predict_logits(torch.from_numpy(ids).to(dev), torch.from_numpy(x).to(dev) if x is not None else None)
            pr = binary_predictions(logits.clone(), eng.k)
        host = {k: pr[k].to("cpu", copy=True).numpy() for k in OUTPUTS[:4]}     # (copies: the device buffers are reused)
        host["classes"] = host["class_ids"]
        return host

    def __call__(self, features):
        ids, x = self.transform(features)
        return self.predict_ids(ids, x)
