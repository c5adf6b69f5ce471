#!/usr/bin/env python
"""Serving latency: the fused launch (DeepFM.predict_fused, csrc/serve.hip) against the layered path (predict_logits +
binary_predictions, the training engine's forward) -> the table of profiles/serve_latency.md.

Two models on weights-only engines with random variables and random ids: the CLI default (the 26 MovieLens fields, E = 4,
hidden [16, 16]) and config 3 of BASELINE.json (26 fields x 1 M ids, E = 64, hidden [512, 256, 128]).  Per batch size:
  gpu   HIP-event time of one call on the stream (warm-up first; median and 10th / 90th percentile of --calls calls,
        the two paths alternating call by call in this process, fresh ids every call);
  wall  host time of Predictor.predict_ids from transformed ids, copies in and out included, ending in a synchronise.
`--trace-calls N` runs N calls of each path at one point and nothing else: the body of a
`rocprofv3 --kernel-trace --stats -- python tools/serve_bench.py --trace-calls N ...` run that lists the launches per call.

    python tools/serve_bench.py [--models cli config3] [--batches 1 32 ...] [--calls 200] [--out FILE.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "recommender-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mi355x_rec.engine import DeepFM, OptimizerSpec          # noqa: E402
from mi355x_rec.feature_column import FieldPlan               # noqa: E402
from mi355x_rec.model import binary_predictions               # noqa: E402
from mi355x_rec.predictor import Predictor                    # noqa: E402
from trainers.ml_100k import get_feature_columns              # noqa: E402

BATCHES = (1, 32, 256, 1024, 4096, 65536)


def make_engine(name):
    if name == "cli":
        vocab, E, hidden = FieldPlan(get_feature_columns(4)["linear"]).vocab_sizes, 4, [16, 16]
    elif name == "config3":
        vocab, E, hidden = [1_000_000] * 26, 64, [512, 256, 128]
    else:
        raise SystemExit("unknown model %r" % name)
    eng = DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=OptimizerSpec("SGD"), device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    eng.init_variables(gen, lin_scale=0.01)
    return eng


def id_pool(eng, B, n, seed):
    rng = np.random.default_rng(seed)
    return [np.stack([rng.integers(0, v, B) for v in eng.vocab_sizes], 1).astype(np.int32) for _ in range(n)]


def pct(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def measure(eng, B, calls, warmup):
    pool_h = id_pool(eng, B, 8 if B <= 4096 else 3, B)
    pool = [torch.from_numpy(a).cuda() for a in pool_h]
    pred = {m: Predictor({"receiver_tensors": {}}, None, eng, mode=m) for m in ("fused", "layered")}
    bufs = pred["fused"]._buffers(B)["out"]

    def fused(ids):
        eng.predict_fused(ids, out=bufs)

    def layered(ids):
        binary_predictions(eng.predict_logits(ids).clone(), eng.k)

    paths = (("fused", fused), ("layered", layered))
    for i in range(warmup):
        for _, fn in paths:
            fn(pool[i % len(pool)])
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in paths}
    for i in range(calls):
        for name, fn in paths:                                   # alternating: both see the same clocks and cache state
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(pool[i % len(pool)])
            e.record()
            ev[name].append((s, e))
    torch.cuda.synchronize()
    gpu = {name: pct([s.elapsed_time(e) * 1e3 for s, e in v]) for name, v in ev.items()}          # us
    wall = {}
    n_wall = max(20, calls // 4)
    for name in ("fused", "layered"):
        p = pred[name]
        for i in range(5):
            p.predict_ids(pool_h[i % len(pool_h)])
        ts = []
        for i in range(n_wall):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.predict_ids(pool_h[i % len(pool_h)])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        wall[name] = pct(ts)
    return {"gpu_us": gpu, "wall_us": wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["cli", "config3"])
    ap.add_argument("--batches", nargs="+", type=int, default=list(BATCHES))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="markdown table (and FILE.json beside it)")
    ap.add_argument("--trace-calls", type=int, default=0, help="only run this many calls of each path (for a kernel trace)")
    args = ap.parse_args()
    rows, lines = [], []
    for name in args.models:
        eng = make_engine(name)
        for B in args.batches:
            if args.trace_calls:
                ids = [torch.from_numpy(a).cuda() for a in id_pool(eng, B, 2, 0)]
                for i in range(args.trace_calls):
                    eng.predict_fused(ids[i % 2])
                    binary_predictions(eng.predict_logits(ids[i % 2]).clone(), eng.k)
                torch.cuda.synchronize()
                continue
            calls = args.calls if B < 65536 or name == "cli" else max(200, args.calls // 2)
            r = measure(eng, B, calls, args.warmup)
            r.update(model=name, B=B, calls=calls)
            rows.append(r)
            f, l = r["gpu_us"]["fused"], r["gpu_us"]["layered"]
            spread = l[2] - l[1]
            verdict = "fused" if f[0] < l[0] - spread else "layered"
            line = "| %s | %d | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | %.2f | %s | %.0f | %.0f |" % (
                name, B, f[0], f[1], f[2], l[0], l[1], l[2], l[0] / f[0], verdict, r["wall_us"]["fused"][0], r["wall_us"]["layered"][0])
            lines.append(line)
            print(line, flush=True)
        del eng
        torch.cuda.empty_cache()
    if args.trace_calls:
        return
    head = ["| model | B | fused GPU us: median (p10-p90) | layered GPU us: median (p10-p90) | layered / fused | faster beyond the "
            "layered spread | fused wall us | layered wall us |", "|---|---|---|---|---|---|---|---|"]
    text = "\n".join(head + lines) + "\n"
    print(text)
    print(json.dumps({"serve_bench": rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
