#!/usr/bin/env python
"""Ensemble serving latency: M members and their mean in ONE launch (FusedGroup: mi_predict_group, csrc/serve.hip) against
doing the same work member by member -> the table of profiles/ensemble_latency.md.

M weights-only engines of the CLI default model (the 26 MovieLens fields, E = 4, hidden [16, 16]) with random variables
and random ids.  Per (M, B):
  group      one mi_predict_group call into buffers kept per batch size;
  per-member M DeepFM.predict_fused calls (outputs kept per member), a torch fp32 sum in member order, a division and
             mi_binary_predictions: what serving the same ensemble took before the group launch existed;
  single     one predict_fused call of member 0: the price of serving the best member alone.
HIP-event time of one call on the stream (warm-up first; median and 10th / 90th percentile of --calls calls, the three
paths alternating call by call in this process, fresh ids every call).  `--trace-calls N` runs N calls of the group and
the per-member path at one point and nothing else: the body of a
`rocprofv3 --kernel-trace --stats -- python tools/ensemble_bench.py --trace-calls N --members 8 --batches 32` run.

    python tools/ensemble_bench.py [--members 1 4 8 16 64] [--batches 1 32 256 4096] [--calls 200] [--out FILE.md]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "recommender-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mi355x_rec.engine import DeepFM, OptimizerSpec          # noqa: E402
from mi355x_rec.feature_column import FieldPlan               # noqa: E402
from mi355x_rec.model import binary_predictions               # noqa: E402
from mi355x_rec.predictor import FusedGroup                   # noqa: E402
from trainers.ml_100k import get_feature_columns              # noqa: E402

MEMBERS = (1, 4, 8, 16, 64)
BATCHES = (1, 32, 256, 4096)


def make_engines(M):
    vocab = FieldPlan(get_feature_columns(4)["linear"]).vocab_sizes
    out = []
    for i in range(M):
        eng = DeepFM(vocab, embedding_size=4, hidden_units=[16, 16], optimizer=OptimizerSpec("SGD"), device="cuda")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(i)
        eng.init_variables(gen, lin_scale=0.01)
        out.append(eng)
    return out


def id_pool(eng, B, n, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(np.stack([rng.integers(0, v, B) for v in eng.vocab_sizes], 1).astype(np.int32)).cuda() for _ in range(n)]


def pct(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def make_paths(engines, group, B):
    M = len(engines)
    bufs = group.buffers(B)
    solo = [group.buffers(B)["out"] for _ in engines]
    div = torch.full((B,), float(M), device="cuda")

    def grouped(ids):
        group.run(ids, None, bufs)

    def per_member(ids):
        acc = None
        for eng, out in zip(engines, solo):
            z = eng.predict_fused(ids, out=out)["logits"].reshape(-1)
            acc = z if acc is None else acc + z
        binary_predictions(acc / div, engines[0].k)

    def single(ids):
        engines[0].predict_fused(ids, out=solo[0])

    return (("group", grouped), ("per_member", per_member), ("single", single))


def measure(engines, group, B, calls, warmup):
    pool = id_pool(engines[0], B, 8, B)
    paths = make_paths(engines, group, B)
    for i in range(warmup):
        for _, fn in paths:
            fn(pool[i % len(pool)])
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in paths}
    for i in range(calls):
        for name, fn in paths:                                   # alternating: all see the same clocks and cache state
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(pool[i % len(pool)])
            e.record()
            ev[name].append((s, e))
    torch.cuda.synchronize()
    return {name: pct([s.elapsed_time(e) * 1e3 for s, e in v]) for name, v in ev.items()}          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", nargs="+", type=int, default=list(MEMBERS))
    ap.add_argument("--batches", nargs="+", type=int, default=list(BATCHES))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="markdown table (and FILE.json beside it)")
    ap.add_argument("--trace-calls", type=int, default=0, help="only run this many calls of the group and the per-member path "
                                                                "(for a kernel trace)")
    args = ap.parse_args()
    engines = make_engines(max(args.members))
    rows, lines = [], []
    for M in args.members:
        group = FusedGroup(engines[:M])
        for B in args.batches:
            if args.trace_calls:
                ids = id_pool(engines[0], B, 2, 0)
                paths = dict(make_paths(engines[:M], group, B))
                for i in range(args.trace_calls):
                    paths["group"](ids[i % 2])
                    paths["per_member"](ids[i % 2])
                torch.cuda.synchronize()
                continue
            r = measure(engines[:M], group, B, args.calls, args.warmup)
            rows.append({"M": M, "B": B, "calls": args.calls, "gpu_us": r})
            g, p, s = r["group"], r["per_member"], r["single"]
            verdict = "group" if g[0] < p[0] - (p[2] - p[1]) else "per-member"
            line = "| %d | %d | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | %.2f | %.2f | %s |" % (
                M, B, g[0], g[1], g[2], p[0], p[1], p[2], s[0], s[1], s[2], p[0] / g[0], g[0] / s[0], verdict)
            lines.append(line)
            print(line, flush=True)
    if args.trace_calls:
        return
    head = ["| M | B | group GPU us: median (p10-p90) | per-member GPU us: median (p10-p90) | single member GPU us: median (p10-p90) | "
            "per-member / group | group / single | faster beyond the per-member spread |", "|---:|---:|---:|---:|---:|---:|---:|---|"]
    text = "\n".join(head + lines) + "\n"
    print(text)
    print(json.dumps({"ensemble_bench": rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
