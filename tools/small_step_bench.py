#!/usr/bin/env python3
"""Step latency of small models — the reference's default configuration (trainers.deep_fm: E=4, hidden [16,16], B=32,
the 26 MovieLens fields) and its neighbours — launch-bound, not roofline-bound: us per train step for the three ways
the engine runs one step on one GPU:

    eager (one launch per kernel)      DeepFM.train_step
    hipGraph replay                    DeepFM.graph_train_step
    fused (one launch)                 DeepFM.fused_train_step   (where the model and batch are inside its scope)

Protocol: the three paths run in ONE process on three engines with identical initial state; every
path walks the same ring of ROTATE different batches (with one repeated batch no row ever sits a step out, and the
catch-up / sweep would have nothing to do); a block is STEPS consecutive steps of one path between two device
synchronisations, timed on the host clock (the host's cost is part of what a user pays); blocks of the three paths
alternate; per path the median and the 10th / 90th percentile over BLOCKS blocks are reported.

    python tools/small_step_bench.py [--json FILE] [--blocks N] [--steps N]
    python tools/small_step_bench.py --rules ...     the legs of profiles/fused_step_rules.md instead: B = 32, the three canned
                                                     CLIs' default models and the default DeepFM under Adagrad, Ftrl, RMSProp, SGD
    python tools/small_step_bench.py --numeric N [N ...]   the legs of profiles/fused_step_numeric.md instead: B = 32, the
                                                     default DeepFM with N numeric embedding columns beside the 26 categorical
                                                     ones (x_num standard normal), one case per N
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
import math

import numpy as np
import torch
from mi355x_rec.engine import DeepFM, OptimizerSpec

ROTATE = 8


def vocab(big=1000):
    """the 26 MovieLens columns; `big` scales the three hash-bucket columns (user, item, zipcode: 1000 / 2000 / 1000)"""
    return [2] * 19 + [big, 2 * big, 50, big, 7, 8, 3]


CASES = [
    # name, vocab, E, hidden, batch sizes
    ("default", vocab(), 4, [16, 16], (1, 32, 128, 1024)),
    ("top of the envelope", vocab(), 16, [64, 64, 32], (32,)),
    ("default, 8x the rows", vocab(8000), 4, [16, 16], (32,)),
    ("default, 32x the rows", vocab(32000), 4, [16, 16], (32,)),
    ("default, 64x the rows", vocab(65000), 4, [16, 16], (32,)),
]


_FTRL = OptimizerSpec("Ftrl", min(0.2, 1.0 / math.sqrt(26)))        # trainers/linear.py:30
# --rules: name, vocab, E, hidden, batch sizes, engine arguments (mi_train_step_model's models: DESIGN section 11)
RULE_CASES = [
    ("trainers.linear (Ftrl)", vocab(), 4, [], (32,), dict(use_mf=False, use_dnn=False, optimizer=_FTRL, reduction="sum", dropout=0.0)),
    ("trainers.deep (Adagrad)", vocab(), 4, [16, 16], (32,),
     dict(use_linear=False, use_mf=False, optimizer=OptimizerSpec("Adagrad", 0.05), reduction="sum")),
    ("trainers.linear_deep (Ftrl + Adagrad)", vocab(), 4, [16, 16], (32,),
     dict(use_mf=False, optimizer=OptimizerSpec("Adagrad", 0.05), linear_optimizer=_FTRL, reduction="sum")),
] + [("default DeepFM, %s" % name, vocab(), 4, [16, 16], (32,), dict(optimizer=OptimizerSpec(name, lr)))
     for name, lr in (("Adagrad", 0.05), ("Ftrl", 0.05), ("RMSProp", 0.001), ("SGD", 0.05))]


def numeric_cases(counts):
    return [("default + %d numeric" % n, vocab(), 4, [16, 16], (32,), dict(n_numeric=n, fused_numeric=True)) for n in counts]


def engines(voc, E, hidden, n, **kw):
    out = []
    kw = dict(dict(dropout=0.1, optimizer=OptimizerSpec("Adam", 0.001)), **kw)
    for _ in range(n):
        m = DeepFM(voc, embedding_size=E, hidden_units=hidden, **kw)
        g = torch.Generator(device="cuda")
        g.manual_seed(0)
        m.init_variables(g, lin_scale=1e-3)
        out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write every cell to this file")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rules", action="store_true", help="the legs of profiles/fused_step_rules.md instead of the Adam cases")
    ap.add_argument("--numeric", type=int, nargs="+", default=None, metavar="N",
                    help="the legs of profiles/fused_step_numeric.md instead: the default DeepFM with N numeric embedding columns")
    args = ap.parse_args()
    cells = []
    for name, voc, E, hidden, batches, *kw in (numeric_cases(args.numeric) if args.numeric else RULE_CASES if args.rules else CASES):
        for B in batches:
            eager, graph, fused = engines(voc, E, hidden, 3, **(kw[0] if kw else {}))
            nd = fused.n_numeric
            g = torch.Generator(device="cuda")
            g.manual_seed(1)
            ring = []
            for _ in range(ROTATE):
                ids = torch.stack([torch.randint(0, v, (B,), device="cuda", generator=g) for v in voc], 1).to(torch.int32).contiguous()
                ring.append((ids, (torch.rand(B, device="cuda", generator=g) < 0.3).to(torch.uint8)) +
                            ((torch.randn(B, nd, device="cuda", generator=g),) if nd else ()))
            paths = [("eager (one launch per kernel)", eager.train_step), ("hipGraph replay", graph.graph_train_step)]
            if fused.fused_step_ok(B):
                paths.append(("fused (one launch)", fused.fused_train_step))

            def block(step, n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    step(*ring[i % ROTATE])
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n * 1e6

            for _, step in paths:                              # warm-up: every shape, the graph's capture, the ring once round
                block(step, 3 * ROTATE)
            times = {p: [] for p, _ in paths}
            for _ in range(args.blocks):
                for p, step in paths:
                    times[p].append(block(step, args.steps))
            state = fused.state_bytes()
            for p, _ in paths:
                t = np.asarray(times[p])
                cell = {"case": name, "E": E, "hidden": hidden, "B": B, "n_numeric": nd, "rows": fused.R, "state_bytes": state, "path": p,
                        "us_median": float(np.median(t)), "us_p10": float(np.percentile(t, 10)),
                        "us_p90": float(np.percentile(t, 90)), "blocks": args.blocks, "steps_per_block": args.steps}
                cells.append(cell)
                print("%-22s E=%2d %-13s B=%5d rows=%6d  %-30s %7.1f us/step  (p10 %.1f, p90 %.1f; %.0f steps/s)" % (
                    name, E, hidden, B, fused.R, p, cell["us_median"], cell["us_p10"], cell["us_p90"], 1e6 / cell["us_median"]),
                    flush=True)
            del eager, graph, fused
    if args.json:
        with open(args.json, "w") as f:
            json.dump(cells, f, indent=1)


if __name__ == "__main__":
    main()
