#!/usr/bin/env python3
"""M small DeepFM models, one training step each: us per step of

    A  one launch for all (population)    FusedPopulation.train_step          (mi_train_group_step)
    B  M launches, one per model          a Python loop of M DeepFM.fused_train_step calls on M engines

for the reference's default configuration (trainers.deep_fm: E=4, hidden [16,16], B=32, the 26 MovieLens fields, dropout
0.1) at M = 1 .. 256, one row with mixed members (half default, half E 16 [64, 64, 32]) at M = 16, and one row of 16 default
models under mixed optimizers (Adam, Adagrad, Ftrl on the wide part + Adagrad, RMSProp, SGD in turn: mi_train_group_plan_models).

Protocol (tools/small_step_bench.py): both paths in ONE process on engines with identical initial
state; every path walks the same ring of ROTATE different batches; a block is STEPS consecutive steps of one path between
two device synchronisations, timed on the host clock; blocks of A and B alternate; per path the median and the 10th /
90th percentile over BLOCKS blocks.

    python tools/population_bench.py [--json FILE] [--blocks N] [--steps N] [--members 1 2 4 ...]
    python tools/population_bench.py --only-a --members 64 --blocks 1      (under a kernel trace: path A alone)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
import numpy as np
import torch
from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.population import FusedPopulation

ROTATE = 8
B = 32
VOCAB = [2] * 19 + [1000, 2000, 50, 1000, 7, 8, 3]
DEFAULT, LARGE = (4, [16, 16]), (16, [64, 64, 32])


RULES = [dict(optimizer=OptimizerSpec("Adam", 0.001)), dict(optimizer=OptimizerSpec("Adagrad", 0.05)),
         dict(optimizer=OptimizerSpec("Adagrad", 0.05), linear_optimizer=OptimizerSpec("Ftrl", 0.2)),
         dict(optimizer=OptimizerSpec("RMSProp", 0.001)), dict(optimizer=OptimizerSpec("SGD", 0.05))]


def engines(shapes):
    out = []
    for i, (E, hidden, *kw) in enumerate(shapes):
        kw = kw[0] if kw else dict(optimizer=OptimizerSpec("Adam", 0.001))
        m = DeepFM(VOCAB, embedding_size=E, hidden_units=hidden, dropout=0.1, seed=i, **kw)
        g = torch.Generator(device="cuda")
        g.manual_seed(i)
        m.init_variables(g, lin_scale=1e-3)
        out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write every cell to this file")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64, 128, 256])
    ap.add_argument("--only-a", action="store_true", help="path A alone, default members only (for a kernel trace)")
    args = ap.parse_args()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    ring = []
    for _ in range(ROTATE):
        ids = torch.stack([torch.randint(0, v, (B,), device="cuda", generator=g) for v in VOCAB], 1).to(torch.int32).contiguous()
        ring.append((ids, (torch.rand(B, device="cuda", generator=g) < 0.3).to(torch.uint8)))
    cases = [("default", [DEFAULT] * M) for M in args.members]
    if not args.only_a:
        cases.append(("mixed: half default, half E 16 [64, 64, 32]", [DEFAULT, LARGE] * 8))
        cases.append(("mixed optimizers: default model, five rules in turn", [DEFAULT + (RULES[i % 5],) for i in range(16)]))
    cells = []
    for name, shapes in cases:
        M = len(shapes)
        pop = FusedPopulation(engines(shapes))
        solo = [] if args.only_a else engines(shapes)

        def step_b(ids, y):
            for m in solo:
                m.fused_train_step(ids, y)
        paths = [("A: one launch for all", pop.train_step)] + ([] if args.only_a else [("B: one launch per model", step_b)])

        def block(step, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                step(*ring[i % ROTATE])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6

        for _, step in paths:
            block(step, 2 * ROTATE)
        times = {p: [] for p, _ in paths}
        for _ in range(args.blocks):
            for p, step in paths:
                times[p].append(block(step, args.steps))
        for p, _ in paths:
            t = np.asarray(times[p])
            cell = {"case": name, "M": M, "B": B, "path": p, "us_median": float(np.median(t)), "us_p10": float(np.percentile(t, 10)),
                    "us_p90": float(np.percentile(t, 90)), "model_steps_per_s": M * 1e6 / float(np.median(t)),
                    "blocks": args.blocks, "steps_per_block": args.steps}
            cells.append(cell)
            print("%-44s M=%3d  %-24s %9.1f us/step  (p10 %.1f, p90 %.1f; %.0f model-steps/s)" % (
                name, M, p, cell["us_median"], cell["us_p10"], cell["us_p90"], cell["model_steps_per_s"]), flush=True)
        del pop, solo
    if args.json:
        with open(args.json, "w") as f:
            json.dump(cells, f, indent=1)


if __name__ == "__main__":
    main()
