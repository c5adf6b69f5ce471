#!/usr/bin/env python3
"""Evaluating M small DeepFM models on one held-out set: ms per evaluation of

    A  one launch for all (population)    FusedPopulation.evaluate            (mi_eval_group; one device-to-host copy)
    B  per member and per batch           eng.loss followed by mi_eval_accumulate, one host finish per member
                                          (what model.run_batch does in EVAL mode for Estimator.evaluate: the device work of
                                          the end of a sweep before this path existed)

for the reference's default configuration (trainers.deep_fm: E=4, hidden [16,16], the 26 MovieLens fields) on N = 20,000
synthetic examples in batches of B = 32 (625 batches): the end of a trainers.sweep run at its defaults.

Protocol (tools/population_bench.py): both paths in ONE process on engines with identical state; a block
of B is one whole evaluation, from the call to the metrics on the host, on the host clock; a block of A is --a-evals such
evaluations one after the other (one alone is a window of a millisecond) and its time is divided by their number; blocks
of A and B alternate; per path the median and the 10th / 90th percentile over BLOCKS blocks.  A at every M; B only up to --b-max
members (it is linear in M: a block at M = 64 takes seconds).

    python tools/population_eval_bench.py [--json FILE] [--blocks N] [--members 1 8 64 256]
    python tools/population_eval_bench.py --only-a --members 64 --blocks 3      (under a kernel trace: path A alone)
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
from mi355x_rec.metrics import metrics_from_counters
from mi355x_rec.population import FusedPopulation

N = 20000
B = 32
VOCAB = [2] * 19 + [1000, 2000, 50, 1000, 7, 8, 3]


def engines(M):
    out = []
    for i in range(M):
        m = DeepFM(VOCAB, embedding_size=4, hidden_units=[16, 16], dropout=0.1, optimizer=OptimizerSpec("Adam", 0.001), seed=i)
        g = torch.Generator(device="cuda")
        g.manual_seed(i)
        m.init_variables(g, lin_scale=1e-3)
        out.append(m)
    return out


def layered_eval(members, batches):
    """path B: per member, per batch, the layered forward and the counters; the host finish once per member"""
    out = []
    for m in members:
        hist = torch.zeros(2 * 201, dtype=torch.int64, device="cuda")
        counts = torch.zeros(8, dtype=torch.int64, device="cuda")
        sums = torch.zeros(4, dtype=torch.float64, device="cuda")
        losses = []
        for ids, y in batches:
            loss, logits = m.loss(ids, y)
            m.k.mi_eval_accumulate(logits, y, ids.shape[0], hist, counts, sums)
            losses.append(loss.clone())
        r = metrics_from_counters(hist.cpu().numpy(), counts.cpu().numpy(), sums.cpu().numpy())
        r["loss"] = float(torch.stack(losses).mean())
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write every cell to this file")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--b-max", type=int, default=8, help="path B runs for at most this many members")
    ap.add_argument("--a-evals", type=int, default=20, help="evaluations in one block of path A")
    ap.add_argument("--only-a", action="store_true", help="path A alone (for a kernel trace)")
    args = ap.parse_args()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    ids = torch.stack([torch.randint(0, v, (N,), device="cuda", generator=g) for v in VOCAB], 1).to(torch.int32).contiguous()
    y = (torch.rand(N, device="cuda", generator=g) < 0.3).to(torch.uint8)
    batches = [(ids[lo:lo + B].contiguous(), y[lo:lo + B].contiguous()) for lo in range(0, N, B)]
    cells = []
    for M in args.members:
        members = engines(M)
        pop = FusedPopulation(members)
        paths = [("A: one launch for all", lambda: pop.evaluate(ids, y, batch_size=B), args.a_evals)]
        if not args.only_a and M <= args.b_max:
            paths.append(("B: per member and batch", lambda: layered_eval(members, batches), 1))

        def block(run, n=1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = run()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n, out

        first = [block(run)[1] for _, run, _ in paths]                      # (warm-up; and the two paths must agree)
        if len(first) == 2:
            worst = max(abs(a[k] - b[k]) for a, b in zip(*first) for k in ("auc", "accuracy", "average_loss", "loss"))
            print("M=%d: largest difference between the paths' auc / accuracy / average_loss / loss: %.2e" % (M, worst), flush=True)
        times = {p: [] for p, _, _ in paths}
        for _ in range(args.blocks):
            for p, run, n in paths:
                times[p].append(block(run, n)[0])
        for p, _, n in paths:
            t = np.asarray(times[p])
            cell = {"M": M, "N": N, "B": B, "path": p, "ms_median": float(np.median(t)), "ms_p10": float(np.percentile(t, 10)),
                    "ms_p90": float(np.percentile(t, 90)), "member_evaluations_per_s": M * 1e3 / float(np.median(t)),
                    "blocks": args.blocks, "evaluations_per_block": n}
            cells.append(cell)
            print("M=%3d  %-26s %10.3f ms/evaluation  (p10 %.3f, p90 %.3f; %.1f member-evaluations/s)" % (
                M, p, cell["ms_median"], cell["ms_p10"], cell["ms_p90"], cell["member_evaluations_per_s"]), flush=True)
        del pop, members
    if args.json:
        with open(args.json, "w") as f:
            json.dump(cells, f, indent=1)


if __name__ == "__main__":
    main()
