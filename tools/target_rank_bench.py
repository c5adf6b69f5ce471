#!/usr/bin/env python3
"""Ranking metrics for every member of a sweep: ONE engine.target_ranks_group call (per-side precompute per member + one
mi_pair_target_ranks launch for all members, then metrics.ranking_metrics_from_ranks per member) against the loop the
project had before it (per member DeepFM.top_k at k = 10, then trainers.recommend.ranking_metrics on the lists).
Shape: MovieLens-100k's, U = 943 users x I = 1,682 items, 10 held-out targets per user, the CLI-default member (E = 4, hidden
[16, 16], 26 fields split 5 query / 21 candidate), M in --members.

One process, the two legs alternating call by call after a warm-up; a leg's time is a host clock around work that ENDS on
the host (the device-to-host copy of the ranks or of the lists synchronises), once up to that copy and once including the
host metrics.  Blocks of --reps alternations: the table gives the median of the blocks' medians and the lowest and highest
block median (the run-to-run spread).  Both legs' hit_rate@10 / recall@10 / ndcg@10 are compared for every member: the
exact ranks must say what the lists say.
usage: python tools/target_rank_bench.py [--members 1 8 16 64] [--blocks 5] [--reps 5] [--out profiles/target_ranks.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

U, I, VOCAB, T, K = 943, 1682, 2000, 10, 10
QF = [0, 1, 2, 3, 4]
E, HIDDEN = 4, [16, 16]


def build(M, device="cuda"):
    import torch
    from mi355x_rec.engine import DeepFM
    g = torch.Generator(device=device)
    engines = []
    for i in range(M):
        g.manual_seed(i)
        m = DeepFM([VOCAB] * 26, embedding_size=E, hidden_units=HIDDEN, device=device)
        m.init_variables(g, lin_scale=0.01)
        engines.append(m)
    g.manual_seed(1000)
    q = torch.randint(0, VOCAB, (U, 5), dtype=torch.int32, device=device, generator=g)
    cand = torch.randint(0, VOCAB, (I, 21), dtype=torch.int32, device=device, generator=g)
    rng = np.random.default_rng(7)
    targets = np.stack([np.sort(rng.choice(I, T, replace=False)) for _ in range(U)])
    return engines, q, cand, targets


def legs(engines, q, cand, targets):
    """(one_call, loop): each returns (seconds up to the results on the host, seconds including the metrics, the members'
    metrics)"""
    from mi355x_rec import engine
    from mi355x_rec.metrics import ranking_metrics_from_ranks
    from trainers.recommend import ranking_metrics
    csr = (np.arange(U + 1, dtype=np.int64) * T, targets.reshape(-1))
    n_pos = [T] * U
    positives = {u: set(targets[u].tolist()) for u in range(U)}

    def one_call():
        t0 = time.perf_counter()
        ranks = engine.target_ranks_group(engines, q, cand, QF, csr).cpu().numpy()
        t1 = time.perf_counter()
        out = [ranking_metrics_from_ranks(r, n_pos, [K]) for r in ranks]
        return t1 - t0, time.perf_counter() - t0, out

    def loop():
        t0 = time.perf_counter()
        lists = [m.top_k(q, cand, QF, K)[1].cpu().numpy() for m in engines]
        t1 = time.perf_counter()
        out = [ranking_metrics({u: row.tolist() for u, row in enumerate(idx)}, positives, K) for idx in lists]
        return t1 - t0, time.perf_counter() - t0, out
    return one_call, loop


def measure(M, warmup, blocks, reps, device="cuda"):
    engines, q, cand, targets = build(M, device)
    fns = dict(zip(("one_call", "loop"), legs(engines, q, cand, targets)))
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    med = {(leg, part): [] for leg in fns for part in ("host", "metrics")}
    for _ in range(blocks):
        ms = {key: [] for key in med}
        for _ in range(reps):
            for leg, fn in fns.items():                                      # the legs alternate
                a, b, _ = fn()
                ms[(leg, "host")].append(1e3 * a)
                ms[(leg, "metrics")].append(1e3 * b)
        for key in med:
            med[key].append(float(np.median(ms[key])))
    one, lp = fns["one_call"]()[2], fns["loop"]()[2]
    names = ["hit_rate@%d" % K, "recall@%d" % K, "ndcg@%d" % K]
    row = {"M": M, "blocks": blocks, "reps": reps,
           "max_metric_diff": max(abs(a[n] - b[n]) for a, b in zip(one, lp) for n in names)}
    for (leg, part), v in med.items():
        row["%s_%s_ms" % (leg, part)] = [float(np.median(v)), min(v), max(v)]
    row["loop_over_one_call"] = row["loop_metrics_ms"][0] / row["one_call_metrics_ms"][0]
    return row


def table(rows):
    cell = lambda v: "%.3f (%.3f - %.3f)" % tuple(v)
    out = ["| M | one call: ranks on the host, ms | one call: with metrics, ms | loop: lists on the host, ms | loop: with metrics, ms | "
           "loop / one call (with metrics) | largest metric difference |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %s | %s | %s | %s | %.2f | %.3g |" % (
            r["M"], cell(r["one_call_host_ms"]), cell(r["one_call_metrics_ms"]), cell(r["loop_host_ms"]), cell(r["loop_metrics_ms"]),
            r["loop_over_one_call"], r["max_metric_diff"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 16, 64])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.blocks < 3 or a.reps < 3:
        raise SystemExit("--blocks %d --reps %d: medians are taken over at least 3 of each" % (a.blocks, a.reps))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/target_rank_bench.py measures on the GPU: none found")
    rows = []
    for M in a.members:
        rows.append(measure(M, a.warmup, a.blocks, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    text = ("# Ranking metrics for every sweep member: one counting launch against top-K lists member by member\n\n"
            "tools/target_rank_bench.py on one MI355X: U = %d, I = %d, %d targets per user, E = %d, hidden %s, 26 fields split 5 / 21; "
            "the two legs alternate in one process after %d warm-up calls; host clock around work that ends with the results on "
            "the host; median of %d block medians of %d calls (lowest - highest block median).  one call = "
            "engine.target_ranks_group (per-side precompute per member + ONE mi_pair_target_ranks launch) and "
            "ranking_metrics_from_ranks per member; loop = per member DeepFM.top_k at k = %d and "
            "trainers.recommend.ranking_metrics.  The loop's lists end at k = %d; the one call's ranks also give every cutoff, mrr "
            "and mean_rank.\n\n" % (U, I, T, E, HIDDEN, a.warmup, a.blocks, a.reps, K, K) + table(rows) + "\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
