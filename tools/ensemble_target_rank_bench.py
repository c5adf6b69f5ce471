#!/usr/bin/env python3
"""The exact rank of held-out targets under an ensemble's MEAN logit: ONE engine.target_ranks_mean call (per-side precompute
per member + one mi_pair_target_ranks_mean launch) against what the project had before it — engine.top_k_group with
return_scores=True (the [U, I] mean matrix written to HBM by the group launch) and the key count on it by torch comparisons
on the device (engine.ranks_from_scores).
Shape: MovieLens-100k's, U = 943 users x I = 1,682 items, 10 held-out targets per user, the CLI-default member (E = 4, hidden
[16, 16], 26 fields split 5 query / 21 candidate), M in --members.

One process, the two legs alternating call by call after a warm-up; a leg's time is a host clock around work that ENDS on
the host (the device-to-host copy of the ranks synchronises).  Blocks of --reps alternations: the table gives the median of
the blocks' medians and the lowest and highest block median (the run-to-run spread).  Both legs' integers are compared.
usage: python tools/ensemble_target_rank_bench.py [--members 1 2 8 16] [--blocks 5] [--reps 5] [--out profiles/ensemble_target_ranks.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

U, I, VOCAB, T = 943, 1682, 2000, 10
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
    """(one_call, matrix): each returns (seconds up to the ranks on the host, the ranks)"""
    import torch
    from mi355x_rec import engine
    csr = (np.arange(U + 1, dtype=np.int64) * T, targets.reshape(-1))

    def one_call():
        t0 = time.perf_counter()
        ranks = engine.target_ranks_mean(engines, q, cand, QF, csr).cpu().numpy()
        return time.perf_counter() - t0, ranks

    def matrix():
        t0 = time.perf_counter()
        z = engine.top_k_group(engines, q, cand, QF, 1, return_scores=True)[2]
        tg = torch.from_numpy(engine.dense_targets(csr, U, I)).to(z.device).long()
        ranks = engine.ranks_from_scores(z, tg, None)[0].cpu().numpy()
        return time.perf_counter() - t0, ranks
    return one_call, matrix


def measure(M, warmup, blocks, reps, device="cuda"):
    engines, q, cand, targets = build(M, device)
    fns = dict(zip(("one_call", "matrix"), legs(engines, q, cand, targets)))
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    med = {leg: [] for leg in fns}
    for _ in range(blocks):
        ms = {leg: [] for leg in fns}
        for _ in range(reps):
            for leg, fn in fns.items():                                      # the legs alternate
                ms[leg].append(1e3 * fn()[0])
        for leg in med:
            med[leg].append(float(np.median(ms[leg])))
    row = {"M": M, "blocks": blocks, "reps": reps,
           "equal_ranks": bool(np.array_equal(fns["one_call"]()[1], fns["matrix"]()[1]))}
    for leg, v in med.items():
        row["%s_ms" % leg] = [float(np.median(v)), min(v), max(v)]
    row["matrix_over_one_call"] = row["matrix_ms"][0] / row["one_call_ms"][0]
    return row


def table(rows):
    cell = lambda v: "%.3f (%.3f - %.3f)" % tuple(v)
    out = ["| M | one call: ranks on the host, ms | mean matrix + torch key count: ranks on the host, ms | matrix / one call | "
           "equal integers |", "|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %s | %s | %.2f | %s |" % (r["M"], cell(r["one_call_ms"]), cell(r["matrix_ms"]), r["matrix_over_one_call"],
                                                     "yes" if r["equal_ranks"] else "NO"))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 8, 16])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.blocks < 3 or a.reps < 3:
        raise SystemExit("--blocks %d --reps %d: medians are taken over at least 3 of each" % (a.blocks, a.reps))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/ensemble_target_rank_bench.py measures on the GPU: none found")
    rows = []
    for M in a.members:
        rows.append(measure(M, a.warmup, a.blocks, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    text = ("# Exact target ranks under an ensemble's mean logit: one counting launch against the mean matrix and a torch key count\n\n"
            "tools/ensemble_target_rank_bench.py on one MI355X: U = %d, I = %d, %d targets per user, E = %d, hidden %s, 26 fields "
            "split 5 / 21; the two legs alternate in one process after %d warm-up calls; host clock around work that ends with the "
            "ranks on the host; median of %d block medians of %d calls (lowest - highest block median).  one call = "
            "engine.target_ranks_mean (per-side precompute per member + ONE mi_pair_target_ranks_mean launch); matrix = "
            "engine.top_k_group(k = 1, return_scores=True) — the same precompute, the group launch writing the [U, I] mean matrix "
            "— and engine.ranks_from_scores on it (torch comparisons on the device, one pass per target column).\n\n"
            % (U, I, T, E, HIDDEN, a.warmup, a.blocks, a.reps) + table(rows) + "\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
