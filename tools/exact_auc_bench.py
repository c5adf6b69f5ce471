#!/usr/bin/env python3
"""The exact AUC / GAUC of a population's logits (mi355x_rec.exact_auc, mi_auc_pair_counts): what it costs and what it
changes.  Writes profiles/exact_auc.md (--out).

1  the kernel against what a user has today, N = 20,000 examples, one segment and 943 groups, M in {1, 8, 64}:
     A  mi_auc_pair_counts alone (zeroing its counts included): HIP events around --reps calls, ms per call;
     A' ExactAuc.metrics: from the logits on the device to the M dicts on the host (host clock, ends in the copy);
     B  today: copy the [M, N] logits to the host and take the midrank rank sum there with numpy (one lexsort per member),
        from the logits on the device to the M numbers on the host (host clock).
2  the cost added to an evaluation: FusedPopulation.evaluate without and with exact= (943 groups: both layouts), M = 8 and
   64, evaluation sets of 32 and 20,000 examples in batches of 32; host clock around whole evaluations.
3  (--sweep) what the metric changes: one trainers.sweep --synthetic 20000 over 4 learning rates x 4 seeds with --eval-every
   500 --exact-auc --gauc-by user_id: per member auc, auc_exact, gauc, the largest gap, whether the order of the members and
   any best_step differ.

Protocol: after a warm-up of every shape, per cell the median (p10, p90) over --blocks >= 7 blocks, the legs of a comparison
alternating block by block in one process.

    python tools/exact_auc_bench.py [--out FILE] [--blocks N] [--sweep] [--sweep-steps N]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
import numpy as np
import torch
from mi355x_rec.engine import DeepFM, OptimizerSpec
from mi355x_rec.exact_auc import ExactAuc
from mi355x_rec.population import FusedPopulation

N = 20000
GROUPS = 943
VOCAB = [2] * 19 + [1000, 2000, 50, 1000, 7, 8, 3]


def host_rank_sum(z, y, g, S):
    """today's way: per member the midrank rank sum per group, vectorised in numpy -> (auc of every group [S], weights)"""
    o = np.lexsort((z, g))
    gs, zs, ys = g[o], z[o], y[o].astype(np.float64)
    new = np.r_[True, (gs[1:] != gs[:-1]) | (zs[1:] != zs[:-1])]
    run = np.cumsum(new) - 1
    cnt = np.bincount(run)
    start = np.r_[0, np.cumsum(cnt)[:-1]]
    size = np.bincount(gs, minlength=S)
    mid = (start + (cnt + 1) / 2.0)[run] - np.r_[0, np.cumsum(size)[:-1]][gs]
    P = np.bincount(gs, weights=ys, minlength=S)
    Q = size - P
    U = np.bincount(gs, weights=mid * ys, minlength=S) - P * (P + 1) / 2.0
    both = (P > 0) & (Q > 0)
    return np.where(both, U / np.where(both, P * Q, 1.0), 0.0), np.where(both, size, 0)


def stats(t):
    t = np.asarray(t)
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def events_ms(run, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def host_ms(run, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def part1(args, lines):
    rng = np.random.default_rng(7)
    y = (rng.random(N) < 0.55).astype(np.uint8)
    users = rng.integers(0, GROUPS, N)
    lines += ["## 1. The kernel against the host rank sum", "",
              "N = %d examples (%d positives), logits normal(0, 3) + label; ms, median (p10, p90) over %d blocks." % (N, int(y.sum()), args.blocks),
              "A: `mi_auc_pair_counts` alone, HIP events around %d calls.  A': `ExactAuc.metrics`, logits on the device -> dicts on the host." % args.reps,
              "B: `logits.cpu()` + numpy midrank rank sum per member, logits on the device -> numbers on the host.",
              "With groups, A' and B give BOTH numbers (the whole set's AUC and the GAUC: two launches / two sorts per member); A is the "
              "grouped launch alone.", "",
              "| layout | M | pairs / member | items | A kernel | A' to the host | B host rank sum | B / A' |", "|---|---:|---:|---:|---:|---:|---:|---:|"]
    for name, groups, S in (("one segment", None, 1), ("%d groups" % GROUPS, users, GROUPS)):
        ex = ExactAuc(y, groups, device="cuda")
        lay = ex.whole if groups is None else ex.grouped
        g = np.zeros(N, np.int64) if groups is None else np.unique(users, return_inverse=True)[1].reshape(-1)
        pairs = int((lay.n_pos * lay.n_neg).sum())
        for M in (1, 8, 64):
            z = (rng.normal(0, 3, (M, N)) + y).astype(np.float32)
            zd = torch.from_numpy(z).cuda()
            counts = torch.zeros(M, S, 2, dtype=torch.int64, device="cuda")

            def kernel():
                counts.zero_()
                ex.k.mi_auc_pair_counts(lay.plan, zd, N, M, lay.order, counts)

            def to_host():
                return [(d["auc_exact"], d.get("gauc", 0.0)) for d in ex.metrics(zd)]

            def today():
                zh = zd.cpu().numpy()
                out = []
                for m in range(M):
                    auc = float(host_rank_sum(zh[m], y, np.zeros(N, np.int64), 1)[0][0])
                    gauc = 0.0
                    if groups is not None:
                        per, w = host_rank_sum(zh[m], y, g, S)
                        gauc = float((per * w).sum() / w.sum())
                    out.append((auc, gauc))
                return out

            kernel(); a = to_host(); b = today()                      # warm-up; and the legs must agree
            assert max(abs(u - v) for p, q in zip(a, b) for u, v in zip(p, q)) < 1e-12, (a[:2], b[:2])
            ta, tb, tc = [], [], []
            for _ in range(args.blocks):
                ta.append(events_ms(kernel, args.reps))
                tb.append(host_ms(to_host)[0])
                tc.append(host_ms(today)[0])
            fmt = lambda t: "%.3f (%.3f, %.3f)" % stats(t)
            lines.append("| %s | %d | %d | %d | %s | %s | %s | %.1fx |" % (name, M, pairs, lay.plan.n_items, fmt(ta), fmt(tb), fmt(tc),
                                                                           stats(tc)[0] / stats(tb)[0]))
            print(lines[-1], flush=True)
    lines.append("")


def part2(args, lines):
    rng = np.random.default_rng(1)
    lines += ["## 2. The cost added to an evaluation", "",
              "`FusedPopulation.evaluate` of CLI-default members (E = 4, hidden [16, 16], 26 fields) in batches of 32, without and with "
              "`exact=ExactAuc(labels, user_id)` (943 user groups: the whole-set and the grouped count, two launches, one more copy); "
              "ms per evaluation on the host clock, median (p10, p90) over %d blocks of %d evaluations, the legs alternating.  The "
              "count kernels' own time inside an evaluation was not measured separately (section 1 has it alone)." % (args.blocks, args.evals), "",
              "| M | examples | without exact | with exact | added | ratio |", "|---:|---:|---:|---:|---:|---:|"]
    for M in (8, 64):
        members = []
        for i in range(M):
            m = DeepFM(VOCAB, embedding_size=4, hidden_units=[16, 16], dropout=0.1, optimizer=OptimizerSpec("Adam", 0.001), seed=i)
            g = torch.Generator(device="cuda")
            g.manual_seed(i)
            m.init_variables(g, lin_scale=0.05)
            members.append(m)
        pop = FusedPopulation(members)
        for n in (32, N):
            ids = torch.from_numpy(np.stack([rng.integers(0, v, n) for v in VOCAB], 1).astype(np.int32)).cuda()
            y = (rng.random(n) < 0.45).astype(np.uint8)
            yd = torch.from_numpy(y).cuda()
            ex = ExactAuc(y, rng.integers(0, GROUPS, n), device="cuda")
            plain = lambda: pop.evaluate(ids, yd, batch_size=32)
            exact = lambda: pop.evaluate(ids, yd, batch_size=32, exact=ex)
            a, b = plain(), exact()
            assert all({k: q[k] for k in p} == p for p, q in zip(a, b))
            t0, t1 = [], []
            for _ in range(args.blocks):
                t0.append(host_ms(plain, args.evals)[0])
                t1.append(host_ms(exact, args.evals)[0])
            fmt = lambda t: "%.3f (%.3f, %.3f)" % stats(t)
            lines.append("| %d | %d | %s | %s | %.3f | %.2fx |" % (M, n, fmt(t0), fmt(t1), stats(t1)[0] - stats(t0)[0],
                                                                    stats(t1)[0] / stats(t0)[0]))
            print(lines[-1], flush=True)
        del pop, members
    lines.append("")


def part3(args, lines):
    from trainers import sweep
    job = tempfile.mkdtemp(prefix="exact_auc_sweep_")
    flags = ["--synthetic", "20000", "--learning-rate", "0.001", "0.003", "0.01", "0.03", "--seeds", "4", "--eval-every", "500",
             "--exact-auc", "--gauc-by", "user_id", "--train-steps", str(args.sweep_steps), "--final-eval", "fused", "--job-dir", job]
    t0 = time.perf_counter()
    sweep.train_and_evaluate(sweep.make_parser().parse_args(flags))
    took = time.perf_counter() - t0
    rows = json.load(open(os.path.join(job, "sweep.json")))["members"]
    curve = [json.loads(line) for line in open(os.path.join(job, "sweep_eval.jsonl"))]
    rows.sort(key=lambda r: r["member"])
    lines += ["## 3. What the metric changes", "",
              "`python -m trainers.sweep %s` (%.0f s); the test set has %d examples." % (" ".join(flags[:-2]), took, 2000), "",
              "| member | learning rate | seed | auc (200 buckets) | auc_exact | auc - auc_exact | gauc | groups | best_step by auc | by auc_exact | by gauc |",
              "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    best = lambda i, key: min(curve, key=lambda rec: (-rec["members"][i][key], rec["global_step"]))["global_step"]
    moved = 0
    for r in rows:
        m, i = r["metrics"], r["member"]
        steps = [best(i, k) for k in ("auc", "auc_exact", "gauc")]
        moved += len(set(steps[:2])) > 1
        lines.append("| %d | %g | %d | %.6f | %.6f | %+.2e | %.6f | %d | %d | %d | %d |" % (
            i, r["params"]["learning_rate"], r["params"]["seed"], m["auc"], m["auc_exact"], m["auc"] - m["auc_exact"], m["gauc"],
            m["gauc_groups"], steps[0], steps[1], steps[2]))
    by = lambda key: [r["member"] for r in sorted(rows, key=lambda r: (-r["metrics"][key], r["member"]))]
    gap = max(abs(r["metrics"]["auc"] - r["metrics"]["auc_exact"]) for r in rows)
    lines += ["", "Largest |auc - auc_exact|: %.3g.  Order of the members by auc: %s; by auc_exact: %s (%s); by gauc: %s.  best_step by auc "
              "and by auc_exact differ for %d of %d members." % (gap, by("auc"), by("auc_exact"),
                                                                "the same" if by("auc") == by("auc_exact") else "DIFFERENT", by("gauc"), moved, len(rows)), ""]
    print("\n".join(lines[-(len(rows) + 6):]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_auc.md"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls of the kernel between two HIP events")
    ap.add_argument("--evals", type=int, default=10, help="evaluations in one block of section 2")
    ap.add_argument("--sweep", action="store_true", help="also section 3: the sweep")
    ap.add_argument("--sweep-steps", type=int, default=3000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    assert args.blocks >= 7, "--blocks: at least 7"
    lines = ["# Exact AUC and GAUC of a population: pair counts in one launch", "",
             "Written by `tools/exact_auc_bench.py` on %s (%s).  DESIGN.md section 18." % (torch.cuda.get_device_name(0), torch.version.hip), ""]
    part1(args, lines)
    part2(args, lines)
    if args.sweep:
        part3(args, lines)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
