#!/usr/bin/env python3
"""The exact AUC / GAUC by sorting (mi_auc_sorted_counts, csrc/auc_sort.hip): what it costs at evaluation sizes from a
sweep's held-out set to a day of traffic, and where it overtakes the pair count.  Writes profiles/sorted_auc.md (--out).

One member, N in {2e4, 1e5, 1e6, 1e7, 4e7} examples (a quarter positive, logits normal(0, 3) + label), S in {1, 943, N / 20}
groups drawn uniformly.  Every leg starts from the logits on the device and ends with the numbers on the host (host clock):
  sorted   counts zeroed, mi_auc_sorted_counts, counts copied to the host — and the entry alone between HIP events, from
           which the sort's share of 8 TB/s is taken: algorithmic bytes (per pass the histogram's read and the scatter's read
           and write of 8 N bytes each; pass 0 reads the 4 + 1 (+ 4) bytes of an example instead) over the time of the WHOLE
           entry, the three count launches included — a lower bound of the sort's own share;
  (a)      counts zeroed, mi_auc_pair_counts on a plan made before (not timed), counts copied — where the set has at most
           --pairs-max pairs and the plan is accepted;
  (b)      logits.cpu() and the numpy midrank rank sum: what the README's exact-AUC bullet compares with;
  (c)      for information: the same words sorted by torch.sort and counted with cumsum / cummax on the device.
Then a scan of N between 3e4 and 8e4 with one group, sorted against (a) only: where the sort overtakes the pair count — the
number ExactAuc(method="auto") chooses by.
After a warm-up of every leg, per cell the median (p10, p90) over --blocks blocks, the legs alternating block by block in one
process; (b) at N >= 1e7 runs --slow-blocks blocks (a block takes seconds there).  The legs must agree before they are timed.

    python tools/sorted_auc_bench.py [--out FILE] [--sizes N ...] [--crossover N ...] [--blocks K] [--json FILE]
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
from mi355x_rec import _lib
from mi355x_rec.engine import HipKernels
from mi355x_rec.exact_auc import ExactAuc

SIZES = [20000, 100000, 1000000, 10000000, 40000000]
PEAK = 8.0e12            # bytes / s


def host_rank_sum(z, y, g, S):
    """per group the midrank rank sum, vectorised in numpy -> 2 U = 2 gt + eq of every group as float64 [S]"""
    o = np.lexsort((z, g))
    gs, zs, ys = g[o], z[o], y[o].astype(np.float64)
    new = np.r_[True, (gs[1:] != gs[:-1]) | (zs[1:] != zs[:-1])]
    run = np.cumsum(new) - 1
    cnt = np.bincount(run)
    start = np.r_[0, np.cumsum(cnt)[:-1]]
    size = np.bincount(gs, minlength=S)
    mid = (start + (cnt + 1) / 2.0)[run] - np.r_[0, np.cumsum(size)[:-1]][gs]
    P = np.bincount(gs, weights=ys, minlength=S)
    return 2.0 * (np.bincount(gs, weights=mid * ys, minlength=S) - P * (P + 1) / 2.0)


def torch_counts(z, y, g, S):
    """(c): the entry's words, torch.sort, and the run count with cumsum / cummax -> int64 [S, 2] on the device"""
    u = z.view(torch.int32).long() & 0xFFFFFFFF
    k = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    k = torch.where(z == 0, torch.full_like(k, 0x80000000), k)
    k = torch.where(z != z, torch.zeros_like(k), k)
    w = (k << 1) | y.long()
    if g is not None:
        w = w | (g.long() << 33)
    w = torch.sort(w).values
    neg = 1 - (w & 1)
    C = torch.cumsum(neg, 0) - neg
    idx = torch.arange(len(w), device=w.device)
    head = torch.ones_like(neg, dtype=torch.bool)
    head[1:] = (w[1:] >> 1) != (w[:-1] >> 1)
    ghead = torch.ones_like(head)
    ghead[1:] = (w[1:] >> 33) != (w[:-1] >> 33)
    c_run = C[torch.cummax(torch.where(head, idx, torch.zeros_like(idx)), 0).values]
    c_grp = C[torch.cummax(torch.where(ghead, idx, torch.zeros_like(idx)), 0).values]
    pos = (w & 1).bool()
    out = torch.zeros(S, 2, dtype=torch.int64, device=w.device)
    grp = (w >> 33)[pos]
    out[:, 0].index_add_(0, grp, (c_run - c_grp)[pos])
    out[:, 1].index_add_(0, grp, (C - c_run)[pos])
    return out


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


def host_ms(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def sort_bytes(N, S):
    """(passes, the sort's algorithmic bytes) of one member — the pass arithmetic of mi_auc_sorted_counts"""
    bits = 33
    while (1 << (bits - 33)) < S:
        bits += 1
    passes = -(-bits // 9)
    raw = 5 + (4 if S > 1 else 0)
    return passes, N * (2 * raw + 8) + (passes - 1) * 24 * N


def cell(k, N, S, args, rng, quick=False):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(N + S)
    yd = (torch.rand(N, device="cuda", generator=gen) < 0.25).to(torch.uint8)
    zd = torch.randn(N, device="cuda", generator=gen) * 3 + yd.float()
    gd = torch.randint(0, S, (N,), device="cuda", generator=gen, dtype=torch.int32) if S > 1 else None
    y = yd.cpu().numpy()
    g = gd.cpu().numpy().astype(np.int64) if S > 1 else np.zeros(N, np.int64)
    nbytes = int(k.query("mi_auc_sorted_workspace_bytes", N, S))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(1, S, 2, dtype=torch.int64, device="cuda")

    def entry():
        counts.zero_()
        k.mi_auc_sorted_counts(zd, N, 1, yd, gd, S, N, counts, ws, nbytes)

    def sorted_leg():
        entry()
        return counts.cpu().numpy()[0]

    size = np.bincount(g, minlength=S).astype(np.int64)
    n_pos = np.bincount(g, weights=y, minlength=S).astype(np.int64)
    pairs = int((n_pos * (size - n_pos)).sum())
    pairs_leg = None
    if pairs <= args.pairs_max:
        try:
            ex = ExactAuc(y, g if S > 1 else None, device="cuda", kernels=k)
            lay = ex.grouped if S > 1 else ex.whole
            pc = torch.zeros(1, lay.S, 2, dtype=torch.int64, device="cuda")

            def pairs_leg():
                pc.zero_()
                k.mi_auc_pair_counts(lay.plan, zd, N, 1, lay.order, pc)
                return pc.cpu().numpy()[0]
        except _lib.MiError as e:
            print("(a) refused at N = %d, S = %d: %s" % (N, S, e), flush=True)

    def host_leg():
        return host_rank_sum(zd.cpu().numpy(), y, g, S)

    def torch_leg():
        return torch_counts(zd, yd, gd, S).cpu().numpy()

    want = sorted_leg()                                                # warm-up; and the legs must agree
    assert quick or np.array_equal(torch_leg(), want)
    if S > 1 and pairs_leg is not None:                                # (ExactAuc numbers the groups by value: here the same numbers,
        assert len(ex.group_values) == S                               # where every group has an example)
    if pairs_leg is not None:
        assert np.array_equal(pairs_leg(), want)
    assert quick or np.array_equal(host_leg(), (2 * want[:, 0] + want[:, 1]).astype(np.float64))
    slow = N >= 10 ** 7
    te, ts, ta, tb, tc = [], [], [], [], []
    for b in range(args.blocks):
        te.append(events_ms(entry, args.reps if N <= 10 ** 6 else 3))
        ts.append(host_ms(sorted_leg)[0])
        if pairs_leg is not None:
            ta.append(host_ms(pairs_leg)[0])
        if quick:                                                      # (the crossover scan: sorted against (a) only)
            continue
        if not slow or b < args.slow_blocks:
            tb.append(host_ms(host_leg)[0])
        tc.append(host_ms(torch_leg)[0])
    passes, nb = sort_bytes(N, S)
    rec = {"N": N, "S": S, "passes": passes, "pairs": pairs, "entry_ms": stats(te), "sorted_ms": stats(ts),
           "pairs_ms": stats(ta) if ta else None, "host_ms": stats(tb) if tb else None, "host_blocks": len(tb),
           "torch_ms": stats(tc) if tc else None,
           "sort_bytes": nb, "share_of_8TBs": nb / (stats(te)[0] * 1e-3) / PEAK}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sorted_auc.md"))
    ap.add_argument("--json", default=None, help="also append one JSON line per cell to this file as the cells finish")
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--crossover", type=int, nargs="*", default=[30000, 40000, 50000, 60000, 80000],
                    help="sizes of the scan for the crossover with the pair count (one group)")
    ap.add_argument("--slow-blocks", type=int, default=3, help="blocks of leg (b) at N >= 1e7")
    ap.add_argument("--reps", type=int, default=10, help="calls of the entry between two HIP events (3 above N = 1e6)")
    ap.add_argument("--pairs-max", type=float, default=1.2e12, help="leg (a) runs up to this many pairs (about a second)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    assert args.blocks >= 7, "--blocks: at least 7"
    k = HipKernels()
    rng = np.random.default_rng(0)
    recs = []
    for N in args.sizes:
        for S in (1, 943, N // 20):
            recs.append(cell(k, N, S, args, rng))
            if args.json:
                with open(args.json, "a") as f:
                    f.write(json.dumps(recs[-1]) + "\n")
    fmt = lambda t: "-" if t is None else "%.3f (%.3f, %.3f)" % tuple(t)
    lines = ["# Exact AUC and GAUC at any evaluation size: sort the keys, count", "",
             "Written by `tools/sorted_auc_bench.py` on %s (%s).  DESIGN.md section 19." % (torch.cuda.get_device_name(0), torch.version.hip), "",
             "One member, a quarter positives, logits normal(0, 3) + label, groups drawn uniformly.  ms, median (p10, p90) over %d "
             "blocks, the legs alternating; every leg but `entry` goes from the logits on the device to the numbers on the host (host "
             "clock).  `entry`: `mi_auc_sorted_counts` alone between HIP events; `share`: the sort's algorithmic bytes over the "
             "whole entry's time, of 8 TB/s (a lower bound of the sort's own share: the count's three launches are in the time).  "
             "(a) `mi_auc_pair_counts` on a plan made before, where the set has at most %.3g pairs; (b) `logits.cpu()` + numpy "
             "midrank rank sum (%d blocks from N = 1e7); (c) for information, `torch.sort` + cumsum / cummax on the device." % (
                 args.blocks, args.pairs_max, args.slow_blocks), "",
             "| N | S | passes | pairs | entry | share | sorted | (a) pairs | (b) host | (c) torch | (a) / sorted | (b) / sorted | (c) / sorted |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in recs:
        s = r["sorted_ms"][0]
        lines.append("| %d | %d | %d | %.3g | %s | %.1f %% | %s | %s | %s | %s | %s | %.1fx | %.2fx |" % (
            r["N"], r["S"], r["passes"], r["pairs"], fmt(r["entry_ms"]), 100 * r["share_of_8TBs"], fmt(r["sorted_ms"]),
            fmt(r["pairs_ms"]), fmt(r["host_ms"]), fmt(r["torch_ms"]),
            "-" if r["pairs_ms"] is None else "%.2fx" % (r["pairs_ms"][0] / s), r["host_ms"][0] / s, r["torch_ms"][0] / s))
    # where the sort overtakes the pair count: one group (the whole set is what ExactAuc always counts), N between the
    # table's first two sizes
    scan = [cell(k, N, 1, args, rng, quick=True) for N in args.crossover]
    ahead = [r for r in scan if r["pairs_ms"] is None or r["sorted_ms"][0] < r["pairs_ms"][0]]
    lines += ["", "## Where the sort overtakes the pair count", "",
              "One group, sorted against (a) only, as above.", "",
              "| N | pairs | sorted | (a) pairs | (a) / sorted |", "|---:|---:|---:|---:|---:|"]
    for r in scan:
        lines.append("| %d | %d | %s | %s | %.2fx |" % (r["N"], r["pairs"], fmt(r["sorted_ms"]), fmt(r["pairs_ms"]),
                                                       r["pairs_ms"][0] / r["sorted_ms"][0]))
    lines += ["", "The sort is ahead from N = %d on: P x N- = %d pairs." % (ahead[0]["N"], ahead[0]["pairs"]) if ahead else
              "The pair count is ahead at every size of the scan.", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
