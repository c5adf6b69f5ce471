#!/usr/bin/env python3
"""Ranking with an ensemble: the fused group call (engine.top_k_group = per-side precompute per member + ONE
mi_pair_topk_group) against the member-by-member baseline (M x DeepFM.top_k(return_scores=True), a torch fp32 mean of the
M [U, I] score matrices, torch.topk).  One process, the two legs alternating call by call, HIP events after a warm-up,
the median (and the 10th / 90th percentile: the run-to-run spread) over the timed iterations.  Shapes:
  ml     U = 943, I = 1,682, E = 4, hidden [16, 16], k = 10 (MovieLens-100k, the CLI default)
  large  U = 1,024, I = 65,536, the same model
26 fields split 5 (query) / 21 (candidate); M in --members.  Writes a markdown table (--out).

The kernel's own time comes from a separate run under the profiler, which this script only reads:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/ensemble_rank_bench.py --fused-only
  python tools/ensemble_rank_bench.py --kernel-trace DIR/.../run_kernel_trace.csv --out profiles/ensemble_rank.md --append
(--fused-only makes `--trace-calls` group calls per (shape, M) and nothing else; the trace is cut into those groups in
dispatch order).
usage: python tools/ensemble_rank_bench.py [--shape ml|large|both] [--members 1 4 8 16] [--iters 7] [--out FILE]"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SHAPES = {"ml": dict(U=943, I=1682, vocab=2000), "large": dict(U=1024, I=65536, vocab=1 << 17)}
QF = [0, 1, 2, 3, 4]
E, HIDDEN = 4, [16, 16]
KERNEL = "pair_score_topk_group_k"


def build(name, M):
    import torch
    from mi355x_rec.engine import DeepFM
    c = SHAPES[name]
    g = torch.Generator(device="cuda")
    engines = []
    for i in range(M):
        g.manual_seed(i)
        m = DeepFM([c["vocab"]] * 26, embedding_size=E, hidden_units=HIDDEN, device="cuda")
        m.init_variables(g, lin_scale=0.01)
        engines.append(m)
    g.manual_seed(1000)
    q = torch.randint(0, c["vocab"], (c["U"], 5), dtype=torch.int32, device="cuda", generator=g)
    cand = torch.randint(0, c["vocab"], (c["I"], 21), dtype=torch.int32, device="cuda", generator=g)
    return engines, q, cand


def legs(engines, q, cand, k):
    import torch
    from mi355x_rec import engine
    M = len(engines)

    def fused():
        return engine.top_k_group(engines, q, cand, QF, k)

    def baseline():
        acc = None
        for m in engines:
            z = m.top_k(q, cand, QF, k, return_scores=True)[2]
            acc = z if acc is None else acc + z
        return torch.topk(acc / torch.full_like(acc, float(M)), k, 1)
    return fused, baseline


def measure(name, M, k, warmup, iters):
    import torch
    engines, q, cand = build(name, M)
    fused, baseline = legs(engines, q, cand, k)
    for _ in range(warmup):
        fused()
        baseline()
    torch.cuda.synchronize()
    ms = {"fused": [], "baseline": []}
    for _ in range(iters):
        for leg, fn in (("fused", fused), ("baseline", baseline)):          # the legs alternate
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[leg].append(s.elapsed_time(e))
    # the two legs pick the same candidates (up to near-ties between the two summation paths)
    (s_f, i_f), (s_b, i_b) = fused(), baseline()
    row = {"shape": name, "U": SHAPES[name]["U"], "I": SHAPES[name]["I"], "M": M, "k": k, "iters": iters,
           "same_top1": float((i_f[:, 0].long() == i_b[:, 0]).float().mean()),
           "max_abs_diff_top_scores": float((s_f - s_b).abs().max())}
    for leg in ms:
        v = np.asarray(ms[leg])
        row.update({leg + "_ms": float(np.median(v)), leg + "_p10": float(np.percentile(v, 10)), leg + "_p90": float(np.percentile(v, 90))})
    row["speedup"] = row["baseline_ms"] / row["fused_ms"]
    return row


def table(rows):
    out = ["| shape | U x I | M | fused ms (p10 - p90) | baseline ms (p10 - p90) | baseline / fused | same top-1 |",
           "|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %s | %d x %d | %d | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.4f |" % (
            r["shape"], r["U"], r["I"], r["M"], r["fused_ms"], r["fused_p10"], r["fused_p90"], r["baseline_ms"],
            r["baseline_p10"], r["baseline_p90"], r["speedup"], r["same_top1"]))
    return "\n".join(out)


def kernel_table(path, shapes, members, calls):
    """the group kernel's own time per (shape, M) from a kernel trace of a --fused-only run: its dispatches in order, `calls`
    per (shape, M), the first of each group (the warm-up) left out"""
    with open(path, newline="") as f:
        ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f) if KERNEL in r["Kernel_Name"]]
    ev.sort()
    groups = [(s, M) for s in shapes for M in members]
    if len(ev) != calls * len(groups):
        raise SystemExit("%s: %d dispatches of %s, expected %d x %d" % (path, len(ev), KERNEL, calls, len(groups)))
    out = ["| shape | M | %s us (median of %d) | per member us |" % (KERNEL, calls - 1), "|---|---|---|---|"]
    for g, (s, M) in enumerate(groups):
        d = [(e - b) / 1e3 for b, e in ev[g * calls + 1:(g + 1) * calls]]
        out.append("| %s | %d | %.1f | %.1f |" % (s, M, float(np.median(d)), float(np.median(d)) / M))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["ml", "large", "both"], default="both")
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--fused-only", action="store_true", help="only --trace-calls group calls per (shape, M): for the profiler")
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--kernel-trace", default=None, help="kernel_trace.csv of a --fused-only run: write the kernel's own times")
    a = ap.parse_args()
    if a.iters < 7:
        raise SystemExit("--iters %d: the median is taken over at least 7" % a.iters)
    shapes = ["ml", "large"] if a.shape == "both" else [a.shape]
    if a.kernel_trace:
        text = "\n## The kernel's own time (rocprofv3 --kernel-trace, a run of its own)\n\n" + kernel_table(
            a.kernel_trace, shapes, a.members, a.trace_calls) + "\n"
    elif a.fused_only:
        import torch
        for s in shapes:
            for M in a.members:
                engines, q, cand = build(s, M)
                fused, _ = legs(engines, q, cand, a.k)
                for _ in range(a.trace_calls):
                    fused()
                torch.cuda.synchronize()
        return
    else:
        rows = []
        for s in shapes:
            for M in a.members:
                rows.append(measure(s, M, a.k, a.warmup, a.iters))
                print(json.dumps(rows[-1]), flush=True)
        text = ("# Ranking with an ensemble: one group launch against member-by-member\n\n"
                "tools/ensemble_rank_bench.py: E = %d, hidden %s, k = %d, 26 fields split 5 / 21; the two legs alternate in one "
                "process, HIP events, median of %d after %d warm-up calls (p10 - p90: the run-to-run spread).  fused = "
                "engine.top_k_group (per-side precompute per member + mi_pair_topk_group); baseline = M x "
                "top_k(return_scores=True), a torch fp32 mean, torch.topk.\n\n" % (E, HIDDEN, a.k, a.iters, a.warmup)
                + table(rows) + "\n")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
