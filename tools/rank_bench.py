#!/usr/bin/env python3
"""Top-K recommendation: the fused path (DeepFM.top_k = per-side precompute + mi_pair_topk, whose launches are the
a_q / s_q transposes, pair_score_topk_k and topk_merge_k) against the materialised baseline (predict_logits over the
explicit pairs in query chunks, then torch.topk).  HIP events after warm-up, median over the timed iterations.  One
JSON line per shape:
  ml     U = 943, I = 1,682, E = 4, hidden [16, 16] (MovieLens-100k, the CLI default)
  large  U = 1,024, I = 65,536, E = 64, hidden [512, 256, 128]
26 fields split 5 (query) / 21 (candidate).  MLP FLOP/s: 2 * sum(fan_in * fan_out) over layers 2..L per pair, over the
mi_pair_topk time; its share of the 157.3 TF fp32 matrix peak.
usage: python tools/rank_bench.py [--shape ml|large|both] [--k 10] [--iters N] [--no-baseline]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mi355x_rec.engine import DeepFM  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
SHAPES = {"ml": dict(U=943, I=1682, E=4, hidden=[16, 16], vocab=2000, warmup=3, iters=20),
          "large": dict(U=1024, I=65536, E=64, hidden=[512, 256, 128], vocab=1 << 17, warmup=1, iters=5)}
QF = [0, 1, 2, 3, 4]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return float(np.median(ms))


def run(name, k, iters, baseline):
    c = SHAPES[name]
    U, I, E, hidden = c["U"], c["I"], c["E"], c["hidden"]
    iters = iters or c["iters"]
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    m = DeepFM([c["vocab"]] * 26, embedding_size=E, hidden_units=hidden, device="cuda")
    m.init_variables(g, lin_scale=0.01)
    q = torch.randint(0, c["vocab"], (U, 5), dtype=torch.int32, device="cuda", generator=g)
    cand = torch.randint(0, c["vocab"], (I, 21), dtype=torch.int32, device="cuda", generator=g)
    # the fused path: the whole call, and mi_pair_topk's share of it from the engine's own event brackets
    m.k.timers, m.k.timer_only = {}, {"mi_pair_topk"}
    fused_ms = timed(lambda: m.top_k(q, cand, QF, k), c["warmup"], iters)
    ev = m.k.timers["mi_pair_topk"][-iters:]
    pair_ms = float(np.median([s.elapsed_time(e) for s, e in ev]))
    m.k.timers = m.k.timer_only = None
    widths = [m.layers[0][3]] + [h for (_, _, _, h) in m.layers[1:]]
    mlp_flop = 2.0 * sum(a * b for a, b in zip(widths[:-1], widths[1:])) * U * I
    out = {"shape": name, "U": U, "I": I, "E": E, "hidden": hidden, "k": k, "fused_ms": round(fused_ms, 4),
           "precompute_ms": round(fused_ms - pair_ms, 4), "pair_topk_ms": round(pair_ms, 4),
           "pairs_per_s": U * I / (fused_ms * 1e-3), "mlp_tflops": mlp_flop / (pair_ms * 1e-3) / 1e12,
           "mlp_share_of_fp32_peak": mlp_flop / (pair_ms * 1e-3) / PEAK_FP32_MATRIX}
    if baseline:
        chunk = max(1, (1 << 20) // I)
        cols = torch.empty(chunk * I, 26, dtype=torch.int32, device="cuda")

        def materialised():
            res = []
            for u0 in range(0, U, chunk):
                n = min(chunk, U - u0)
                ids = cols[:n * I]
                ids[:, :5] = q[u0:u0 + n].repeat_interleave(I, 0)
                ids[:, 5:] = cand.repeat(n, 1)
                logits = m.predict_logits(ids).view(n, I)
                res.append(torch.topk(logits, k, 1))
            return res
        base_ms = timed(materialised, 1, max(2, iters // 4))
        out.update(baseline_ms=round(base_ms, 4), baseline_pairs_per_s=U * I / (base_ms * 1e-3),
                   speedup=base_ms / fused_ms)
        # the two paths pick the same candidates (up to near-ties)
        s_f, i_f = m.top_k(q[:8], cand, QF, k)
        ids = cols[:8 * I] if chunk >= 8 else torch.empty(8 * I, 26, dtype=torch.int32, device="cuda")
        ids[:, :5] = q[:8].repeat_interleave(I, 0)
        ids[:, 5:] = cand.repeat(8, 1)
        s_b = torch.topk(m.predict_logits(ids).view(8, I), k, 1).values
        out["max_abs_diff_top_scores"] = float((s_f - s_b).abs().max())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["ml", "large", "both"], default="both")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    for s in (["ml", "large"] if a.shape == "both" else [a.shape]):
        run(s, a.k, a.iters, not a.no_baseline)
