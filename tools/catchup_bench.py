#!/usr/bin/env python3
"""The lazy Adam catch-up alone at config 3's size: 26 M rows x E = 64 (table + m + v = 20 GB), a batch's ~1.65 M distinct
rows with geometric gaps (mean 15 steps), sorted by staleness as the step does (mi_catchup_rows_by_gap), then
mi_sparse_catchup in the exact and the bounded-error form (deferred slots, as inside a train step).  HIP events.
MI_CATCHUP_BLOCKS sets the pipelined bounded kernel's grid."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "recommender-tensorflow_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mi355x_rec import _lib  # noqa: E402


def main():
    if os.environ.get("MI_TUNING_LIB"):          # the tools' build (make -C csrc tuning): reads MI_CATCHUP_BLOCKS
        _lib.LIB_PATH = os.path.join(ROOT, "tools", "probe", "libmi355x_rec_tuning.so")
    lib = _lib.load()
    dev = "cuda"
    R, E, U, step_to = 26_000_000, 64, 1_650_000, 400
    g = torch.Generator(device=dev); g.manual_seed(0)
    w = torch.randn(R, E, device=dev, generator=g) * 0.1
    m = torch.randn(R, E, device=dev, generator=g) * 1e-4
    v = torch.rand(R, E, device=dev, generator=g) * 1e-7 + 1e-9
    rec = torch.zeros(R, 4, device=dev)
    rec[:, 0].normal_(0, 0.01, generator=g); rec[:, 1].normal_(0, 1e-4, generator=g); rec[:, 2].uniform_(1e-9, 1e-7, generator=g)
    gaps = torch.empty(R, device=dev).geometric_(1.0 / 15.0, generator=g).clamp_(1, step_to - 1).to(torch.int32)
    stamps = (step_to - gaps).to(torch.int32)
    rec.view(torch.int32)[:, 3] = stamps
    last = rec.view(torch.int32)[:, 3]
    rows = torch.randperm(R, device=dev, generator=g)[:U].to(torch.int32).sort().values.contiguous()
    nu = torch.tensor([U], dtype=torch.int32, device=dev)
    lr = torch.from_numpy((1e-3 * np.sqrt(1 - 0.999 ** np.arange(step_to + 2)) / np.maximum(1 - 0.9 ** np.arange(step_to + 2), 1e-30)).astype(np.float32)).to(dev)
    by_gap = torch.empty(U, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mi_sort_unique_workspace_bytes(U) + 512, dtype=torch.uint8, device=dev)
    st = _lib.cur_stream
    _lib.check(lib.mi_catchup_rows_by_gap(rows.data_ptr(), nu.data_ptr(), last.data_ptr(), U, step_to, 4, by_gap.data_ptr(), ws.data_ptr(), ws.numel(), st()), "by_gap")
    w0 = w.clone()
    lin0 = rec[:, 0].clone()

    def run(flags, n=6, order=None):
        order = by_gap if order is None else order
        ts = []
        for _ in range(n):
            w.copy_(w0); rec[:, 0].copy_(lin0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            _lib.check(lib.mi_sparse_catchup(w.data_ptr(), m.data_ptr(), v.data_ptr(), None, None, None, last.data_ptr(),
                                             order.data_ptr(), nu.data_ptr(), U, E, step_to, lr.data_ptr(), 0.9, 0.999, 1e-8, flags, 4, 0, st()), "catchup")
            b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return min(ts), float(np.median(ts))

    elem_steps = float(gaps[rows.long()].double().sum().item()) * E
    for name, flags in (("exact", 1), ("bounded", 3)):
        best, med = run(flags)
        print("%-8s rows kernel: best %.3f ms, median %.3f ms  (%.2f G element-steps, 1.69 GB -> %.2f TB/s)" %
              (name, best, med, elem_steps / 1e9, U * 4 * E * 4 / best / 1e9), flush=True)
    # the same rows in ROW order: the four rows a wave holds then have unrelated staleness and every wave runs as long as its
    # stalest row — what a replay inside the gather (rows in example order) would see (round 4: VERDICT r3 item 3a)
    for name, flags in (("exact", 1), ("bounded", 3)):
        best, med = run(flags, order=rows)
        print("%-8s rows kernel, rows NOT sorted by staleness: best %.3f ms, median %.3f ms" % (name, best, med), flush=True)
    we = w.clone()
    run(1, 1); wx = w.clone()
    run(3, 1); wb = w.clone()
    d = (wb.double() - wx.double()).abs()
    print("bounded vs exact: bit-identical %.4f, max rel %.3g, frac > 1e-7 rel %.5f" %
          (float((wb == wx).float().mean()), float((d / wx.abs().clamp_min(1e-30)).max()), float((d > 1e-7 * wx.abs()).float().mean())))


if __name__ == "__main__":
    main()
