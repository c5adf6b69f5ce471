#!/usr/bin/env python3
"""The lazy Adam catch-up alone at config 3's size: 26 M rows x E = 64 (table + m + v = 20 GB), a batch's ~1.65 M distinct
rows with geometric gaps (mean 15 steps), sorted by staleness as the step does (mi_catchup_rows_by_gap), then
mi_sparse_catchup in the exact and the bounded-error form (deferred slots, as inside a train step).  HIP events.
MI_CATCHUP_BLOCKS sets the pipelined bounded kernel's grid.
Then the step's whole catch-up both ways: mi_catchup_rows_by_gap + the wide part's kernel + the bounded row kernel (three
calls, timed together and apart) against the ONE MI_CATCHUP_LOCAL_ORDER launch on the rows in the sort's row order — with
the replayed steps per wave of its windowed order (simulated on the host from the same gaps) against the ideal."""
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
    # ---- the step's whole catch-up: today's three calls against the one local-order launch
    def timed(calls, n=6):
        ts = []
        for _ in range(n):
            w.copy_(w0); rec[:, 0].copy_(lin0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for c in calls:
                c()
            b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return min(ts), float(np.median(ts))

    lw, lm, lv = rec[:, 0], rec[:, 1], rec[:, 2]

    def by_gap_call():
        _lib.check(lib.mi_catchup_rows_by_gap(rows.data_ptr(), nu.data_ptr(), last.data_ptr(), U, step_to, 4, by_gap.data_ptr(), ws.data_ptr(), ws.numel(), st()), "by_gap")

    def catchup_call(table, wide, order, flags):
        return lambda: _lib.check(lib.mi_sparse_catchup(
            w.data_ptr() if table else None, m.data_ptr() if table else None, v.data_ptr() if table else None,
            lw.data_ptr() if wide else None, lm.data_ptr() if wide else None, lv.data_ptr() if wide else None, last.data_ptr(),
            order.data_ptr(), nu.data_ptr(), U, E, step_to, lr.data_ptr(), 0.9, 0.999, 1e-8, flags, 4, 0, st()), "catchup")

    legs = (("rows_by_gap", [by_gap_call]), ("wide part alone (catchup_lin_k)", [catchup_call(False, True, by_gap, 3)]),
            ("bounded rows alone, sorted", [catchup_call(True, False, by_gap, 3)]),
            ("the three in sequence", [by_gap_call, catchup_call(False, True, by_gap, 3), catchup_call(True, False, by_gap, 3)]),
            ("LOCAL_ORDER, one launch (rows + wide part)", [catchup_call(True, True, rows, 3 | 8)]),
            ("LOCAL_ORDER, rows only", [catchup_call(True, False, rows, 3 | 8)]))
    for name, calls in legs:
        best, med = timed(calls)
        print("%-44s best %.3f ms, median %.3f ms" % (name, best, med), flush=True)
    timed(legs[3][1], 1); w3, l3 = w.clone(), rec[:, 0].clone()
    timed(legs[4][1], 1)
    print("LOCAL_ORDER vs the three calls: table bit-identical %s, wide part bit-identical %s" %
          (bool(torch.equal(w.view(torch.int32), w3.view(torch.int32))), bool(torch.equal(rec[:, 0].view(torch.int32), l3.view(torch.int32)))))
    # replayed steps per wave (E = 64: four rows per wave, a wave runs as long as its stalest row) over the ideal (the mean)
    ch, plan = int(lib.mi_catchup_local_chunk_rows()), np.zeros(3, np.int64)
    _lib.check(lib.mi_catchup_local_plan(U, U, plan.ctypes.data), "plan")
    G, ln = int(plan[0]), int(plan[2])
    gp = gaps[rows.long()].cpu().numpy().astype(np.int64)

    def per_wave(x):
        pad = (-len(x)) % 4
        return np.concatenate([x, np.zeros(pad, np.int64)]).reshape(-1, 4).max(1).sum() * 4

    def keyed(x):                 # the kernel's order: a counting sort on min(gap, 63)
        return x[np.argsort(np.minimum(x, 63), kind="stable")]

    local = sum(per_wave(keyed(gp[i:i + ln])) for i in range(0, U, ln))
    print("replayed steps per wave / ideal: unsorted %.3f, local order (%d workgroups, chunks of %d <= %d rows) %.3f, global sort %.3f" %
          (per_wave(gp) / gp.sum(), G, ln, ch, local / gp.sum(), per_wave(np.sort(gp)) / gp.sum()), flush=True)
    we = w.clone()
    run(1, 1); wx = w.clone()
    run(3, 1); wb = w.clone()
    d = (wb.double() - wx.double()).abs()
    print("bounded vs exact: bit-identical %.4f, max rel %.3g, frac > 1e-7 rel %.5f" %
          (float((wb == wx).float().mean()), float((d / wx.abs().clamp_min(1e-30)).max()), float((d > 1e-7 * wx.abs()).float().mean())))


if __name__ == "__main__":
    main()
