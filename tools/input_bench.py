#!/usr/bin/env python3
"""What the dataset on the device (mi355x_rec/dataset.py, mi_batch_gather, --device-dataset) gives end to end.  Writes
profiles/device_dataset.md (--out).  One MI355X; the legs of every comparison alternate; every step is a child process
under its own time limit, and after a child that ends on a signal or at its limit nothing more is started.

1  python -m trainers.deep_fm --synthetic 262144 --batch-size 65536 --train-steps 200, --device-dataset off / on times
   --device-transform off / on: the logged global_step/sec of the last 100 steps (both ends of that window wait for the
   device: the log line prints the loss).  --parent DIR: the same command in a checkout of the parent commit, alternating too.
2  tools/cli_speed.py (B = 32, the reference's defaults), the switch off and on.
3  mi_batch_gather alone between HIP events at B = 65,536, F = 26, against the torch.index_select calls it replaces and
   against its algorithmic bytes over 8 TB/s.
4  DeviceDataset.bind of 262,144 examples, host clock, ends synchronised, both transform modes.
5  Estimator.evaluate of the test data of 1 (26,214 examples, one batch) and of 2,000 examples in batches of 32: the plain
   input_fn against the dataset's (bound once).

    python tools/input_bench.py [--out FILE] [--rounds N] [--parent DIR] [--only 1,2,...]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "recommender-tensorflow_amd")
HBM_TBS = 8.0
PARENT_RATES = (15.1, 18.3)     # profiles/device_transform.md section 3: --device-transform off, on


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


class Trouble(Exception):
    pass


def child(cmd, limit, cwd=PKG, root=ROOT):
    """one step as a child process under its own time limit; its stdout.  A signal or the limit ends the whole bench."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "recommender-tensorflow_amd"), root]))
    print("[input_bench] %s" % " ".join(cmd[1:]), file=sys.stderr, flush=True)
    try:
        r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise Trouble("`%s` did not end within %d s" % (" ".join(cmd[1:]), limit))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        raise Trouble("`%s` ended with status %d: %s" % (" ".join(cmd[1:]), r.returncode, r.stderr[-400:]))
    if r.returncode:
        raise RuntimeError("`%s` failed (%d): %s" % (" ".join(cmd[1:]), r.returncode, r.stderr[-2000:]))
    return r.stdout


# ---- the measured children (python tools/input_bench.py --part NAME): one JSON line each -----------------------------------
def part_kernel():
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    from mi355x_rec.engine import HipKernels
    k = HipKernels()
    N, B, F = 262144, 65536, 26
    rng = np.random.default_rng(0)
    out = []
    for n_num in (0, 13):
        ids_all = torch.from_numpy(rng.integers(0, 10 ** 6, (N, F)).astype(np.int32)).cuda()
        x_all = torch.from_numpy(rng.standard_normal((N, max(n_num, 1))).astype(np.float32)).cuda()
        y_all = torch.from_numpy(rng.integers(0, 2, N).astype(np.uint8)).cuda()
        order = torch.from_numpy(rng.permutation(N)[:B].astype(np.int32)).cuda()
        ids = torch.empty(B, F, dtype=torch.int32, device="cuda")
        x = torch.empty(B, n_num, dtype=torch.float32, device="cuda") if n_num else None
        y = torch.empty(B, dtype=torch.uint8, device="cuda")
        status = torch.zeros(2, dtype=torch.int32, device="cuda")

        def ours():
            k.mi_batch_gather(ids_all, F, x_all if n_num else None, n_num, y_all, N, order, B, F, n_num, ids, x, y, status)

        def torchs():
            torch.index_select(ids_all, 0, order, out=ids)
            if n_num:
                torch.index_select(x_all, 0, order, out=x)
            torch.index_select(y_all, 0, order, out=y)
        ours()
        ref = (ids.clone(), None if x is None else x.clone(), y.clone())
        torchs()
        assert torch.equal(ref[0], ids) and torch.equal(ref[2], y) and (x is None or torch.equal(ref[1], x)) and int(status[0]) == 0

        def events(run, reps=100):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                run()
            e.record()
            e.synchronize()
            return s.elapsed_time(e) * 1e3 / reps
        a, b = [], []
        for _ in range(7):
            a.append(events(ours))
            b.append(events(torchs))
        nbytes = 4 * B + 2 * 4 * B * F + 2 * 4 * B * n_num + 2 * B
        out.append({"n_num": n_num, "ours_us": med(a), "torch_us": med(b), "calls": 3 if n_num else 2, "bytes": nbytes,
                    "floor_us": nbytes / (HBM_TBS * 1e12) * 1e6})
    print(json.dumps(out))


def part_bind():
    import numpy as np
    import torch
    import types
    sys.path.insert(0, PKG)
    from mi355x_rec.dataset import DeviceDataset
    from mi355x_rec.engine import HipKernels
    from mi355x_rec.feature_column import FieldPlan
    from trainers import ml_100k
    n = 262144
    cols, _ = ml_100k.synthetic_columns(n, 1)
    label = cols.pop("rating") >= 5
    eng = types.SimpleNamespace(device=torch.device("cuda", 0), k=HipKernels(), shard=None)
    times = {"off": [], "on": []}
    for rep in range(4):                                     # (the first round warms both up and is dropped)
        for mode in ("off", "on"):
            plan = FieldPlan(ml_100k.get_feature_columns()["linear"])
            plan.set_device_mode(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            DeviceDataset(cols, label, n).bind(plan, eng)
            torch.cuda.synchronize()
            if rep:
                times[mode].append(time.perf_counter() - t0)
    print(json.dumps({"n": n, "off_s": med(times["off"]), "on_s": med(times["on"])}))


def part_eval():
    import torch
    sys.path.insert(0, PKG)
    from mi355x_rec.estimator import Estimator, RunConfig
    from trainers import deep_fm, ml_100k
    out = []
    with tempfile.TemporaryDirectory() as job:
        for n, B in ((26214, 65536), (2000, 32)):
            est = Estimator(deep_fm.model_fn, model_dir=job, config=RunConfig(device="cuda"),
                            params={"categorical_columns": ml_100k.get_feature_columns()["linear"]})
            legs = {"plain": ml_100k.get_input_fn("synthetic:%d:2" % n, "eval", batch_size=B),
                    "dataset": ml_100k.get_input_fn("synthetic:%d:2" % n, "eval", batch_size=B, device_dataset=True)}
            times = {"plain": [], "dataset": []}
            got = {}
            for rep in range(6):                             # (the first round builds, binds and warms up and is dropped)
                for name, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    devnull = open(os.devnull, "w")
                    stdout, sys.stdout = sys.stdout, devnull
                    try:
                        got[name] = est.evaluate(fn)
                    finally:
                        sys.stdout = stdout
                        devnull.close()
                    torch.cuda.synchronize()
                    if rep:
                        times[name].append(time.perf_counter() - t0)
            # (the evaluation's fp64 sums are added by atomics across the workgroups of a batch of more than 1,024 examples: two
            # evaluations of the SAME inputs differ in their last bits there; the counters behind every other metric are integers)
            assert got["plain"].keys() == got["dataset"].keys(), got
            assert all(abs(got["plain"][m] - v) <= 1e-12 * abs(v) for m, v in got["dataset"].items()), got
            out.append({"n": n, "B": B, "plain_ms": med(times["plain"]) * 1e3, "dataset_ms": med(times["dataset"]) * 1e3})
    print(json.dumps(out))


# ---- the driver ---------------------------------------------------------------------------------------------------------
def section1(args, lines):
    legs = [("off", "off"), ("on", "off"), ("off", "on"), ("on", "on")]
    rates = {leg: [] for leg in legs}
    parent = []
    for _ in range(args.rounds):
        for ds, tr in legs:
            with tempfile.TemporaryDirectory() as job:
                out = child([sys.executable, "-m", "trainers.deep_fm", "--synthetic", "262144", "--batch-size", "65536", "--job-dir", job,
                             "--train-steps", "200", "--device-dataset", ds, "--device-transform", tr], 300)
            rates[(ds, tr)].append(float(re.findall(r"step = 200 \(([0-9.]+) global_step/sec\)", out)[-1]))
        if args.parent:
            with tempfile.TemporaryDirectory() as job:
                out = child([sys.executable, "-m", "trainers.deep_fm", "--synthetic", "262144", "--batch-size", "65536", "--job-dir", job,
                             "--train-steps", "200"], 300, cwd=os.path.join(args.parent, "recommender-tensorflow_amd"), root=args.parent)
            parent.append(float(re.findall(r"step = 200 \(([0-9.]+) global_step/sec\)", out)[-1]))
    base = med(parent) if parent else med(rates[("off", "off")])
    lines += ["## 1. `python -m trainers.deep_fm --synthetic 262144 --batch-size 65536 --train-steps 200`", "",
              "Logged global_step/sec of steps 101 to 200 (the log line prints the loss: both ends of the window wait for the device); "
              "%d runs a leg, alternating, each a fresh process; median (all runs).  A fast leg's window is a fraction of a second long." % args.rounds, "",
              "| --device-dataset | --device-transform | global_step/sec | ms per step | against the parent |", "|---|---|---:|---:|---:|"]
    if parent:
        lines.append("| (the parent commit, same session) | off | %.1f (%s) | %.2f | 1.0x |" % (base, ", ".join("%.1f" % r for r in parent), 1e3 / base))
    for leg in legs:
        r = med(rates[leg])
        lines.append("| %s | %s | %.1f (%s) | %.2f | %.1fx |" % (leg[0], leg[1], r, ", ".join("%.1f" % v for v in rates[leg]), 1e3 / r, r / base))
    note = "" if parent else ("  No parent checkout was given (--parent): the first row, the plain input pipeline, whose code this "
                              "change leaves as it was, stands for it.")
    lines += ["", "The parent's recorded figures (profiles/device_transform.md section 3): %.1f with --device-transform off, %.1f on.%s" % (
        PARENT_RATES + (note,)), ""]


def section2(args, lines):
    rates = {"off": [], "on": []}
    for _ in range(args.rounds):
        for flag in ("off", "on"):
            out = child([sys.executable, os.path.join(ROOT, "tools", "cli_speed.py"), "3000", "--device-dataset", flag], 300)
            rates[flag].append(float(re.findall(r"RESULT: .*?: ([0-9.]+) global_step/sec", out)[-1]))
    lines += ["## 2. `tools/cli_speed.py 3000` (B = 32, the reference's defaults; input parsing, final evaluation and export included)", "",
              "| --device-dataset | global_step/sec (all runs) |", "|---|---:|"]
    lines += ["| %s | %.0f (%s) |" % (f, med(rates[f]), ", ".join("%.0f" % v for v in rates[f])) for f in ("off", "on")] + [""]


def section3(args, lines):
    rows = json.loads(child([sys.executable, os.path.abspath(__file__), "--part", "kernel"], 300).strip().splitlines()[-1])
    lines += ["## 3. `mi_batch_gather` alone, B = 65,536 of N = 262,144 rows, F = 26, labels", "",
              "HIP events around 100 calls, median of 7 blocks, the two legs alternating; the results compared for equality first.  "
              "Bytes: the index stream, every output dword read once and written once; the floor is those bytes over %.0f TB/s." % HBM_TBS, "",
              "| n_num | mi_batch_gather | torch.index_select calls | bytes | floor | floor / measured |", "|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        lines.append("| %d | %.1f us | %.1f us (%d calls) | %.1f MB | %.2f us | %.0f %% |" % (
            r["n_num"], r["ours_us"], r["torch_us"], r["calls"], r["bytes"] / 1e6, r["floor_us"], 100 * r["floor_us"] / r["ours_us"]))
    lines.append("")


def section4(args, lines):
    r = json.loads(child([sys.executable, os.path.abspath(__file__), "--part", "bind"], 600).strip().splitlines()[-1])
    lines += ["## 4. `DeviceDataset.bind`, %d examples of ML-100k's 26 columns (once per run)" % r["n"], "",
              "Host clock, ends synchronised, median of 3 after a warm-up, the modes alternating.", "",
              "| --device-transform | bind |", "|---|---:|", "| off | %.2f s |" % r["off_s"], "| on | %.2f s |" % r["on_s"], ""]


def section5(args, lines):
    rows = json.loads(child([sys.executable, os.path.abspath(__file__), "--part", "eval"], 600).strip().splitlines()[-1])
    lines += ["## 5. One `Estimator.evaluate`", "",
              "Host clock, ends synchronised, median of 5 after the round that builds and binds, the legs alternating; the metrics agree to 1e-12 "
              "(integer counters; the fp64 sums of a batch above 1,024 examples are added by atomics in any order).  "
              "The plain input_fn makes the test data again at every evaluation (here: generates it; a CSV is read and parsed).", "",
              "| test examples | batch | plain input_fn | dataset | ratio |", "|---:|---:|---:|---:|---:|"]
    for r in rows:
        lines.append("| %d | %d | %.1f ms | %.1f ms | %.1fx |" % (r["n"], r["B"], r["plain_ms"], r["dataset_ms"], r["plain_ms"] / r["dataset_ms"]))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_dataset.md"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built (section 1 runs it too)")
    ap.add_argument("--only", default="1,2,3,4,5")
    ap.add_argument("--part", default=None, help="(a measured child of this script)")
    args = ap.parse_args()
    if args.part:
        return {"kernel": part_kernel, "bind": part_bind, "eval": part_eval}[args.part]()
    info = child([sys.executable, "-c", "import torch; from mi355x_rec import _lib; assert torch.cuda.is_available(), 'no GPU'; "
                  "print(_lib.load().mi_build_info().decode() + '; ' + torch.cuda.get_device_name(0))"], 300).strip().splitlines()[-1]
    lines = ["# The dataset on the device (tools/input_bench.py)", "", info + ".", ""]
    sections = {"1": section1, "2": section2, "3": section3, "4": section4, "5": section5}
    todo = [s for s in args.only.split(",") if s in sections]
    for i, s in enumerate(todo):
        try:
            sections[s](args, lines)
        except Trouble as e:
            lines += ["**Stopped at section %s: %s.  Sections %s: not measured yet.**" % (s, e, ", ".join(todo[i:])), ""]
            break
        except Exception as e:                               # (an ordinary failure of one section: the others still run)
            lines += ["**Section %s failed: %s.  Not measured yet.**" % (s, str(e)[-600:]), ""]
    missing = [s for s in sorted(sections) if s not in todo]
    if missing:
        lines += ["Sections %s were not run: **not measured yet**." % ", ".join(missing), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
