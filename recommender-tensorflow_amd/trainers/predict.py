"""Serving CLI: ``python -m trainers.predict --job-dir DIR --input CSV [--output CSV] [--mode auto|fused|layered]``.

Scores the rows of a CSV in the training files' format (or ``synthetic:N[:seed]``) from the newest export under
``DIR/export/exporter`` and writes ``logit,probability,class_id`` per row.  It takes no model flags: the columns, the
model's parts and its sizes all come from the export (mi355x_rec/predictor.py).  The CSV's columns that the export's
signature does not receive (rating, timestamp, ...) are dropped here; the predictor itself refuses unknown keys.

``--top N`` on the job directory of a ``trainers.sweep`` run scores with the ensemble of the sweep's N best members
(EnsemblePredictor.from_sweep: the mean logit, one launch for all members in fused mode)."""
import csv
import os
import sys
from argparse import ArgumentParser

from mi355x_rec.predictor import EnsemblePredictor, Predictor
from trainers.ml_100k import _read_csv


def make_parser():
    p = ArgumentParser()
    p.add_argument("--job-dir", required=True, help="job directory of a trainer run (its export/exporter folder is read)")
    p.add_argument("--input", required=True, help="CSV in the training files' format, or synthetic:N[:seed]")
    p.add_argument("--output", default=None, help="CSV to write (default: <job-dir>/predict/predictions.csv)")
    p.add_argument("--mode", choices=["auto", "fused", "layered"], default="auto",
                   help="fused: the whole model as one launch; layered: the engine's forward; auto: the faster of the two "
                        "for the batch and the model (default: %(default)s)")
    p.add_argument("--top", type=int, default=None, metavar="N",
                   help="--job-dir is a trainers.sweep directory: score with the mean of its N best members (default: off, one "
                        "export is served)")
    p.add_argument("--device-transform", choices=["off", "on"], default="off",
                   help="on: a call's raw columns go to the device and become row ids there in one launch; off: the host "
                        "transform (default: %(default)s)")
    p.add_argument("--batch-size", type=int, default=4096, help="rows scored per call (default: %(default)s)")
    p.add_argument("--device", default="cuda", help="torch device of the MI355X to run on (default: %(default)s)")
    return p


def main(argv=None):
    args = make_parser().parse_args(sys.argv[1:] if argv is None else argv)
    if args.top is not None:
        if not os.path.exists(os.path.join(args.job_dir, "sweep.json")):
            raise SystemExit("--top %d: %s has no sweep.json (an ensemble is taken from the job directory of a trainers.sweep run)"
                             % (args.top, args.job_dir))
        predictor = EnsemblePredictor.from_sweep(args.job_dir, top=args.top, device=args.device, mode=args.mode,
                                                 device_transform=args.device_transform)
        predictor.export_dir = "the %d best members of %s (%s)" % (args.top, args.job_dir, ", ".join(
            "member %d" % m for m in predictor.sweep_members))
    else:
        predictor = Predictor.from_export(os.path.join(args.job_dir, "export", "exporter"), device=args.device, mode=args.mode,
                                          device_transform=args.device_transform)
    cols, n = _read_csv(args.input)
    cols = {k: v for k, v in cols.items() if k in predictor.receivers}
    out = args.output or os.path.join(args.job_dir, "predict", "predictions.csv")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["logit", "probability", "class_id"])
        for s in range(0, n, max(1, args.batch_size)):
            pr = predictor({k: v[s:s + args.batch_size] for k, v in cols.items()})
            for z, p, c in zip(pr["logits"][:, 0], pr["logistic"][:, 0], pr["class_ids"][:, 0]):
                w.writerow([repr(float(z)), repr(float(p)), int(c)])
    print("INFO: %d rows scored from %s (%s) -> %s" % (n, predictor.export_dir, args.mode, out))
    return out


if __name__ == "__main__":
    main()
