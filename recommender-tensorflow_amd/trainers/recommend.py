"""Top-K recommendation CLI: ``python -m trainers.recommend --model {deep_fm,linear,deep,linear_deep} --job-dir DIR``.

Restores the newest checkpoint a trainer wrote to --job-dir (the model's own flags, as given to that trainer, rebuild
the same estimator), ranks every item for every user of the test file on one GPU (Estimator.recommend: the user columns
are the query side, the item columns the candidate side) and writes ``user_id,rank,item_id,logit,probability`` rows.
Users are the distinct user_ids of --test-csv, items the distinct item_ids of --train-csv and --test-csv; each takes
its features from its first row.  A user's training items are excluded unless --include-seen.  hit_rate@K, recall@K
and ndcg@K over the test positives (rating >= 5, get_input_fn's cutoff; users with at least one positive) are printed
and saved next to the CSV.  ``--metrics-at K [K ...]`` adds the same three metrics at any cutoffs (above 256 too), mrr and
mean_rank, from the exact rank of every test positive among all eligible items (Estimator.rank_targets: one counting
launch, no list).

``--top N`` (with ``--model deep_fm``) ranks with an ensemble instead: --job-dir is then the job directory of a
``trainers.sweep`` run, the sweep's N best members are loaded from their exports (EnsemblePredictor.from_sweep) and every
item is ranked by the members' mean logit, in one launch where the members allow it (EnsemblePredictor.recommend).  The
output goes to ``<job-dir>/recommend/top<K>_ensemble<N>.csv`` with the same columns and the same ``_metrics.json``.
``--mean-metrics-at K [K ...]`` (with ``--top N``) adds what --metrics-at adds for one model, under the ensemble's mean
logit (EnsemblePredictor.rank_targets)."""
import csv
import json
import math
import os
import sys

import numpy as np

from trainers import _cli, deep, deep_fm, linear, linear_deep
from trainers.conf_utils import get_run_config
from trainers.ml_100k import _read_csv, get_feature_columns

MODELS = {
    "deep_fm": (deep_fm, ("exclude_linear", "exclude_mf", "exclude_dnn", "hidden_units", "dropout")),
    "linear": (linear, ()),
    "deep": (deep, ("hidden_units", "dropout")),
    "linear_deep": (linear_deep, ("hidden_units", "dropout")),
}
QUERY_KEYS = ("user_id", "age", "gender", "occupation", "zipcode")
CUTOFF = 5


def make_parser(model):
    p = _cli.make_parser(model, MODELS[model][1])
    p.add_argument("--model", choices=sorted(MODELS), required=True, help="the trainer whose checkpoint --job-dir holds")
    p.add_argument("--top-k", type=int, default=10, help="items per user (default: %(default)s)")
    p.add_argument("--include-seen", action="store_true", help="also rank the items a user rated in the training file")
    p.add_argument("--output", default=None, help="CSV to write (default: <job-dir>/recommend/top<K>.csv; with --top: "
                                                   "<job-dir>/recommend/top<K>_ensemble<N>.csv)")
    p.add_argument("--top", type=int, default=None, metavar="N",
                   help="rank with the ensemble of the N best members of the trainers.sweep run in --job-dir (--model deep_fm)")
    p.add_argument("--metrics-at", type=int, nargs="+", default=None, metavar="K",
                   help="also report hit_rate@K, recall@K and ndcg@K at these cutoffs (any K >= 1, above 256 too), mrr and "
                        "mean_rank, from the exact rank of every test positive among all eligible items "
                        "(Estimator.rank_targets); not with --top (default: off)")
    p.add_argument("--mean-metrics-at", type=int, nargs="+", default=None, metavar="K",
                   help="with --top N: what --metrics-at reports for one model, from the exact rank of every test positive "
                        "under the ensemble's MEAN logit (EnsemblePredictor.rank_targets) (default: off)")
    return p


def parse_args(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    pre = make_parser("deep_fm").parse_known_args([a for a in argv if a not in ("-h", "--help")])[0] \
        if any(a.startswith("--model") for a in argv) else None
    return make_parser(pre.model if pre is not None else "deep_fm").parse_args(argv)


def first_rows(cols, key):
    """distinct values of cols[key], ascending, and for each the index of its first row"""
    vals, first = np.unique(np.asarray(cols[key]), return_index=True)
    return vals, first


def tables(train, test):
    """(users, user features, items, item features) of the recommendation run: users = distinct test user_ids, items =
    distinct item_ids of train + test (in that row order), each with the features of its first row."""
    users, u_first = first_rows(test, "user_id")
    both = {k: np.concatenate([np.asarray(train[k]), np.asarray(test[k])]) for k in test}
    items, i_first = first_rows(both, "item_id")
    qf = {k: np.asarray(test[k])[u_first] for k in QUERY_KEYS}
    cf = {k: v[i_first] for k, v in both.items() if k not in QUERY_KEYS}
    return users, qf, items, cf


def exclusion_csr(users, items, train):
    """per user (ascending users), the candidate indices of the items it has in the training file: (offsets, indices)"""
    pos = {int(v): i for i, v in enumerate(items)}
    seen = {}
    for u, it in zip(np.asarray(train["user_id"]), np.asarray(train["item_id"])):
        seen.setdefault(int(u), set()).add(pos[int(it)])
    rows = [sorted(seen.get(int(u), ())) for u in users]
    off = np.zeros(len(users) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.asarray([c for r in rows for c in r], np.int32)
    return off, idx


def positive_targets(users, items, test):
    """per user (ascending users), the candidate indices of the items it rates >= CUTOFF in the test file, ascending and
    distinct: the targets whose ranks the exact-rank metrics are made of"""
    pos = {int(v): i for i, v in enumerate(items)}
    liked = {}
    for u, it, r in zip(np.asarray(test["user_id"]), np.asarray(test["item_id"]), np.asarray(test["rating"])):
        if r >= CUTOFF:
            liked.setdefault(int(u), set()).add(pos[int(it)])
    return [sorted(liked.get(int(u), ())) for u in users]


def ranking_metrics(top_items, positives, k):
    """hit_rate@k, recall@k, ndcg@k (binary relevance) averaged over the users with at least one positive.
    top_items: user -> ranked item list; positives: user -> set of items."""
    hits, recalls, ndcgs = [], [], []
    for u, pos in positives.items():
        if not pos:
            continue
        ranked = list(top_items.get(u, []))[:k]
        rel = [1.0 if it in pos else 0.0 for it in ranked]
        n_hit = sum(rel)
        hits.append(1.0 if n_hit else 0.0)
        recalls.append(n_hit / len(pos))
        dcg = sum(r / math.log2(i + 2) for i, r in enumerate(rel))
        idcg = sum(1.0 / math.log2(i + 2) for i in range(min(len(pos), k)))
        ndcgs.append(dcg / idcg)
    n = len(hits)
    mean = lambda v: float(np.mean(v)) if v else 0.0
    return {"hit_rate@%d" % k: mean(hits), "recall@%d" % k: mean(recalls), "ndcg@%d" % k: mean(ndcgs), "users": n}


def main(argv=None):
    args = parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("trainers.recommend ranks on one GPU: run it without torch.distributed.run (WORLD_SIZE > 1)")
    k = args.top_k
    if not 1 <= k <= 256:
        raise SystemExit("--top-k %d outside [1, 256]" % k)
    if getattr(args, "synthetic", None):
        args.train_csv, args.test_csv = "synthetic:%d:1" % args.synthetic, "synthetic:%d:2" % max(args.synthetic // 10, 1)
    ens = None
    if args.metrics_at is not None:
        if args.top is not None:
            raise SystemExit("--metrics-at: not with --top %d: the exact-rank metrics rank by ONE model's logit; an ensemble's "
                             "mean logit is ranked through its top-K list only (--top-k)" % args.top)
        if min(args.metrics_at) < 1:
            raise SystemExit("--metrics-at %s: cutoffs are at least 1" % " ".join(str(v) for v in args.metrics_at))
    if args.mean_metrics_at is not None:
        if args.top is None:
            raise SystemExit("--mean-metrics-at: needs --top N: it ranks by an ensemble's mean logit; one model's exact-rank "
                             "metrics are --metrics-at")
        if min(args.mean_metrics_at) < 1:
            raise SystemExit("--mean-metrics-at %s: cutoffs are at least 1" % " ".join(str(v) for v in args.mean_metrics_at))
    if args.top is not None:
        from mi355x_rec.predictor import EnsemblePredictor
        if args.model != "deep_fm":
            raise SystemExit("--top %d: an ensemble is made of the members of a trainers.sweep run, which are deep_fm models "
                             "(--model %s)" % (args.top, args.model))
        if not os.path.exists(os.path.join(args.job_dir, "sweep.json")):
            raise SystemExit("--top %d: %s has no sweep.json (an ensemble is taken from the job directory of a trainers.sweep run)"
                             % (args.top, args.job_dir))
        with open(os.path.join(args.job_dir, "sweep.json")) as f:
            n_members = len(json.load(f)["members"])
        if not 1 <= args.top <= n_members:
            raise SystemExit("--top %d out of range: the sweep in %s has %d members (1 <= top <= %d)" % (
                args.top, args.job_dir, n_members, n_members))
        try:
            ens = EnsemblePredictor.from_sweep(args.job_dir, top=args.top, device=args.device,
                                               device_transform=args.device_transform)
        except ValueError as e:
            raise SystemExit("--top %d: %s" % (args.top, e))
    else:
        module = MODELS[args.model][0]
        config = get_run_config()
        config.device = args.device
        est = module.make_estimator(args, get_feature_columns(embedding_size=args.embedding_size), config)
        est.params["device_transform"] = args.device_transform      # (both sides' raw columns to the device, ids made there)
        if est.latest_checkpoint() is None:
            raise SystemExit("no checkpoint in %s: train the model first (python -m trainers.%s --job-dir %s ...)" % (
                args.job_dir, args.model, args.job_dir))
    train, _ = _read_csv(args.train_csv)
    test, _ = _read_csv(args.test_csv)
    users, qf, items, cf = tables(train, test)
    excl = None if args.include_seen else exclusion_csr(users, items, train)
    try:
        out = ens.recommend(qf, cf, k, exclude=excl) if ens is not None else est.recommend(qf, cf, k, exclude=excl)
    except ValueError as e:
        raise SystemExit("recommend: %s" % e)
    logits, probs, idx = out["logits"], out["probabilities"], out["indices"]
    path = args.output or os.path.join(args.job_dir, "recommend",
                                       "top%d.csv" % k if ens is None else "top%d_ensemble%d.csv" % (k, args.top))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    top = {}
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["user_id", "rank", "item_id", "logit", "probability"])
        for u in range(len(users)):
            top[int(users[u])] = []
            for r in range(k):
                if idx[u, r] < 0:
                    break
                it = int(items[idx[u, r]])
                top[int(users[u])].append(it)
                w.writerow([int(users[u]), r + 1, it, repr(float(logits[u, r])), repr(float(probs[u, r]))])
    positives = {}
    for u, it, r in zip(np.asarray(test["user_id"]), np.asarray(test["item_id"]), np.asarray(test["rating"])):
        if r >= CUTOFF:
            positives.setdefault(int(u), set()).add(int(it))
    m = ranking_metrics(top, positives, k)
    exact_at = args.metrics_at if ens is None else args.mean_metrics_at
    if exact_at is not None:
        from mi355x_rec.metrics import ranking_metrics_from_ranks
        targets = positive_targets(users, items, test)
        try:
            ranks = (est if ens is None else ens).rank_targets(qf, cf, targets, exclude=excl)
        except ValueError as e:
            raise SystemExit("recommend: %s" % e)
        exact = ranking_metrics_from_ranks(ranks, [len(t) for t in targets], exact_at)
        m.update({key: v for key, v in exact.items() if key not in m})      # (the top-K list's keys keep their values)
    m_path = os.path.splitext(path)[0] + "_metrics.json"
    with open(m_path, "w") as f:
        json.dump(m, f, indent=1)
    print("INFO: %d users x %d items -> %s; %s" % (len(users), len(items), path, ", ".join(
        "%s = %.6g" % (key, v) for key, v in m.items())))
    return m


if __name__ == "__main__":
    main()
