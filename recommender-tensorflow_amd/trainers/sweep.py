"""Grid search over small DeepFM models: ``python -m trainers.sweep``.

What one does with a model of trainers.deep_fm's default size is train it many times — a grid of learning rates, dropout
rates, embedding sizes and layer specs, several seeds.  With the reference that is M runs of trainers/deep_fm.py one
after the other; here the M members train SIDE BY SIDE: the data is read once, every batch's ids are transformed once and
every member takes its step on it in ONE kernel launch (mi355x_rec.population.FusedPopulation), member i's variables
being bit for bit those of a stand-alone ``trainers.deep_fm --fused-step on`` run with its hyper-parameters.

Every member is an ordinary Estimator of trainers.deep_fm.model_fn with model_dir = <job-dir>/member_<i>: its
checkpoints and export are accepted by ``trainers.deep_fm --restore``, ``trainers.predict`` and ``trainers.recommend``.
<job-dir>/sweep.json lists the members, best first.

--eval-every N: the held-out set is read and transformed once, kept on the device, and every N steps (and at the last) ALL
members are evaluated on all of it in one launch (FusedPopulation.evaluate): <job-dir>/sweep_eval.jsonl holds one line per
evaluation — the members' learning curves — and sweep.json names every member's best point.  --final-eval fused takes the
end-of-sweep metrics from that evaluation too, instead of one Estimator.evaluate per member.

--rank-metrics K [K ...]: after the final evaluation every member is also measured as a recommender — the exact rank of
every test user's positives among all items the user has not rated, for ALL members in one launch
(FusedPopulation.rank_targets) — and every row of sweep.json gains "ranking" (hit_rate@K, recall@K, ndcg@K, mrr,
mean_rank: what trainers.recommend --metrics-at reports for the member's directory); --select takes these names too.

--ensemble N: after the ranking, the N best members are served as ONE model (EnsemblePredictor: their mean logit, one launch
for all of them) over the test set; sweep.json gains "ensemble": its members and its metrics, next to the best member's.
With --rank-metrics the ensemble is measured as a recommender too: "ensemble" gains "ranking", the members' keys under the
ensemble's MEAN logit (EnsemblePredictor.rank_targets: what trainers.recommend --top N --mean-metrics-at reports).

--exact-auc: every evaluation of the population also COUNTS every member's correctly ranked (positive, negative) pairs on
the logits it has anyway (mi355x_rec.exact_auc.ExactAuc: one more launch for all members) and the members' metrics gain
"auc_exact" — free of the 200-bucket "auc"'s dependence on the scale of the logits, which between the members of a grid
over learning rates is a bias.  --gauc-by COLUMN (user_id is the usual choice) adds "gauc", the mean of every group's own
AUC weighted by the group's examples, and "gauc_groups".  --select takes auc_exact and gauc with the matching flag.
--auc-method sorted counts the same integers by sorting every member's logits on the device (mi_auc_sorted_counts) instead
of comparing every pair: the way for test sets of millions of examples.

--optimizer NAME [NAME ...]: model_fn's params["optimizer"] joins the grid — any of model_utils.get_optimizer's Adagrad,
Adam, Ftrl, RMSProp and SGD; the members of one population may differ in it (the one-launch step applies each member's own
rule).  Without the flag every member trains under Adam and its hyper-parameters carry no "optimizer" key.

trainers.deep_fm has neither a learning-rate nor an optimizer flag (the reference has none): a member restored through
``trainers.deep_fm --restore`` continues at that CLI's 0.001 and under ITS optimizer, Adam (whose slots are not the ones an
Adagrad, Ftrl, RMSProp or SGD member saved); a member restored through ``trainers.sweep --restore`` with the flags it was
made with continues at its own rate under its own optimizer."""
import itertools
import json
import os
import re
import shutil
import time
from argparse import ArgumentParser, ArgumentTypeError

import numpy as np
import torch

from mi355x_rec.estimator import Estimator, ModeKeys
from mi355x_rec.exact_auc import ExactAuc
from mi355x_rec.metrics import metrics_from_counters, ranking_metrics_from_ranks
from mi355x_rec.predictor import EnsemblePredictor
from mi355x_rec.population import FusedPopulation
from trainers import _cli, deep_fm
from trainers.conf_utils import get_exporter
from trainers.model_utils import _OPTIMIZERS
from trainers.ml_100k import _read_csv, get_feature_columns, get_input_fn, serving_input_fn

_KEPT = ("--train-csv", "--test-csv", "--restore", "--batch-size", "--train-steps", "--device", "--catchup", "--synthetic",
         "--device-transform")
_ASCENDING = ("loss", "average_loss", "mean_rank")
_EVAL_METRICS = ("auc", "accuracy", "auc_precision_recall", "loss", "average_loss")
_EXACT_METRICS = ("auc_exact", "gauc")      # of --exact-auc / --gauc-by
_RANK_AT = re.compile(r"^(hit_rate|recall|ndcg)@([1-9][0-9]*)$")


def select_metric(name):
    """--select: an evaluation metric, or a ranking metric of --rank-metrics (hit_rate@K, recall@K, ndcg@K, mrr, mean_rank)"""
    if name in _EVAL_METRICS or name in _EXACT_METRICS or name in ("mrr", "mean_rank") or _RANK_AT.match(name):
        return name
    raise ArgumentTypeError("%r is none of %s, hit_rate@K, recall@K, ndcg@K, mrr, mean_rank" % (name, ", ".join(_EVAL_METRICS)))


def is_ranking(select):
    return select not in _EVAL_METRICS and select not in _EXACT_METRICS


def make_parser():
    p = ArgumentParser(description="Train the Cartesian product of the given hyper-parameters as one population of DeepFM "
                                   "models, one kernel launch per step for all of them.  No step of a sweep records layer "
                                   "summaries (the fused kernel keeps no activations).  A member restored through "
                                   "trainers.deep_fm --restore continues at that CLI's learning rate of 0.001; through "
                                   "trainers.sweep --restore at its own.")
    p.add_argument("--job-dir", default="checkpoints/sweep", help="job directory; member i lives in <job-dir>/member_<i> "
                                                                  "(default: %(default)s)")
    for flag, kw in _cli._COMMON:
        if flag in _KEPT:
            p.add_argument(flag, **kw)
    for name in ("exclude_linear", "exclude_mf", "exclude_dnn"):
        flag, kw = _cli._OPTIONAL[name]
        p.add_argument(flag, **kw)
    p.add_argument("--learning-rate", type=float, nargs="+", default=[0.001], help="Adam learning rates (default: %(default)s)")
    p.add_argument("--optimizer", nargs="+", default=None, choices=sorted(_OPTIMIZERS), metavar="NAME",
                   help="optimizers of the grid, model_fn's params[\"optimizer\"]: " + ", ".join(sorted(_OPTIMIZERS)) +
                        "; --learning-rate is then that optimizer's (default: Adam only)")
    p.add_argument("--dropout", type=float, nargs="+", default=[0.1], help="dropout rates (default: %(default)s)")
    p.add_argument("--embedding-size", type=int, nargs="+", default=[4], help="embedding sizes (default: %(default)s)")
    p.add_argument("--hidden-units", type=int, nargs="+", action="append", default=None,
                   help="a hidden layer specification; repeat the flag for several (default: 16 16)")
    p.add_argument("--seeds", type=int, default=1, metavar="N", help="seeds 0 .. N-1 of the variable initialisers and dropout "
                                                                     "masks (default: %(default)s)")
    p.add_argument("--select", default="auc", type=select_metric,
                   help="the metric sweep.json is sorted by, best first: auc, accuracy, auc_precision_recall, loss, average_loss "
                        "(loss / average_loss: lowest first), or with --rank-metrics hit_rate@K, recall@K, ndcg@K (K among "
                        "--rank-metrics), mrr, mean_rank (lowest first), or auc_exact with --exact-auc, gauc with --gauc-by "
                        "(default: %(default)s)")
    p.add_argument("--rank-metrics", type=int, nargs="+", default=None, metavar="K",
                   help="after the final evaluation, rank every test user's positives (rating >= 5) among all items the user "
                        "has not rated in the training file, for ALL members in one launch, and give every row of sweep.json "
                        "\"ranking\": hit_rate@K, recall@K, ndcg@K at these cutoffs, mrr and mean_rank (default: off)")
    p.add_argument("--eval-every", type=int, default=0, metavar="N",
                   help="evaluate every member on the whole test set every N steps and at the last step, in one launch for all "
                        "of them; one line per evaluation goes to <job-dir>/sweep_eval.jsonl and sweep.json gains best_step / "
                        "best_value by --select (default: 0 = off)")
    p.add_argument("--final-eval", default="layered", choices=["layered", "fused"],
                   help="where the end-of-sweep metrics come from: one Estimator.evaluate per member (layered) or the one-launch "
                        "population evaluation (fused) (default: %(default)s)")
    p.add_argument("--ensemble", type=int, default=0, metavar="N",
                   help="after the ranking, evaluate the mean of the N best members on the test set as one model and write it "
                        "to sweep.json as \"ensemble\" (default: 0 = off)")
    p.add_argument("--exact-auc", action="store_true",
                   help="count every member's exact AUC (the fraction of (positive, negative) pairs ranked the right way, ties "
                        "half) on the population evaluation's logits, one launch for all members: metrics gain auc_exact "
                        "(default: off)")
    p.add_argument("--gauc-by", default=None, metavar="COLUMN",
                   help="also the per-group AUC over the groups this column of the test file names by its raw values (user_id "
                        "is the usual choice): metrics gain gauc, the groups' AUCs weighted by their examples, and gauc_groups; "
                        "implies --exact-auc (default: off)")
    p.add_argument("--auc-method", default="pairs", choices=["pairs", "sorted"],
                   help="how --exact-auc / --gauc-by count (the same integers): pairs compares every (positive, negative) pair of "
                        "a test set laid out once, sorted sorts every member's logits on the device — the way for test sets of "
                        "millions (default: %(default)s)")
    return p


def evaluate_ensemble(ens, test_csv, batch_size=4096, exact=None):
    """The EVAL metrics of the mean of the sweep's best members (ens: EnsemblePredictor.from_sweep) over the test set: its
    logits through mi_eval_accumulate and metrics_from_counters, as Estimator.evaluate counts one model's.  "loss" is the
    average loss (the whole set as one batch of a mean reduction).  exact: the sweep's ExactAuc of the test set — the
    mean logits are counted by it too and the metrics gain its keys."""
    dev = ens.device
    hist = torch.zeros(2 * 201, dtype=torch.int64, device=dev)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    n = 0
    kept = []
    for features, labels in get_input_fn(test_csv, ModeKeys.EVAL, batch_size=batch_size)():
        ids, x = ens.plan.transform(features)
        z = torch.from_numpy(np.ascontiguousarray(ens.predict_ids(ids, x)["logits"][:, 0])).to(dev)
        y = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1)).astype(np.uint8)).to(dev)
        ens.k.mi_eval_accumulate(z, y, z.numel(), hist, counts, sums)
        n += z.numel()
        kept.append(z)
    if not n:
        raise ValueError("no evaluation data in %s" % test_csv)
    metrics = metrics_from_counters(hist.cpu().numpy(), counts.cpu().numpy(), sums.cpu().numpy())
    metrics["loss"] = metrics["average_loss"]
    if exact is not None:
        metrics.update(exact.metrics(torch.cat(kept))[0])
    return ens.sweep_members, {k: float(v) for k, v in metrics.items()}


def rank_tables(train_csv, test_csv):
    """The recommendation run trainers.recommend makes of the two files: (user features, item features, the test
    positives' candidate indices per user, the users' training items as an exclusion CSR pair)"""
    from trainers import recommend
    train, _ = _read_csv(train_csv)
    test, _ = _read_csv(test_csv)
    users, qf, items, cf = recommend.tables(train, test)
    return qf, cf, recommend.positive_targets(users, items, test), recommend.exclusion_csr(users, items, train)


def rank_population(pop, plan, train_csv, test_csv, ks):
    """Every member's ranking metrics as a recommender, what trainers.recommend --metrics-at reports for its directory:
    users, items, exclusions and test positives as that CLI builds them (rank_tables), the positives' exact ranks for all
    members of the population in ONE launch (FusedPopulation.rank_targets; a member outside that launch's scope is ranked
    on its own, and a line says so).  Returns a list of M dicts."""
    qf, cf, targets, excl = rank_tables(train_csv, test_csv)
    ranks = pop.rank_targets(plan, qf, cf, targets, exclude=excl, say=lambda text: print("INFO: --rank-metrics: %s" % text))
    n_pos = [len(t) for t in targets]
    return [ranking_metrics_from_ranks(r, n_pos, ks) for r in ranks]


def rank_ensemble(ens, train_csv, test_csv, ks):
    """rank_population for the ensemble's MEAN logit, what trainers.recommend --top N --mean-metrics-at reports: the
    positives' exact ranks on the same tables (EnsemblePredictor.rank_targets: one launch where the members allow it).
    Returns one dict with a member row's "ranking" keys."""
    qf, cf, targets, excl = rank_tables(train_csv, test_csv)
    return ranking_metrics_from_ranks(ens.rank_targets(qf, cf, targets, exclude=excl), [len(t) for t in targets], ks)


def grid(args):
    """The members' hyper-parameters: the Cartesian product of the flags, in the flags' order."""
    specs = args.hidden_units or [[16, 16]]
    if args.seeds < 1:
        raise ValueError("--seeds %d (at least 1)" % args.seeds)
    out = [dict(embedding_size=E, hidden_units=list(h), dropout=d, learning_rate=lr, seed=s)
           for E, h, d, lr, s in itertools.product(args.embedding_size, specs, args.dropout, args.learning_rate, range(args.seeds))]
    names = getattr(args, "optimizer", None)
    if names:                                     # (the key exists only with the flag: the default grid's dicts stay as they were)
        out = [dict(embedding_size=E, hidden_units=list(h), dropout=d, learning_rate=lr, optimizer=o, seed=s)
               for E, h, d, lr, o, s in itertools.product(args.embedding_size, specs, args.dropout, args.learning_rate, names,
                                                          range(args.seeds))]
    if len(out) > FusedPopulation.MAX_MEMBERS:
        raise ValueError("the grid has %d members (at most %d train in one launch): split the sweep" % (
            len(out), FusedPopulation.MAX_MEMBERS))
    return out


def member_flags(args, hp):
    """The flags that rebuild a member's model with the existing CLIs (trainers.deep_fm --restore --job-dir <member dir> ...)"""
    flags = ["--embedding-size", str(hp["embedding_size"]), "--hidden-units"] + [str(h) for h in hp["hidden_units"]] + [
        "--dropout", repr(hp["dropout"])]
    return flags + [f for f, on in (("--exclude-linear", args.exclude_linear), ("--exclude-mf", args.exclude_mf),
                                    ("--exclude-dnn", args.exclude_dnn)) if on]


def make_members(args, hps, config):
    """One Estimator of trainers.deep_fm.model_fn per member, model_dir = <job-dir>/member_<i>, with its own params"""
    members = []
    for i, hp in enumerate(hps):
        cols = get_feature_columns(embedding_size=hp["embedding_size"])
        params = {"categorical_columns": cols["linear"],
                  "use_linear": not args.exclude_linear, "use_mf": not args.exclude_mf, "use_dnn": not args.exclude_dnn,
                  "catchup": getattr(args, "catchup", "bounded"), "fused_step": "on",
                  "device_transform": getattr(args, "device_transform", "off")}
        if cols.get("numeric"):                   # (a feature-column set with numeric columns: DeepFM's numeric embeddings)
            params["numeric_columns"] = cols["numeric"]
        params.update(hp)
        members.append(Estimator(model_fn=deep_fm.model_fn, model_dir=os.path.join(args.job_dir, "member_%d" % i), config=config,
                                 params=params))
    return members


def build(members, features, labels, batch_size):
    """Every member's variables (model_fn's "_build" call: a stand-alone run's initial values for its params), its newest
    checkpoint if its directory holds one, and the checks a population asks for — before any step."""
    for i, est in enumerate(members):
        est._first_call(features, labels, ModeKeys.TRAIN)
        why = est._engine()._fused_step_limit(batch_size)
        if why is not None:
            hp = {k: est.params[k] for k in ("embedding_size", "hidden_units", "dropout", "learning_rate", "optimizer", "seed")
                  if k in est.params}
            raise ValueError("member %d (%s): the model has %s; a sweep trains models inside the fused step's scope" % (i, hp, why))
    steps = [est.global_step for est in members]
    if len(set(steps)) > 1:
        raise ValueError("the members are at different steps (%s): a sweep steps its members together" % ", ".join(
            "member %d at step %d" % (i, s) for i, s in enumerate(steps)))
    return FusedPopulation([est._engine() for est in members])


class PopulationEval:
    """The held-out set on the device and the members' curves on it: every run() is one FusedPopulation.evaluate (one launch
    for all members), one line of <job-dir>/sweep_eval.jsonl and one log line."""

    def __init__(self, test_csv, batch_size, select, job_dir, every=0, exact_auc=False, gauc_by=None, auc_method="pairs"):
        self.test_csv, self.batch_size, self.select, self.job_dir, self.every = test_csv, batch_size, select, job_dir, int(every)
        self.exact_auc, self.gauc_by, self.auc_method = bool(exact_auc or gauc_by), gauc_by, auc_method
        self.exact = None          # the test set's ExactAuc (--exact-auc / --gauc-by), made with the data
        self.path = os.path.join(job_dir, "sweep_eval.jsonl")
        self.data = None
        self.curve = []            # (global_step, [the members' metrics]), in step order
        if os.path.exists(self.path):                                   # (--restore: the curves carry on)
            with open(self.path) as f:
                self.curve = [(rec["global_step"], rec["members"]) for rec in map(json.loads, f)]

    def load(self, plan, dev):
        """the test set, read and transformed ONCE: ids int32 [N, F], the numeric columns' values float32 [N, nd] (None
        without any) and labels uint8 [N] on the device"""
        ids, xs, ys, groups = [], [], [], []
        for features, labels in get_input_fn(self.test_csv, ModeKeys.EVAL, batch_size=4096)():
            i_, x_ = _ids_x(plan, features, dev)
            ids.append(i_)
            xs.append(x_)
            ys.append(np.asarray(labels).reshape(-1).astype(np.uint8))
            if self.gauc_by:
                if self.gauc_by not in features:
                    raise SystemExit("--gauc-by %s: the test file has no such column (it has %s)" % (
                        self.gauc_by, ", ".join(sorted(features))))
                groups.append(np.asarray(features[self.gauc_by]).reshape(-1))
        if not ids:
            raise ValueError("no evaluation data in %s" % self.test_csv)
        if self.exact_auc:
            self.exact = ExactAuc(np.concatenate(ys), np.concatenate(groups) if self.gauc_by else None, device=dev,
                                  method=self.auc_method)
        self.data = (torch.cat(ids),
                     torch.from_numpy(np.ascontiguousarray(np.concatenate(ys))).to(dev),
                     None if xs[0] is None else torch.cat(xs).contiguous())

    def run(self, pop, step, lead):
        """All members on the whole test set at global step `step`; returns their metrics (at most once per step)"""
        newest = "gauc" if self.gauc_by else "auc_exact" if self.exact_auc else "auc"
        if self.curve and self.curve[-1][0] == step and newest in self.curve[-1][1][0]:
            return self.curve[-1][1]       # (--restore: a line of this step without the keys asked for now is measured again)
        if self.data is None:
            self.load(lead.params["_store"]["plan"], lead._engine().device)
        metrics = [{k: float(v) for k, v in m.items()} for m in pop.evaluate(self.data[0], self.data[1], batch_size=self.batch_size,
                                                                                     exact=self.exact, x_num=self.data[2])]
        self.curve.append((step, metrics))
        os.makedirs(self.job_dir, exist_ok=True)
        with open(self.path, "a") as f:
            f.write(json.dumps({"global_step": step, "members": metrics}) + "\n")
        vals = np.asarray([m[self.select] for m in metrics])
        best, worst = (vals.min(), vals.max()) if self.select in _ASCENDING else (vals.max(), vals.min())
        print("INFO: evaluation at step %d (%d members, %d examples): %s best = %.6f, median = %.6f, worst = %.6f" % (
            step, len(metrics), self.data[1].numel(), self.select, best, float(np.median(vals)), worst))
        return metrics

    def best(self, i):
        """(best_step, best_value) of member i's curve by the select metric; the earliest step among equals"""
        sign = 1.0 if self.select in _ASCENDING else -1.0
        curve = [rec for rec in self.curve if self.select in rec[1][i]]       # (--restore: earlier lines may lack auc_exact / gauc)
        step, ms = min(curve, key=lambda rec: (sign * rec[1][i][self.select], rec[0]))
        return step, ms[i][self.select]


def _ids_x(plan, features, dev):
    """a batch's ids int32 [B, F] and its numeric columns' values float32 [B, nd] (None when the feature-column set has no
    numeric column) on the device: made there from the raw columns (--device-transform on), or on the host"""
    if plan.device_mode == "on":
        return tuple(plan.on_device(dev).transform(features)[:2])
    ids, x = plan.transform(features)
    return torch.from_numpy(ids).to(dev), None if x is None else torch.from_numpy(x).to(dev)


def train(members, input_fn, max_steps, config, job_dir=None, batch_size=None, evaluator=None):
    """The sweep's loop: ONE input pipeline — every batch is read and its ids are transformed once (in groups, as
    Estimator._grouped does for small batches) — and one population step per batch.  evaluator: a PopulationEval whose
    run() is due every evaluator.every steps.  Returns the population."""
    lead = members[0]
    pop = None
    t_log = t_ckpt = time.time()
    n_log = 0
    log = None
    for features, labels in lead._grouped(input_fn()):
        if pop is None:
            pop = build(members, features, labels, batch_size or len(labels))
            plan, dev = lead.params["_store"]["plan"], lead._engine().device
        step = lead.global_step
        if step >= max_steps:
            break
        ahead = lead.params.get("_ahead")
        if ahead is not None and ahead.get("features") is features:
            g = ahead["group"]
            if "ids" not in g:
                g["ids"], g["x"] = _ids_x(plan, g["features"], dev)
                g["y"] = torch.from_numpy(np.ascontiguousarray(np.asarray(g["labels"]).reshape(-1)).astype(np.uint8)).to(dev)
            lo, hi = ahead["rows"]
            ids, y = g["ids"][lo:hi], g["y"][lo:hi]
            x = None if g["x"] is None else g["x"][lo:hi]
        else:
            ids, x = _ids_x(plan, features, dev)
            y = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1)).astype(np.uint8)).to(dev)
        loss, _ = pop.train_step(ids, y, x_num=x)
        step += 1
        n_log += 1
        if step % config.log_step_count_steps == 0:
            now = time.time()
            ls = loss.cpu().numpy()
            print("INFO: step = %d (%.1f global_step/sec, %d members), member loss lowest = %.6f, median = %.6f, highest = %.6f" % (
                step, n_log / max(now - t_log, 1e-9), len(members), ls.min(), float(np.median(ls)), ls.max()))
            if job_dir is not None:
                if log is None:
                    os.makedirs(job_dir, exist_ok=True)
                    log = open(os.path.join(job_dir, "sweep_log.jsonl"), "a")
                log.write(json.dumps({"global_step": step, "loss": [float(v) for v in ls]}) + "\n")
                log.flush()
            t_log, n_log = now, 0
        if evaluator is not None and evaluator.every > 0 and step % evaluator.every == 0:
            evaluator.run(pop, step, lead)
        if config.save_checkpoints_secs and time.time() - t_ckpt >= config.save_checkpoints_secs:
            for est in members:
                est.save_checkpoint()
            t_ckpt = time.time()
    if log is not None:
        log.close()
    return pop


def train_and_evaluate(args):
    if int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("trainers.sweep runs on one GPU: its members are small models that share it")
    if getattr(args, "synthetic", None):
        args.train_csv, args.test_csv = "synthetic:%d:1" % args.synthetic, "synthetic:%d:2" % max(args.synthetic // 10, 1)
    hps = grid(args)
    rank_ks = list(getattr(args, "rank_metrics", None) or [])
    if rank_ks and min(rank_ks) < 1:
        raise SystemExit("--rank-metrics %s: cutoffs are at least 1" % " ".join(str(k) for k in rank_ks))
    if is_ranking(args.select):
        at = _RANK_AT.match(args.select)
        if not rank_ks or (at and int(at.group(2)) not in rank_ks):
            raise SystemExit("--select %s needs --rank-metrics%s" % (args.select, " with %s among its cutoffs" % at.group(2) if at else ""))
    gauc_by = getattr(args, "gauc_by", None)
    exact_auc = bool(getattr(args, "exact_auc", False) or gauc_by)
    if args.select == "auc_exact" and not exact_auc:
        raise SystemExit("--select auc_exact needs --exact-auc")
    if args.select == "gauc" and not gauc_by:
        raise SystemExit("--select gauc needs --gauc-by")
    if not args.restore:
        shutil.rmtree(args.job_dir, ignore_errors=True)
    config = _cli.get_run_config()
    config.device = args.device
    members = make_members(args, hps, config)
    eval_every = int(getattr(args, "eval_every", 0) or 0)
    final_eval = getattr(args, "final_eval", "layered")
    if eval_every < 0:
        raise ValueError("--eval-every %d (0 = off, or a number of steps)" % eval_every)
    evaluator = None
    if eval_every or final_eval == "fused" or exact_auc:
        # (the curves are made of evaluation metrics: with a ranking --select their best point is taken by auc)
        evaluator = PopulationEval(args.test_csv, args.batch_size, "auc" if is_ranking(args.select) else args.select, args.job_dir,
                                   eval_every, exact_auc, gauc_by, getattr(args, "auc_method", "pairs"))
    pop = train(members, get_input_fn(args.train_csv, batch_size=args.batch_size), args.train_steps, config, args.job_dir,
                args.batch_size, evaluator)
    if pop is None:
        raise ValueError("no training data in %s" % args.train_csv)
    fused = None
    if evaluator is not None:
        fused = evaluator.run(pop, members[0].global_step, members[0])      # (the last step, unless it was just evaluated)
    eval_fn = get_input_fn(args.test_csv, ModeKeys.EVAL, batch_size=args.batch_size)
    exporter = get_exporter(serving_input_fn)
    rows = []
    for i, (est, hp) in enumerate(zip(members, hps)):
        est.save_checkpoint()
        if final_eval == "fused":
            metrics = dict(fused[i], global_step=est.global_step)
        else:
            metrics = est.evaluate(eval_fn)
            if exact_auc:          # (counted on the population evaluation's logits, whatever --final-eval says)
                metrics.update({k: v for k, v in fused[i].items() if k.startswith(("auc_exact", "gauc"))})
        export = exporter.export(est, os.path.join(est.model_dir, "export"))
        rows.append({"member": i, "dir": est.model_dir, "export": export, "global_step": est.global_step, "params": hp,
                     "flags": member_flags(args, hp), "metrics": {k: float(v) for k, v in metrics.items()}})
        if eval_every:
            rows[-1]["best_step"], rows[-1]["best_value"] = evaluator.best(i)
    if rank_ks:
        for row, ranking in zip(rows, rank_population(pop, members[0].params["_store"]["plan"], args.train_csv, args.test_csv, rank_ks)):
            row["ranking"] = ranking
    sign = 1.0 if args.select in _ASCENDING else -1.0
    value = lambda r: r["ranking" if is_ranking(args.select) else "metrics"][args.select]
    rows.sort(key=lambda r: (sign * value(r), r["member"]))
    doc = {"select": args.select, "members": rows}
    if exact_auc:
        gap = max(abs(r["metrics"]["auc"] - r["metrics"]["auc_exact"]) for r in rows)
        by = lambda key: [r["member"] for r in sorted(rows, key=lambda r: (-r["metrics"][key], r["member"]))]
        print("INFO: --exact-auc: the largest |auc - auc_exact| over the %d members is %.3g; the order of the members by auc "
              "and by auc_exact %s" % (len(rows), gap, "DIFFERS" if by("auc") != by("auc_exact") else "is the same"))
    with open(os.path.join(args.job_dir, "sweep.json"), "w") as f:
        json.dump(doc, f, indent=1)
    best = rows[0]
    n_ens = int(getattr(args, "ensemble", 0) or 0)
    if n_ens:
        if n_ens < 0 or n_ens > len(rows):
            raise ValueError("--ensemble %d: the sweep has %d members" % (n_ens, len(rows)))
        ens = EnsemblePredictor.from_sweep(args.job_dir, top=n_ens, device=args.device,
                                           device_transform=getattr(args, "device_transform", "off"))
        if exact_auc and evaluator.data is None:                        # (--restore with nothing left to evaluate)
            evaluator.load(members[0].params["_store"]["plan"], members[0]._engine().device)
        who, metrics = evaluate_ensemble(ens, args.test_csv, exact=evaluator.exact if exact_auc else None)
        doc["ensemble"] = {"members": who, "metrics": metrics}
        if rank_ks:
            doc["ensemble"]["ranking"] = rank_ensemble(ens, args.train_csv, args.test_csv, rank_ks)
        with open(os.path.join(args.job_dir, "sweep.json"), "w") as f:
            json.dump(doc, f, indent=1)
        shown = "auc" if is_ranking(args.select) else args.select      # (evaluation metrics here; a ranking --select: the line below)
        print("INFO: ensemble of the %d best members (%s): %s = %.6g, the best single member (member %d) has %.6g" % (
            n_ens, ", ".join(str(m) for m in who), shown, metrics[shown], best["member"], best["metrics"][shown]))
        if is_ranking(args.select):
            print("INFO: ensemble of the %d best members by its mean logit: %s = %.6g, the best single member (member %d) has %.6g" % (
                n_ens, args.select, doc["ensemble"]["ranking"][args.select], best["member"], value(best)))
    print("INFO: best of %d members by %s: member %d (%s), %s = %.6g, in %s" % (
        len(rows), args.select, best["member"], ", ".join("%s = %s" % kv for kv in sorted(best["params"].items())), args.select,
        value(best), best["dir"]))
    return members


if __name__ == "__main__":
    train_and_evaluate(make_parser().parse_args())
