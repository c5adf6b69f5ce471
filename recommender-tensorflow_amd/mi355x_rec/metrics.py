"""Host-side finish of the streaming eval metrics (reference: the EVAL branch of
``head.create_estimator_spec``, trainers/deep_fm.py:118-125, and get_binary_metric_ops,
trainers/model_utils.py:39-54).  The device side (mi_eval_accumulate) only counts; the 200-threshold
trapezoidal AUC of tf.metrics.auc is a few hundred flops and is done here in fp64."""
import math

import numpy as np

NUM_THRESHOLDS = 200
_EPS = 1.0e-6


def confusion_from_hist(hist):
    """hist [2, 201]: hist[y, k] = examples of label y whose sigmoid exceeds exactly k thresholds.
    prediction is positive at threshold j iff k > j."""
    h = np.asarray(hist, np.int64).reshape(2, NUM_THRESHOLDS + 1)
    # tail[j] = sum_{k > j} h[k]
    tail = np.cumsum(h[:, ::-1], 1)[:, ::-1]
    tot = h.sum(1)
    pos_gt = tail[:, 1:]                 # [2, 200]: count with k > j, j = 0..199
    tp, fp = pos_gt[1], pos_gt[0]
    fn, tn = tot[1] - tp, tot[0] - fp
    return tp, fp, tn, fn


def _auc(tp, fp, tn, fn, curve):
    tp, fp, tn, fn = (a.astype(np.float64) for a in (tp, fp, tn, fn))
    rec = tp / (tp + fn + _EPS)
    if curve == "ROC":
        x, y = fp / (fp + tn + _EPS), rec
    else:
        x, y = rec, (tp + _EPS) / (tp + fp + _EPS)
    return float(np.sum((x[:-1] - x[1:]) * (y[:-1] + y[1:]) / 2.0))


def metrics_from_counters(hist, counts, sums):
    tp, fp, tn, fn = confusion_from_hist(hist)
    n = max(int(counts[0]), 1)
    n_pos, n_correct = int(counts[1]), int(counts[3])
    tp5, fp5, fn5 = int(counts[4]), int(counts[5]), int(counts[6])
    lm = n_pos / n
    return {
        "accuracy": n_correct / n,
        "accuracy_baseline": max(lm, 1 - lm),
        "auc": _auc(tp, fp, tn, fn, "ROC"),
        "auc_precision_recall": _auc(tp, fp, tn, fn, "PR"),
        "average_loss": float(sums[0]) / n,
        "label/mean": lm,
        "prediction/mean": float(sums[1]) / n,
        "precision": tp5 / max(tp5 + fp5, 1),
        "recall": tp5 / max(tp5 + fn5, 1),
    }


def auc_from_pair_counts(gt, eq, n_pos, n_neg):
    """The exact AUC of one set from mi_auc_pair_counts' two integers: of its n_pos * n_neg (positive, negative) pairs, gt
    have the positive's score higher and eq tie (half a pair each): (2 gt + eq) / (2 n_pos n_neg), one correctly rounded
    division of integers.  0.0 for a set with one class, as metrics_from_counters' "auc" is there."""
    pairs = int(n_pos) * int(n_neg)
    return (2 * int(gt) + int(eq)) / (2 * pairs) if pairs else 0.0


def exact_auc_from_counts(counts, n_pos, n_neg):
    """counts [1, 2] (or [2]) of the whole set as one segment -> {"auc_exact", "auc_exact_pairs"}"""
    gt, eq = np.asarray(counts, np.int64).reshape(-1)[:2]
    return {"auc_exact": auc_from_pair_counts(gt, eq, n_pos, n_neg), "auc_exact_pairs": int(n_pos) * int(n_neg)}


def gauc_from_counts(counts, n_pos, n_neg):
    """counts [S, 2], n_pos [S], n_neg [S] of S groups -> {"gauc", "gauc_groups"}: the mean of the groups' own exact AUCs
    weighted by the groups' numbers of examples, sum_u w_u AUC_u / sum_u w_u with w_u = n_pos[u] + n_neg[u], over the groups
    that have both classes (a group of one class has no AUC and no weight), added in fp64 in ascending group order;
    gauc_groups: how many groups counted.  0.0 when none did.  counts [M, S, 2] (M models on the same groups): a list of
    M such dicts."""
    counts = np.asarray(counts, np.int64)
    n_pos, n_neg = np.asarray(n_pos, np.int64).reshape(-1), np.asarray(n_neg, np.int64).reshape(-1)
    if counts.ndim not in (2, 3) or counts.shape[-1] != 2 or not counts.shape[-2] == len(n_pos) == len(n_neg):
        raise ValueError("gauc_from_counts: counts of shape %s for %d / %d group sizes" % (counts.shape, len(n_pos), len(n_neg)))
    both = (n_pos > 0) & (n_neg > 0)
    groups = int(both.sum())
    c = counts.reshape(-1, len(n_pos), 2)[:, both]
    if groups:
        w = (n_pos + n_neg)[both].astype(np.float64)
        auc = (2 * c[..., 0] + c[..., 1]).astype(np.float64) / (2 * n_pos * n_neg)[both].astype(np.float64)
        num = np.cumsum(w * auc, axis=1)[:, -1]           # (one addition after the other, in group order)
        gauc = num / np.cumsum(w)[-1]
    else:
        gauc = np.zeros(len(c))
    out = [{"gauc": float(v), "gauc_groups": groups} for v in gauc]
    return out if counts.ndim == 3 else out[0]


def histogram_limits():
    """TensorFlow's default histogram bucket limits (core/lib/histogram/histogram.cc InitDefaultBucketsInner,
    what tf.summary.histogram of layer_summary — model_utils.py:6 — bins with): 1e-12 * 1.1^k below 1e20,
    DBL_MAX, their negatives and 0; ascending, 1,551 values."""
    pos, v = [], 1.0e-12
    while v < 1.0e20:
        pos.append(v)
        v *= 1.1
    pos.append(np.finfo(np.float64).max)
    return np.asarray([-x for x in reversed(pos)] + [0.0] + pos, np.float64)


def histogram_proto(limits, counts, sums, vmin, vmax):
    """The fields of a tensorflow.HistogramProto, empty buckets dropped (bucket b holds limit[b-1] <= x < limit[b])"""
    counts = np.asarray(counts, np.int64)
    nz = np.flatnonzero(counts)
    lim = np.append(limits, np.finfo(np.float64).max)
    return {"min": float(vmin), "max": float(vmax), "num": int(counts.sum()), "sum": float(sums[0]), "sum_squares": float(sums[1]),
            "bucket_limit": [float(lim[b]) for b in nz], "bucket": [int(counts[b]) for b in nz]}


def ranking_metrics_from_ranks(ranks_by_user, n_positives_by_user, ks):
    """Ranking metrics from the exact 0-based ranks of every user's held-out positives (DeepFM.target_ranks) — no top-K
    list, so any cutoff and the list-free metrics are available.  ranks_by_user: one row per user (an int array [U, T] or a
    sequence of sequences) with the ranks of that user's positives, -1 for a positive without a rank (excluded, or not a
    candidate) and for padding; n_positives_by_user [U]: how many positives the user has — a positive with rank -1 counts
    in the denominators and never as a hit, padding does not count.  Only users with at least one positive are counted.
    For every k in ks: hit_rate@k, recall@k, ndcg@k (binary relevance) with trainers.recommend.ranking_metrics' definitions;
    mrr: the mean over users of 1 / (1 + best rank), 0 for a user without a ranked positive; mean_rank: the mean 0-based
    rank over all ranked positives (0.0 when there is none); users: the number of users counted."""
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError("ranking_metrics_from_ranks: cutoffs %r (at least 1)" % (ks,))
    rows = [np.asarray(row, np.int64).reshape(-1) for row in ranks_by_user]
    n_pos = np.asarray(n_positives_by_user, np.int64).reshape(-1)
    if len(rows) != len(n_pos):
        raise ValueError("ranking_metrics_from_ranks: %d rows of ranks for %d users" % (len(rows), len(n_pos)))
    r = np.full((len(rows), max([len(row) for row in rows] + [1])), -1, np.int64)
    for u, row in enumerate(rows):
        r[u, :len(row)] = row
    r, n_pos = r[n_pos >= 1], n_pos[n_pos >= 1]              # only users with at least one positive are counted
    ranked = r >= 0
    if (ranked.sum(1) > n_pos).any():
        u = int(np.flatnonzero(ranked.sum(1) > n_pos)[0])
        raise ValueError("ranking_metrics_from_ranks: %d ranks for a user with %d positives" % (ranked[u].sum(), n_pos[u]))
    r = np.sort(np.where(ranked, r, np.iinfo(np.int64).max), 1)             # ascending, the positives without a rank last
    ranked = np.sort(~ranked, 1) == 0
    gain = np.where(ranked, 1.0 / np.log2(np.where(ranked, r, 0) + 2.0), 0.0)
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0
    out = {}
    for k in ks:
        top = ranked & (r < k)
        ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(min(k, int(n_pos.max()) if len(n_pos) else 0)) + 2.0))])
        out.update({"hit_rate@%d" % k: mean(top.any(1).astype(np.float64)), "recall@%d" % k: mean(top.sum(1) / n_pos),
                    "ndcg@%d" % k: mean(np.where(top, gain, 0.0).sum(1) / ideal[np.minimum(n_pos, k)])})
    best = np.where(ranked[:, 0], 1.0 / (1.0 + np.where(ranked[:, 0], r[:, 0], 0)), 0.0) if len(r) else np.zeros(0)
    out.update({"mrr": mean(best), "mean_rank": mean(r[ranked].astype(np.float64)), "users": int(len(r))})
    return out
