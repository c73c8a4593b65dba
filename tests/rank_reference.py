"""Float64 restatement of the ranking metrics of cu2rec_model_rank_metrics (include/cu2rec_amd.h), given top-k lists.

For each model row u:
  R_u = distinct items of test row u rated >= threshold (threshold None or -inf: every rating).  Items past the catalogue
        count in |R_u|; they never appear in a list, so they are never hit.
  users with |R_u| = 0 are skipped (NaN per-user values) and counted;
  L_u = the list without its -1 padding; hits = |L_u n R_u|;
  precision = hits / k, recall = hits / |R_u|, hit = [hits > 0],
  ndcg = DCG / IDCG with binary gains (DCG over hit positions j of 1 / log2(j + 2), IDCG over j < min(k, |R_u|)),
  ap = (1 / min(k, |R_u|)) * sum over hit positions j of (hits in L_u[0..j]) / (j + 1).
Means are over evaluated users.
"""
import math

import numpy as np

FIELDS = ("precision", "recall", "ndcg", "ap", "hit")


def relevant(indptr, indices, data, u, threshold=None):
    """R_u of test row u (a Python set)."""
    lo, hi = int(indptr[u]), int(indptr[u + 1])
    everything = threshold is None or threshold == -math.inf
    return {int(i) for i, r in zip(indices[lo:hi], data[lo:hi]) if everything or float(r) >= threshold}


def user_metrics(lst, rel, k):
    """(precision, recall, ndcg, ap, hit) of one list against a non-empty relevant set."""
    hits, dcg, ap = 0, 0.0, 0.0
    for j, item in enumerate(int(x) for x in lst):
        if item < 0:
            break
        if item in rel:
            hits += 1
            dcg += 1.0 / math.log2(j + 2)
            ap += hits / (j + 1)
    m = min(k, len(rel))
    idcg = sum(1.0 / math.log2(j + 2) for j in range(m))
    return hits / k, hits / len(rel), dcg / idcg, ap / m, 1.0 if hits > 0 else 0.0


def rank_metrics(lists, test, k, threshold=None, rows=None):
    """lists: (rows, k) item ids, -1 padding; test: anything with indptr / indices / data / rows (HostCSR).  rows: the model's
    row count (default: len(lists)); test rows past it are an error.  -> (dict of means and counts, (rows, 5) per-user)."""
    rows = len(lists) if rows is None else rows
    if test.rows > rows:
        raise ValueError("test rows past the model's rows")
    per = np.full((rows, 5), np.nan)
    for u in range(min(rows, test.rows)):
        rel = relevant(test.indptr, test.indices, test.data, u, threshold)
        if rel:
            per[u] = user_metrics(lists[u], rel, k)
    ok = ~np.isnan(per[:, 0])
    n = int(ok.sum())
    means = per[ok].sum(axis=0) / n if n else np.full(5, np.nan)
    out = {"precision": means[0], "recall": means[1], "ndcg": means[2], "map": means[3], "hit_rate": means[4],
           "users_evaluated": n, "users_skipped": rows - n, "k": k}
    return out, per
