"""The case tables the EASE tests share (tests/test_ease_cpu.py, tests/test_gpu_ease.py) and the judgements both apply: the CPU test shows
that the float32 restatement of tests/ease_reference64.py passes them on every table and that every deliberate mistake of
ease_reference64.MUTATIONS fails them on some table; the GPU test applies the same judgements to the device's results, stage by stage,
each stage from the device's own output of the stage before.

Tables are knn_checks.table's: half-star values (0.5 .. 5.0), so every product and sum of the Gram matrix is exact in float32 and the
device's G must equal float64 bit for bit.  The inverse is judged by its distance from float64, which grows with the condition
number: l2 varies over the tables.
"""
import functools
from collections import namedtuple

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api

import ease_reference64 as ref
import knn_checks as kchk
import knn_reference64 as kref

L2S = (0.5, 20.0, 500.0)
KS = tuple(k for _, k in kchk.NK)  # 10, 256, 1, 256, 1, 10

# The float32 restatement's distance from float64, max |B - B64| / max |B64|, per table (measured by
# tests/test_ease_cpu.py::test_restatement_distance, which asserts every figure: at most this, at least half of it -- the recorded
# figure is the measured one plus a quarter, since the tile products are the host BLAS's, whose order of sums is the machine's).  The
# GPU test allows the device 4 x: a legitimate blocking may order the same sums differently.  Tables whose B is all zeros have
# distance 0 and admit only zeros.
EASE_DISTANCE = {
    "1-full": 0.0, "1-sparse": 0.0, "2-full": 1.26e-07, "2-sparse": 0.0,
    "63-full": 4.44e-07, "63-sparse": 7.04e-07, "64-full": 4.57e-06, "64-sparse": 4.98e-07,
    "65-full": 8.08e-07, "65-sparse": 4.48e-06, "129-full": 4.36e-06, "129-sparse": 1.05e-06,
    "323-full": 3.77e-05, "323-sparse": 2.97e-06, "2047-full": 3.65e-06, "2047-sparse": 3.82e-06,
    "2048-full": 2.74e-06, "2048-sparse": 8.56e-07, "2049-full": 2.88e-05, "2049-sparse": 9.28e-07,
    "4097-full": 5.84e-06, "4097-sparse": 4.5e-06,
}

# The ML_SMALL experiment (every user's last stored entry held out, k = 10, history = exclusion = the training rows, l2 = 500): the
# held-out hits of 610 users in float64, the restatement's distance at that order, and the users a float32 run may decide differently
# (within_reach()) -- tests/test_ease_cpu.py repeats the run and asserts the figures.
ML_SMALL_L2, ML_SMALL_K = 500.0, 10
ML_SMALL_EASE_HITS = 29
ML_SMALL_EASE_DISTANCE = 4.46e-06
ML_SMALL_EASE_WITHIN_REACH = 2

Case = namedtuple("Case", "name train history exclude l2 k users ids")


def block_items():
    return cu.lib().cu2rec_ease_block_items()  # a constant of the build: no device needed


def slice_items():
    return kchk.slice_items()


def workspace_batch(items, k):
    """Queries per workspace batch (include/cu2rec_amd.h: (slices + 1) * k * 8 bytes per query under CU2REC_EASE_WORKSPACE_BYTES)."""
    slices = max(1, -(-items // slice_items()))
    return max(1, api.EASE_WORKSPACE_BYTES // ((slices + 1) * k * 8))


def sizes():
    nb, s = block_items(), slice_items()
    return (1, 2, nb - 1, nb, nb + 1, 2 * nb + 1, 5 * nb + 3, s - 1, s, s + 1, 2 * s + 1)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: every catalogue of sizes() full (one user stores everything) and sparse (a third of the ids and the last eighth
    stored by nobody); and `batches`, 4 s + 1 items at k = 256, whose recommend call needs two workspace batches."""
    out = {}
    n = 0
    for cols in sizes():
        for full in (True, False):
            name = "%d-%s" % (cols, "full" if full else "sparse")
            t = kchk.table(name, cols, full, (KS[n % len(KS)],) * 2, 300 + n)
            out[name] = Case(name, t.train, t.history, t.exclude, L2S[n % len(L2S)], t.k, t.users, t.ids)
            n += 1
    s = slice_items()
    t = kchk.table("batches", 4 * s + 1, False, (256, 256), 299)
    users = (np.arange(workspace_batch(4 * s + 1, 256) + 500) % 8).astype(np.int32)
    out["batches"] = Case("batches", t.train, t.history, t.exclude, 20.0, 256, users, t.ids)
    return out


def inverse_tables():
    """The tables whose float64 inverse is taken: all but `batches`."""
    return [n for n in sorted(cases()) if n != "batches"]


# ---- float64 references, once per process and read-only ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram64(name):
    case = cases()[name]
    G = ref.gram(case.train, case.l2)
    G.setflags(write=False)
    return G


def weights64(G):
    return ref.weights(np.asarray(G, np.float64))


def unstored(csr):
    return np.bincount(csr.indices, minlength=csr.cols) == 0


def distance(B, B64):
    top = float(np.abs(B64).max(initial=0.0))
    if top == 0.0:
        return 0.0 if not np.asarray(B).any() else np.inf
    return float(np.abs(np.asarray(B, np.float64) - B64).max() / top)


# ---- judgements --------------------------------------------------------------------------------------------------------------
def judge_gram(name, G):
    """(a): G equals float64 exactly -- bits, the diagonal with l2, the rows of unstored items."""
    return [] if np.array_equal(np.asarray(G, np.float64), gram64(name)) else ["G differs from float64"]


def judge_weights(name, G, B, margin=4.0):
    """(b): B within margin x EASE_DISTANCE[name] of the float64 B from G, finite, an exactly zero diagonal, exactly zero rows and
    columns of unstored items."""
    case = cases()[name]
    B = np.asarray(B)
    out = []
    if B.shape != (case.train.cols,) * 2 or not np.isfinite(B).all():
        return ["B has the wrong shape or is not finite"]
    if (np.diag(B) != 0).any():
        out.append("the diagonal of B is not zero")
    none = unstored(case.train)
    if (B[none] != 0).any() or (B[:, none] != 0).any():
        out.append("an unstored item has a nonzero row or column")
    dist = distance(B, weights64(G))
    if not dist <= margin * EASE_DISTANCE[name]:
        out.append("B is %.3g from float64, more than %g x %.3g" % (dist, margin, EASE_DISTANCE[name]))
    return out


def judge_recommend(B, history, exclude, users, ids, vals, k):
    """(c) for recommend: knn_reference64.judge_lists against float64 scores from the given B; the bound is the fold's."""
    B = np.asarray(B, np.float64)
    order, _ = kref.sorted_rows(history)
    cols = B.shape[0]
    out, seen = [], {}
    for p, u in enumerate(users):
        u = int(u)
        if u not in seen:
            items, r = kref.history_row(history, order, u)
            score, terms, sabs = ref.row_scores(B, items, r)
            seen[u] = (score, ~kref.excluded_mask(exclude, u, cols), terms, sabs)
        out += ["row %d: %s" % (u, c) for c in kref.judge_lists(ids[p], vals[p], *seen[u], k)]
    return out


def judge_neighbours(B, rows, ids, vals, k):
    """(c) for neighbors: the list of the one-entry history {i: 1.0} with i excluded."""
    B = np.asarray(B, np.float64)
    out = []
    for p, i in enumerate(rows):
        eligible = np.ones(B.shape[0], bool)
        eligible[i] = False
        out += ["item %d: %s" % (i, c) for c in kref.judge_lists(ids[p], vals[p], B[i], eligible, np.ones(B.shape[0]), np.abs(B[i]), k)]
    return out


# ---- the ML_SMALL experiment -----------------------------------------------------------------------------------------------------
def ml_small():
    return kchk.ml_small()


@functools.lru_cache(maxsize=None)
def ml_small_run():
    """The float64 experiment -> (hits, B64, recommended ids, vals)."""
    train, held = ml_small()
    B = ref.weights(ref.gram(train, ML_SMALL_L2))
    ids, vals = ref.recommend(B, train, train, None, ML_SMALL_K)
    return kref.hits_at(ids, held), B, ids, vals


def within_reach(dist):
    """The users of the ML_SMALL experiment whose hit a float32 run may decide differently from float64: the held-out item's score and
    the k-th best other candidate's differ by a nonzero amount inside both scores' errors.  A score's error is the fold's bound plus the
    inverse's: every B_ij up to 4 x dist x max |B| away (the margin the device is held to), times the row's sum of |r|."""
    train, held = ml_small()
    _, B, _, _ = ml_small_run()
    order, _ = kref.sorted_rows(train)
    top = float(np.abs(B).max())
    reach = 0
    for u in range(train.rows):
        items, r = kref.history_row(train, order, u)
        score, terms, sabs = ref.row_scores(B, items, r)
        err = kref.fold_bound(terms, sabs) + 4 * dist * top * np.abs(r).sum()
        target = int(held.indices[held.indptr[u]])
        others = np.ones(train.cols, bool)
        others[items] = False
        others[target] = False
        others = np.flatnonzero(others)
        kth = others[np.lexsort((others, -score[others]))[ML_SMALL_K - 1]]
        gap = abs(score[target] - score[kth])
        reach += 0 < gap <= err[target] + err[kth]
    return int(reach)
