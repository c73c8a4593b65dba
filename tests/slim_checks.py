"""The case tables the SLIM tests share (tests/test_slim_cpu.py, tests/test_gpu_slim.py) and the judgements both apply: the CPU test
shows that the float32 restatement of tests/slim_reference64.py in the device's order passes them on every table and that every
deliberate mistake of slim_reference64.MUTATIONS fails them on some table; the GPU test applies the same judgements to the device's W.

Tables are knn_checks.table's at 1, 2, nb - 1, nb, nb + 1, 2 nb + 1, 5 nb + 3 and 32 nb + 1 items for the block order nb = 64 (one
tile, the edges of a tile, several tiles with a ragged last one, a 33 x 33 tile grid), each full and sparse.  Larger orders add
nothing to the solver, and the slices of the serving path are EASE's and tested there.  l2 cycles over ease_checks.L2S, l1 over L1S,
`positive` takes both values on full and on sparse tables.  Comparisons are at equal sweep counts, never converged against converged:
at l2 = 0.5 the iteration needs hundreds of sweeps.
"""
import functools
from collections import namedtuple

import numpy as np

import ease_checks as echk
import ease_reference64 as eref
import knn_checks as kchk
import knn_reference64 as kref
import slim_reference64 as ref

L1S = (1.0, 3.0, 6.0, 12.0)
SWEEPS = 3  # the count SLIM_DISTANCE is taken at
COUNTS = (1, 2, 3)

# The float32 restatement's distance from float64 after SWEEPS sweeps, max |W - W64| / max |W64|, per table (measured by
# tests/test_slim_cpu.py::test_restatement_distance, which asserts every figure: at most this, at least half of it -- the recorded
# figure is the measured one plus a quarter, since the block products are the host BLAS's, whose order of sums is the machine's).  The
# GPU test allows the device 4 x: a legitimate tile product may order the same sums differently.  Tables whose W is all zeros have
# distance 0 and admit only zeros.
SLIM_DISTANCE = {
    "1-full": 0.0, "1-sparse": 0.0, "2-full": 3.7e-08, "2-sparse": 0.0,
    "63-full": 9.85e-07, "63-sparse": 1.47e-06, "64-full": 4.19e-07, "64-sparse": 5.25e-07,
    "65-full": 1.81e-06, "65-sparse": 7.82e-07, "129-full": 1.65e-06, "129-sparse": 1.52e-06,
    "323-full": 5.87e-07, "323-sparse": 7.83e-07, "2049-full": 1.41e-06, "2049-sparse": 6.1e-07,
}

# The EASE limit (l1 = 0, free signs, the l2 = 500 tables): the sweeps float64 coordinate descent needs to come within EASE_LIMIT_TOL x
# max |B| of ease_reference64.weights, at most EASE_LIMIT_CAP -- the tables are those for which it does, which test_slim_cpu asserts --
# and the distance between the two float32 restatements (SLIM's after that many sweeps, EASE's), over max |B64|: recorded as measured
# plus a quarter and asserted like SLIM_DISTANCE; the device's W and B are allowed 4 x.
EASE_LIMIT_TOL, EASE_LIMIT_CAP = 1e-6, 50
EASE_LIMIT = {  # name -> (sweeps, distance of the restatements)
    "2-full": (1, 1.29e-07), "63-sparse": (16, 2.76e-06), "65-full": (35, 3.2e-06), "129-sparse": (27, 1.72e-06),
}

# Early stop and optimality: tables run to a tol stop, with the tol and the sweep at which the float64 sequence of largest |delta|
# stops.  The sequence must stay a factor of 4 away from tol on both sides of that sweep (asserted by the CPU test), which takes a
# sixteen-fold drop across one sweep: at the tables' own l2 the sequences fall by 2 to 6 a sweep, so these runs have an l1 and an l2 of
# their own (a large l2 makes A diagonally dominant and the descent fast).  Every stopping |delta| is 100 x above float32's resolution
# of the weights (max |W| about l2^-1 x 60).
STOPS = {  # name -> (l1, l2, positive, tol, stopping sweep)
    "65-sparse": (1.0, 5000.0, False, 1.1e-06, 5),
    "129-full": (6.0, 5000.0, True, 1.4e-04, 4),
    "323-full": (1.0, 50000.0, True, 8e-07, 4),
}
STOP_CAP = 12  # max_sweeps of these runs

# The ML_SMALL experiment (every user's last stored entry held out, k = 10, history = exclusion = the training rows; l1 = 5, l2 = 500,
# non-negative weights, ML_SMALL_SWEEPS sweeps): the held-out hits of 610 users in float64 -- tests/test_slim_cpu.py repeats the run and
# asserts the figures -- the nonzero fraction of W, and the users a float32 run may decide differently (within_reach()).  The
# restatement at 9,724 items takes minutes, so its distance at that order is not measured: within_reach is given the largest recorded
# distance of the tables, ml_distance().
ML_SMALL_L1, ML_SMALL_L2, ML_SMALL_K, ML_SMALL_SWEEPS = 5.0, 500.0, 10, 3
ML_SMALL_SLIM_HITS = 37
ML_SMALL_SLIM_NONZERO = 0.0239  # of 9,724^2 weights, to four decimals
ML_SMALL_SLIM_WITHIN_REACH = 0

Case = namedtuple("Case", "name train history exclude l1 l2 positive k users ids")


def block_items():
    return echk.block_items()


def sizes():
    nb = block_items()
    return (1, 2, nb - 1, nb, nb + 1, 2 * nb + 1, 5 * nb + 3, 32 * nb + 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    n = 0
    for cols in sizes():
        for full in (True, False):
            name = "%d-%s" % (cols, "full" if full else "sparse")
            t = kchk.table(name, cols, full, (echk.KS[n % len(echk.KS)],) * 2, 300 + n)
            out[name] = Case(name, t.train, t.history, t.exclude, L1S[(n // 2) % len(L1S)], echk.L2S[n % len(echk.L2S)], n % 4 in (0, 3), t.k,
                             t.users, t.ids)
            n += 1
    return out


def ml_distance():
    return max(SLIM_DISTANCE.values())


# ---- float64 references, once per process and read-only ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram64(name):
    case = cases()[name]
    A = eref.gram(case.train, case.l2)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def weights64(name, sweeps):
    """W in float64 after `sweeps` sweeps (through R = X W: test_slim_cpu shows it equal to the plain form)."""
    case = cases()[name]
    W, _, _ = ref.sweeps64_rows(case.train, np.diag(gram64(name)), case.l1, case.positive, sweeps)
    W.setflags(write=False)
    return W


def unstored(csr):
    return echk.unstored(csr)


distance = echk.distance


# ---- judgements --------------------------------------------------------------------------------------------------------------
def judge_weights(name, W, sweeps, margin=4.0):
    """W within margin x SLIM_DISTANCE[name] of float64 after the same number of sweeps, finite, an exactly zero diagonal, exactly zero
    rows and columns of unstored items, and no negative weight under `positive`."""
    case = cases()[name]
    W = np.asarray(W)
    out = []
    if W.shape != (case.train.cols,) * 2 or not np.isfinite(W).all():
        return ["W has the wrong shape or is not finite"]
    if (np.diag(W) != 0).any():
        out.append("the diagonal of W is not zero")
    none = unstored(case.train)
    if (W[none] != 0).any() or (W[:, none] != 0).any():
        out.append("an unstored item has a nonzero row or column")
    if case.positive and (W < 0).any():
        out.append("a negative weight under `positive`")
    dist = distance(W, weights64(name, sweeps))
    if not dist <= margin * SLIM_DISTANCE[name]:
        out.append("W is %.3g from float64 after %d sweeps, more than %g x %.3g" % (dist, sweeps, margin, SLIM_DISTANCE[name]))
    return out


def some_but_not_all_zero(name):
    """Of the weights between two different stored items after SWEEPS float64 sweeps, some are zero and some are not (None for a table
    with fewer than 3 stored items: with two, both weights have the same rho over different diagonals, zero together or not at all)."""
    case = cases()[name]
    have = np.flatnonzero(~unstored(case.train))
    if len(have) < 3:
        return None
    W = weights64(name, SWEEPS)[np.ix_(have, have)]
    off = W[~np.eye(len(have), dtype=bool)]
    return bool((off == 0).any() and (off != 0).any())


# ---- the ML_SMALL experiment -----------------------------------------------------------------------------------------------------
def ml_small():
    return kchk.ml_small()


@functools.lru_cache(maxsize=None)
def ml_small_run():
    """The float64 experiment -> (hits, W64, recommended ids, vals)."""
    train, held = ml_small()
    diag = np.diag(eref.gram(train, ML_SMALL_L2)).copy()
    W, _, _ = ref.sweeps64_rows(train, diag, ML_SMALL_L1, True, ML_SMALL_SWEEPS)
    ids, vals = eref.recommend(W, train, train, None, ML_SMALL_K)
    return kref.hits_at(ids, held), W, ids, vals


def within_reach(dist):
    """ease_checks.within_reach for SLIM's W: the users whose hit a float32 run may decide differently from float64 -- the held-out
    item's score and the k-th best other candidate's differ by a nonzero amount inside both scores' errors, the fold's bound plus every
    W_ij up to 4 x dist x max |W| away, times the row's sum of |r|."""
    train, held = ml_small()
    _, W, _, _ = ml_small_run()
    order, _ = kref.sorted_rows(train)
    top = float(np.abs(W).max())
    reach = 0
    for u in range(train.rows):
        items, r = kref.history_row(train, order, u)
        score, terms, sabs = eref.row_scores(W, items, r)
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
