"""The case tables the ItemKNN tests share (tests/test_knn_cpu.py, tests/test_gpu_knn.py) and the judgements both apply: the CPU test
shows that a float32 restatement in the kernels' order passes them on every table and that every deliberate mistake of
knn_reference64.MUTATIONS fails them on some table; the GPU test applies the same judgements to the device's results.

Tables hold half-star values (0.5 .. 5.0), so under the `count` weighting every product and sum is exact in float32 and the device
must equal the float64 reference bit for bit; the float weightings are judged stage by stage with the fold's bound.
"""
import functools
from collections import namedtuple

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api

import knn_reference64 as ref

# The float32 restatement's worst relative distance from the float64 weights over every table and weighting (measured by
# tests/test_knn_cpu.py::test_weights_restatement_distance, which asserts it): the device evaluates the same formulas in double and
# rounds once, so this is float32's rounding.  The GPU test allows 4 x: the device's log / sqrt against numpy's.
WEIGHT_DISTANCE = 5.96e-8
FLOAT_WEIGHTINGS = ("cosine", "tfidf", "bm25")
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 300)
NK = ((10, 10), (1, 256), (256, 1), (256, 256), (10, 1), (1, 10))  # (neighbours, k) of successive tables: each of 1, 10, 256 both ways

# The ML_SMALL experiment (every user's last stored entry held out, N = 20, k = 10, history = exclusion = the training rows): the
# held-out hits of 610 users in float64, per weighting and for the popularity baseline -- tests/test_knn_cpu.py repeats the run and
# asserts every figure -- and for cosine the users a float32 run may decide differently (see within_reach()).
ML_SMALL_N, ML_SMALL_K = 20, 10
ML_SMALL_HITS = {"popularity": 8, "count": 12, "cosine": 26, "tfidf": 21, "bm25": 8}
ML_SMALL_COSINE_WITHIN_REACH = 0

Case = namedtuple("Case", "name train history exclude neighbours k users ids")


def slice_items():
    return cu.lib().cu2rec_knn_slice_items()  # a constant of the build: no device needed


def workspace_batch(items, k):
    """Queries per workspace batch (include/cu2rec_amd.h: (slices + 1) * k * 8 bytes per query under CU2REC_KNN_WORKSPACE_BYTES)."""
    slices = max(1, -(-items // slice_items()))
    return max(1, api.KNN_WORKSPACE_BYTES // ((slices + 1) * k * 8))


def half_star_csr(rows_items, cols, rng):
    """A CSR whose row u stores the columns rows_items[u] in a shuffled order with half-star values."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_items])])
    indices = np.concatenate([rng.permutation(np.asarray(r, np.int64)) for r in rows_items] + [np.zeros(0, np.int64)])
    data = rng.integers(1, 11, len(indices)) / 2.0
    return api.HostCSR(indptr, indices, data, len(rows_items), cols, 0.0)


def table(name, cols, full, nk, seed, n_users_listed=8):
    """One table: a catalogue of `cols` items.  full: one user stores everything (every pair touched); otherwise a third of the ids and
    the last eighth are stored by nobody and few pairs are touched (lists shorter than N: padding).  Rows of ROW_LENGTHS entries
    (clipped to what can be stored), unsorted; the history is another such set, the exclusion has repeats and fewer rows."""
    rng = np.random.default_rng(seed)
    stored = np.arange(cols) if full else np.array([i for i in range(cols) if i % 3 != 1 and i < cols - cols // 8] or [0])

    def rows(lengths):
        return [rng.choice(stored, min(n, len(stored)), replace=False) for n in lengths]

    train = half_star_csr(rows(ROW_LENGTHS + ((cols,) if full else ()) + (5, 7, 3, 2, 2)), cols, rng)
    history = half_star_csr(rows(ROW_LENGTHS + (4,)), cols, rng)
    ex_rows = [rng.choice(cols, min(n, cols), replace=True) for n in (3, 0, 70, 1, 130)]  # repeats; rows 5 .. exclude nothing
    exclude = api.HostCSR(np.concatenate([[0], np.cumsum([len(r) for r in ex_rows])]), np.concatenate(ex_rows), np.ones(sum(map(len, ex_rows))),
                          len(ex_rows), cols, 0.0)
    users = np.array([3, 0, 3, 6, 1, 2, 4, 5, 7, 6][:n_users_listed + 2], np.int32)
    ids = np.array([cols - 1, 0, cols - 1, cols // 2], np.int32)
    return Case(name, train, history, exclude, nk[0], nk[1], users, ids)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: catalogues of 1, 2, 63, 64, 65 items and s - 1, s, s + 1, 2 s + 1 for the slice width s, both kinds at 65 and
    s + 1; and `batches`, whose build and whose recommend call each need two workspace batches."""
    s = slice_items()
    out = {}
    sizes = [(1, True), (2, True), (63, False), (64, True), (65, False), (65, True), (s - 1, False), (s, True), (s + 1, False),
             (s + 1, True), (2 * s + 1, False)]
    for n, (cols, full) in enumerate(sizes):
        name = "%d-%s" % (cols, "full" if full else "sparse")
        out[name] = table(name, cols, full, NK[n % len(NK)], 100 + n)
    big = table("batches", 4 * s + 1, False, (256, 256), 99)
    out["batches"] = big._replace(users=(np.arange(workspace_batch(4 * s + 1, 256) + 500) % 8).astype(np.int32))
    return out


def duplicate_csr():
    """A CSR whose second row stores column 4 twice (not side by side until sorted)."""
    return api.HostCSR([0, 2, 6, 7], [1, 0, 4, 2, 0, 4, 3], [1.0, 2.0, 3.0, 4.0, 5.0, 1.5, 2.5], 3, 6, 0.0)


# ---- judgements --------------------------------------------------------------------------------------------------------------
def weight_ratio(csr, weighting, got):
    """The worst distance of `got` from the float64 weights in units of 4 x WEIGHT_DISTANCE x |weight|; a weight that must be 0 admits
    only 0."""
    want = ref.weights(csr, weighting)
    got = np.asarray(got, np.float64)
    if not len(want):
        return 0.0
    if (got[want == 0] != 0).any() or not np.isfinite(got).all():
        return np.inf
    nz = want != 0
    return float((np.abs(got[nz] - want[nz]) / (4 * WEIGHT_DISTANCE * np.abs(want[nz]))).max()) if nz.any() else 0.0


def judge_neighbours(csr, w, ids, vals, n, rows=None, block=1024):
    """Checks (a) - (d) of the lists of items `rows` (None: all, ids / vals row r = item r) against float64 from the entry weights w."""
    W, B = ref.dense(csr, w)
    out = []
    rows = np.arange(csr.cols) if rows is None else np.asarray(rows)
    for lo in range(0, csr.cols, block):
        hi = min(lo + block, csr.cols)
        mine = np.flatnonzero((rows >= lo) & (rows < hi))
        if not len(mine):
            continue
        S, touched, terms, sabs = ref.similarity_block(W, B, lo, hi)
        for p in mine:
            i = rows[p] - lo
            out += ["item %d: %s" % (rows[p], c) for c in ref.judge_lists(ids[p], vals[p], S[i], touched[i], terms[i], sabs[i], n)]
    return out


def judge_recommend(list_ids, list_vals, history, exclude, users, ids, vals, k):
    """Checks (a) - (d) of the recommendations of rows `users` against float64 from the given (truncated) lists."""
    order, _ = ref.sorted_rows(history)
    cols = list_ids.shape[0]
    out, seen = [], {}
    for p, u in enumerate(users):
        if u not in seen:
            items, r = ref.history_row(history, order, u)
            score, touched, terms, sabs = ref.recommend_scores(list_ids, np.asarray(list_vals, np.float64), items, r, cols)
            seen[u] = (score, touched & ~ref.excluded_mask(exclude, u, cols), terms, sabs)
        out += ["row %d: %s" % (u, c) for c in ref.judge_lists(ids[p], vals[p], *seen[u], k)]
    return out


@functools.lru_cache(maxsize=None)
def exact(name):
    """The float64 reference of a table under `count` -> (neighbour ids, vals, recommend ids, vals for case.users): what the device
    must equal exactly."""
    case = cases()[name]
    n_ids, n_vals = ref.neighbours(case.train, ref.weights(case.train, "count"), case.neighbours)
    distinct = sorted(set(case.users.tolist()))
    r_ids, r_vals = ref.recommend(n_ids, n_vals, case.history, case.exclude, distinct, case.k)
    at = np.searchsorted(distinct, case.users)
    for a in (n_ids, n_vals, r_ids, r_vals):
        a.setflags(write=False)
    return n_ids, n_vals, r_ids[at], r_vals[at]


def same_lists(ids, vals, want_ids, want_vals):
    """ids, values (as float32) and padding all equal."""
    return np.array_equal(ids, want_ids) and np.array_equal(np.asarray(vals, np.float32), np.asarray(want_vals, np.float32), equal_nan=True)


# ---- the ML_SMALL experiment -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ml_small():
    """(train, held): the bundled ML_SMALL with every user's last stored entry held out."""
    from bpr_checks import hold_out_last
    from conftest import ml_small as path
    return hold_out_last(cu.createSparseMatrix(path()))


@functools.lru_cache(maxsize=None)
def ml_small_run(weighting):
    """The float64 experiment -> (hits, list ids, list vals, recommended ids, vals)."""
    train, held = ml_small()
    n_ids, n_vals = ref.neighbours(train, ref.weights(train, weighting), ML_SMALL_N)
    r_ids, r_vals = ref.recommend(n_ids, n_vals, train, train, None, ML_SMALL_K)
    return ref.hits_at(r_ids, held), n_ids, n_vals, r_ids, r_vals


def within_reach(weighting):
    """The users of the ML_SMALL experiment whose hit a float32 run may decide differently from float64.  A list can differ where a
    listed and an unlisted neighbour of an item differ by a nonzero amount inside both values' float32 bounds (an exact tie is decided
    by id both ways: equal weights give equal folds); such an entry may enter or leave a score whole, so its |r s| counts as that
    candidate's error, beside the fold's bound and the lists' own error pushed through.  A user is within reach when the held-out
    item's score and the k-th best other candidate's differ by a nonzero amount inside both errors.  The lists' bounds are the fold's
    plus the weights' rounding (2 x 2^-24 per product)."""
    train, held = ml_small()
    _, n_ids, n_vals, _, _ = ml_small_run(weighting)
    W, B = ref.dense(train, ref.weights(train, weighting))
    list_err = np.zeros((train.cols, ML_SMALL_N))
    flips = {}  # item -> (candidates that may enter or leave its list, |s| of each)
    for lo in range(0, train.cols, 1024):
        hi = min(lo + 1024, train.cols)
        S, touched, terms, sabs = ref.similarity_block(W, B, lo, hi)
        bound = ref.fold_bound(terms, sabs) + 2 * ref.U * sabs
        for i in range(hi - lo):
            idx = np.flatnonzero(touched[i])
            listed = n_ids[lo + i][n_ids[lo + i] >= 0]
            list_err[lo + i, :len(listed)] = bound[i, listed]
            if len(idx) <= ML_SMALL_N:
                continue
            rest = np.setdiff1d(idx, listed)
            rest = rest[S[i, listed[-1]] - S[i, rest] <= 2 * bound[i, idx].max()]  # the others are out of every listed value's reach
            gap = S[i, listed][:, None] - S[i, rest][None, :]
            near = (gap > 0) & (gap <= bound[i, listed][:, None] + bound[i, rest][None, :])
            if near.any():
                moving = np.concatenate([listed[near.any(axis=1)], rest[near.any(axis=0)]])
                flips[lo + i] = (moving, np.abs(S[i, moving]))
    order, _ = ref.sorted_rows(train)
    reach = 0
    for u in range(train.rows):
        items, r = ref.history_row(train, order, u)
        score, touched, terms, sabs = ref.recommend_scores(n_ids, n_vals, items, r, train.cols)
        err = ref.recommend_scores(n_ids, list_err, items, r, train.cols)[3] + ref.fold_bound(terms, sabs)
        for i, ri in zip(items, r):
            if i in flips:
                np.add.at(err, flips[i][0], abs(ri) * flips[i][1])
                touched[flips[i][0]] = True
        touched &= ~ref.excluded_mask(train, u, train.cols)
        target = int(held.indices[held.indptr[u]])
        if not touched[target]:
            continue
        others = np.flatnonzero(touched)
        others = others[others != target]
        if len(others) < ML_SMALL_K:
            continue
        kth = others[np.lexsort((others, -score[others]))[ML_SMALL_K - 1]]
        gap = abs(score[target] - score[kth])
        reach += 0 < gap <= err[target] + err[kth]
    return int(reach)
