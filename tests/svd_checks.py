"""The tables the PureSVD tests share (tests/test_svd_cpu.py, tests/test_gpu_svd.py), the judgements both apply and the recorded
distances of the float32 restatement of tests/svd_reference64.py from float64.  The CPU test shows that the restatement passes every
judgement on every table, pins the recorded figures and shows that each judge catches a planted error; the GPU test applies the same
judgements to the device's results, stage by stage, each stage from the device's own output of the stage before.

The device is allowed MARGIN x a recorded figure: it adds the same numbers in another order (groups of four entries, chunks, tiles of
1,024 rows, matrix-core chains).  The product alone is judged by a derived, order-free bound.
"""
import functools
from collections import namedtuple

import numpy as np

from cu2rec_amd import api

import svd_reference64 as ref

MARGIN = 4.0
U = 2.0 ** -24
FS = (1, 3, 4, 5, 63, 64, 65, 128, 129, 252)  # the float4 tails and every E = 1 .. 4 of the product
ROW_LENGTHS = (0, 1, 3, 4, 5, 1024, 1025, 2049)
LONGEST = 64 * 1024 + 1  # past where the row plan's chunks grow (CU2REC_ALS_MAX_CHUNKS chunks of CU2REC_ALS_CHUNK)

ORTH_FS = (1, 2, 31, 32, 33, 64, 65, 252)
ORTH_KINDS = ("gauss", "scaled")

Table = namedtuple("Table", "name csr f sweeps")

# The float32 restatement's figures per table (tests/test_svd_cpu.py::test_restatement_distance asserts each: at most the figure, at
# least half of it): the score distance max |S32 - S64| / max |S64| from the same start, |Q^T Q - I|max, and the relative distance of
# `captured`.  No figure is recorded below FLOOR = 2^-23, one unit in the last place of a float32 near 1: the entries of Q and P are
# stored rounded, so a restatement that happens to land nearer than that (at f = 1 it often does, exactly) sets no standard.
FLOOR = 2.0 ** -23
SVD_DISTANCE = {
    "70x90-f5": (2.55e-07, 2.83e-07, 1.2e-07),
    "300x200-f33": (2.57e-07, 6.06e-07, 1.2e-07),
    "long-f64": (5.23e-06, 1.09e-06, 1.79e-07),
    "300x400-f252": (6.98e-07, 7.79e-07, 1.96e-07),
}

# The restatement's (|Q^T Q - I|max, span error) of orth on orth_input(n, f, kind), keyed "n-f-kind"
# (tests/test_svd_cpu.py::test_orth_restatement_figures asserts each the same way; FLOOR as above).
ORTH_DISTANCE = {
    "1-1-gauss": (1.2e-07, 1.2e-07), "1-1-scaled": (1.2e-07, 1.2e-07), "2-1-gauss": (1.2e-07, 1.2e-07),
    "2-1-scaled": (1.2e-07, 1.2e-07), "31-1-gauss": (1.2e-07, 1.2e-07), "31-1-scaled": (1.2e-07, 1.2e-07),
    "32-1-gauss": (1.2e-07, 1.2e-07), "32-1-scaled": (1.2e-07, 1.2e-07), "33-1-gauss": (1.23e-07, 1.3e-07),
    "33-1-scaled": (1.23e-07, 1.3e-07), "1025-1-gauss": (2.89e-07, 3.38e-07), "1025-1-scaled": (2.89e-07, 3.38e-07),
    "2-2-gauss": (1.2e-07, 1.2e-07), "2-2-scaled": (1.2e-07, 1.2e-07), "3-2-gauss": (1.29e-07, 1.2e-07),
    "3-2-scaled": (1.24e-07, 1.2e-07), "31-2-gauss": (2.15e-07, 2.04e-07), "31-2-scaled": (2.12e-07, 2.23e-07),
    "32-2-gauss": (1.2e-07, 1.2e-07), "32-2-scaled": (1.2e-07, 1.2e-07), "33-2-gauss": (1.39e-07, 1.6e-07),
    "33-2-scaled": (1.43e-07, 1.43e-07), "1025-2-gauss": (3.07e-07, 2.55e-07), "1025-2-scaled": (4.32e-07, 4.49e-07),
    "31-31-gauss": (3.4e-07, 2.35e-07), "31-31-scaled": (3.26e-07, 1.95e-07), "32-31-gauss": (2.19e-07, 1.6e-07),
    "32-31-scaled": (3.07e-07, 2.68e-07), "33-31-gauss": (2.14e-07, 1.53e-07), "33-31-scaled": (3.45e-07, 1.85e-07),
    "1025-31-gauss": (1.04e-06, 8.25e-07), "1025-31-scaled": (8.35e-07, 7.83e-07), "32-32-gauss": (2.89e-07, 1.95e-07),
    "32-32-scaled": (2.36e-07, 1.3e-07), "33-32-gauss": (2.23e-07, 1.56e-07), "33-32-scaled": (2.77e-07, 1.2e-07),
    "1025-32-gauss": (1.11e-06, 9.14e-07), "1025-32-scaled": (1.07e-06, 2.17e-07), "33-33-gauss": (3.98e-07, 2.14e-07),
    "33-33-scaled": (4.53e-07, 1.41e-07), "34-33-gauss": (3.94e-07, 2.3e-07), "34-33-scaled": (2.99e-07, 2.64e-07),
    "1025-33-gauss": (9.81e-07, 7.58e-07), "1025-33-scaled": (9.19e-07, 4.26e-07), "64-64-gauss": (3.49e-07, 1.95e-07),
    "64-64-scaled": (4.07e-07, 2.41e-07), "65-64-gauss": (3.93e-07, 2.84e-07), "65-64-scaled": (3.84e-07, 2.05e-07),
    "1025-64-gauss": (1.17e-06, 9.79e-07), "1025-64-scaled": (1.02e-06, 3.82e-07), "65-65-gauss": (3.51e-07, 2.39e-07),
    "65-65-scaled": (3.85e-07, 1.58e-07), "66-65-gauss": (5.81e-07, 2.41e-07), "66-65-scaled": (4.07e-07, 1.79e-07),
    "1025-65-gauss": (1.23e-06, 1.04e-06), "1025-65-scaled": (1.17e-06, 3.8e-07), "252-252-gauss": (1.67e-06, 5.42e-07),
    "252-252-scaled": (1.21e-06, 3.23e-07), "253-252-gauss": (8.26e-07, 3.75e-07), "253-252-scaled": (5.95e-07, 3.01e-07),
    "1025-252-gauss": (1.38e-06, 9.58e-07), "1025-252-scaled": (1.19e-06, 1.07e-06),
}

# The ML_SMALL experiment (every user's last stored entry held out, the library's seed-42 start, k = 10, the training rows excluded):
# the held-out hits of 610 users in float64, the restatement's score distance, and the users a float32 run may decide differently.
ML_SMALL_F, ML_SMALL_SWEEPS, ML_SMALL_K = 252, 8, 10
ML_SMALL_SVD_HITS = 35
ML_SMALL_SVD_DISTANCE = 2.54e-05
ML_SMALL_SVD_WITHIN_REACH = 0


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def half_stars(rng, n):
    return rng.randint(1, 11, size=n).astype(np.float32) * np.float32(0.5)


def csr_of(rows_items, cols, rng):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_items])])
    indices = np.concatenate([np.asarray(r, np.int64) for r in rows_items] + [np.zeros(0, np.int64)])
    return api.HostCSR(indptr, indices, half_stars(rng, len(indices)), len(rows_items), cols)


def random_csr(rows, cols, per_row, seed, long_row=0, long_col=0):
    """Every row stores per_row distinct random columns; row 0 stores long_row of them and column 0 is stored by long_col rows."""
    rng = np.random.RandomState(seed)
    out = []
    for u in range(rows):
        n = long_row if (u == 0 and long_row) else per_row
        items = rng.permutation(cols)[:n]
        if long_col and 0 < u <= long_col and 0 not in items:
            items[0] = 0
        out.append(items)
    return csr_of(out, cols, rng)


@functools.lru_cache(maxsize=None)
def tables():
    """name -> Table: the end-to-end tables."""
    t = [Table("70x90-f5", random_csr(70, 90, 12, 11), 5, 3),
         Table("300x200-f33", random_csr(300, 200, 25, 12), 33, 3),
         Table("long-f64", random_csr(1100, 1100, 9, 13, long_row=1030, long_col=1040), 64, 2),
         Table("300x400-f252", random_csr(300, 400, 160, 14), 252, 2)]
    return {x.name: x for x in t}


@functools.lru_cache(maxsize=None)
def product_csrs():
    """name -> HostCSR for the product's tests: `lengths` has a row of every length of ROW_LENGTHS and one that stores a column
    twice; `lengths_t` is its transpose, so that the item-major side meets the same lengths; `longest` is LONGEST x 3 with a column
    every row stores, an empty column and a short one."""
    rng = np.random.RandomState(21)
    cols = 2100
    rows = [rng.permutation(cols)[:n] for n in ROW_LENGTHS]
    rows.append(np.array([5, 7, 5, 2099]))  # column 5 twice
    lengths = csr_of(rows, cols, rng)
    longest = csr_of([[0, 2] if u % 9000 == 0 else [0] for u in range(LONGEST)], 3, rng)
    return {"lengths": lengths, "lengths_t": lengths.transpose(), "longest": longest}


def operand(n, f, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((n, f)).astype(np.float32)


def orth_sizes():
    """(n, f) with n in {f, f + 1, 31, 32, 33, 1025}, n >= f."""
    return [(n, f) for f in ORTH_FS for n in sorted({f, f + 1, 31, 32, 33, 1025}) if n >= f]


def orth_input(n, f, kind):
    """Gaussian; `scaled`: its columns scaled over a 10^3 range."""
    Y = operand(n, f, 1000 * n + f)
    if kind == "scaled" and f > 1:
        Y = Y * (10.0 ** (3.0 * np.arange(f) / (f - 1))).astype(np.float32)
    return np.ascontiguousarray(Y, np.float32)


def orth_key(n, f, kind):
    return "%d-%d-%s" % (n, f, kind)


@functools.lru_cache(maxsize=None)
def start(name):
    t = tables()[name]
    Q0 = ref.start(t.csr.cols, t.f)
    Q0.setflags(write=False)
    return Q0


@functools.lru_cache(maxsize=None)
def run64(name):
    """(P, Q, captured, total) of the float64 reference from the library's start, once per process and read-only."""
    t = tables()[name]
    out = ref.svd64(ref.dense(t.csr), start(name), t.sweeps)
    for a in out[:2]:
        a.setflags(write=False)
    return out


# ---- judgements ------------------------------------------------------------------------------------------------------------------
def pinned(measured, recorded):
    """A recorded figure holds: the measured one is at most it and at least half of it, or the record is the floor."""
    return measured <= recorded and (recorded <= 2 * measured or recorded <= FLOOR * 1.01)


def gamma(n):
    return n * U / (1 - n * U)


def judge_product(csr, D, out, transpose=False):
    """out = X D (X^T D) against float64 by the order-free bound |err| <= gamma_n sum |r d|, n the row's entries: derived from one
    rounding per term and at most n - 1 additions on any path from a term to the sum, whatever the order."""
    D64 = np.asarray(D, np.float64)
    if transpose:
        csr = csr.transpose()
    want = np.zeros((csr.rows, D64.shape[1]))
    mass = np.zeros_like(want)
    terms = np.asarray(csr.data, np.float64)[:, None] * D64[np.asarray(csr.indices)]
    stored = np.flatnonzero(np.diff(csr.indptr) > 0)  # a row's entries are consecutive: one segment per row that has any
    if len(stored):
        want[stored] = np.add.reduceat(terms, np.asarray(csr.indptr)[stored], axis=0)
        mass[stored] = np.add.reduceat(np.abs(terms), np.asarray(csr.indptr)[stored], axis=0)
    out = np.asarray(out, np.float64)
    if out.shape != want.shape or not np.isfinite(out).all():
        return ["the product has the wrong shape or is not finite"]
    n = np.diff(csr.indptr).astype(np.float64)[:, None]
    over = np.abs(out - want) - gamma(n) * mass
    bad = np.argwhere(over > 0)
    return ["row %d column %d is %.3g past the bound" % (bad[0][0], bad[0][1], over.max())] if len(bad) else []


def judge_padding(padded, f):
    return [] if not np.asarray(padded)[:, f:].any() else ["a padding column is not zero"]


def judge_orth(Q, Y, recorded, margin=MARGIN):
    """Q = orth(Y): orthonormal within margin x the recorded |Q^T Q - I|max, and Y's columns inside its span within margin x the recorded
    span error."""
    Q = np.asarray(Q)
    if Q.shape != np.asarray(Y).shape or not np.isfinite(Q).all():
        return ["Q has the wrong shape or is not finite"]
    out = []
    e, s = ref.orth_error(Q), ref.span_error(Q, Y)
    if not e <= margin * recorded[0]:
        out.append("|Q^T Q - I|max is %.3g, more than %g x %.3g" % (e, margin, recorded[0]))
    if not s <= margin * recorded[1]:
        out.append("the span error is %.3g, more than %g x %.3g" % (s, margin, recorded[1]))
    return out


def judge_model(name, P, Q, captured, total, user_bias=None, item_bias=None, margin=MARGIN):
    """An end-to-end result against the float64 reference from the same start: the scores, Q's orthonormality, both biases, and
    captured <= total, captured within its recorded distance."""
    P64, Q64, c64, t64 = run64(name)
    rec = SVD_DISTANCE[name]
    out = []
    if np.asarray(P).shape != P64.shape or np.asarray(Q).shape != Q64.shape or not (np.isfinite(P).all() and np.isfinite(Q).all()):
        return ["P or Q has the wrong shape or is not finite"]
    d = ref.score_distance(P, Q, P64, Q64)
    if not d <= margin * rec[0]:
        out.append("the scores are %.3g from float64, more than %g x %.3g" % (d, margin, rec[0]))
    e = ref.orth_error(Q)
    if not e <= margin * rec[1]:
        out.append("|Q^T Q - I|max is %.3g, more than %g x %.3g" % (e, margin, rec[1]))
    for b, what in ((user_bias, "user"), (item_bias, "item")):
        if b is not None and np.asarray(b).any():
            out.append("the %s biases are not zero" % what)
    if not captured <= total * (1 + 4 * U):
        out.append("captured %.17g exceeds total %.17g" % (captured, total))
    if not abs(total - t64) <= 4 * U * t64:
        out.append("total is %.17g, float64 has %.17g" % (total, t64))
    if not abs(captured - c64) <= margin * rec[2] * c64:
        out.append("captured is %.3g from float64's, more than %g x %.3g" % (abs(captured - c64) / c64, margin, rec[2]))
    return out


def judge_lists(ids, want_ids):
    """Two sets of lists are the same lists."""
    return [] if np.array_equal(ids, want_ids) else ["the lists differ"]


# ---- the ML_SMALL experiment -----------------------------------------------------------------------------------------------------
def ml_small():
    import knn_checks
    return knn_checks.ml_small()


def lists_of(S, train, k):
    """The k best unstored items of every row of the score matrix S (ties by ascending id)."""
    import knn_reference64 as kref
    ok = np.ones(S.shape, bool)
    ok[np.repeat(np.arange(train.rows), np.diff(train.indptr)), train.indices] = False
    return kref.select(S, ok, k)[0]


@functools.lru_cache(maxsize=None)
def ml_small_run():
    """The float64 experiment -> (hits, P64, Q64)."""
    import knn_reference64 as kref
    train, held = ml_small()
    P, Q, _, _ = ref.svd64(ref.dense(train), ref.start(train.cols, ML_SMALL_F), ML_SMALL_SWEEPS)
    return kref.hits_at(lists_of(P @ Q.T, train, ML_SMALL_K), held), P, Q


def within_reach(dist, margin=MARGIN):
    """The users of the ML_SMALL experiment whose hit a run at margin x dist from float64 may decide differently: the held-out item's
    score and the k-th best other candidate's differ by a nonzero amount of at most twice the scores' error, margin x dist x max |S|."""
    train, held = ml_small()
    _, P, Q = ml_small_run()
    S = P @ Q.T
    err = margin * dist * float(np.abs(S).max())
    reach = 0
    for u in range(train.rows):
        target = int(held.indices[held.indptr[u]])
        others = np.ones(train.cols, bool)
        others[train.indices[train.indptr[u]:train.indptr[u + 1]]] = False
        others[target] = False
        others = np.flatnonzero(others)
        kth = others[np.lexsort((others, -S[u, others]))[ML_SMALL_K - 1]]
        reach += 0 < abs(S[u, target] - S[u, kth]) <= 2 * err
    return int(reach)
