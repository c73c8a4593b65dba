"""Float64 restatement of EASE (include/cu2rec_amd.h, cu2rec_ease_*): the regularised Gram matrix G, P = G^-1 (numpy.linalg.inv), the
weights B_ij = -P_ij / P_jj with a zero diagonal, the scores of a history row and the lists.  The list judgement (ids, order, ties,
padding, the fold's bound) is knn_reference64.judge_lists.

A CSR here is anything with indptr / indices / data / rows / cols (cu2rec_amd.HostCSR); rows may be unsorted.  `mutation` names one
deliberate mistake (MUTATIONS): the checks of tests/ease_checks.py must catch each of them on some table.

Also the float32 restatement in the kernels' order: G as the fold acc = fma(r_ui, r_uj, acc) user after user, the inverse blocked with
the device's block order nb -- right-looking Cholesky (the diagonal tile column by column as an fma chain, the panel by forward
substitution, the trailing matrix minus L21 L21^T), the triangular inverse block column by block column from the last, P = W^T W
block row by block row, the mirror -- and the scores as the fold acc = fma(r, B_ij, acc) over the row's entries in ascending id.  The tile products are
numpy's float32 matrix products: the device's matrix-core chain adds the same terms one after the other, so the two differ in the
order of the sums inside a tile, which is what the device's margin over EASE_DISTANCE (tests/ease_checks.py) is for.
"""
import numpy as np

import knn_reference64 as kref

MUTATIONS = ("no_l2", "l2_twice", "row_scaling", "diagonal_kept", "sign", "self_listed", "untouched_dropped", "upper_not_mirrored",
             "tile_skipped")
U = kref.U


def dense(csr):
    """users x items float64 of the stored values (no row stores a column twice)."""
    X = np.zeros((csr.rows, csr.cols))
    X[kref.rows_of(csr), np.asarray(csr.indices, np.int64)] = np.asarray(csr.data, np.float64)
    return X


def gram(csr, l2, mutation=None):
    """G in float64; the diagonal is the float32 nearest to the sum of squares plus l2 (l2 as the float32 the C ABI takes)."""
    X = dense(csr)
    G = X.T @ X
    lam = float(np.float32(l2)) * {"no_l2": 0.0, "l2_twice": 2.0}.get(mutation, 1.0)
    d = np.arange(csr.cols)
    G[d, d] = (G[d, d] + lam).astype(np.float32).astype(np.float64)
    return G


def weights_from_inverse(P, mutation=None):
    d = np.diag(P).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        B = -P / (d[:, None] if mutation == "row_scaling" else d[None, :])
    if mutation != "diagonal_kept":
        np.fill_diagonal(B, 0.0)
    return -B if mutation == "sign" else B


def weights(G, mutation=None, nb=None):
    """B in float64 from G.  The two mistakes of the blocked inverse run the blocked algorithm in float64 with the mistake in it."""
    if mutation in ("upper_not_mirrored", "tile_skipped"):
        return weights_from_inverse(blocked_inverse(G, nb, np.float64, mutation), mutation)
    if not len(G):
        return np.zeros((0, 0))
    return weights_from_inverse(np.linalg.inv(G), mutation)


def row_scores(B, items, r):
    """One history row pushed through B (float64) -> (score, number of terms, sum of |terms|), each (cols,)."""
    cols = B.shape[0]
    if not len(items):
        return np.zeros(cols), np.zeros(cols), np.zeros(cols)
    terms = r[:, None] * B[items]
    return terms.sum(axis=0), np.full(cols, float(len(items))), np.abs(terms).sum(axis=0)


def recommend(B, history, exclude, users, k, mutation=None):
    """The k best candidates of every listed history row -> (ids, vals): every item outside the exclusion row is a candidate."""
    cols = B.shape[0]
    order, _ = kref.sorted_rows(history)
    users = range(history.rows) if users is None else users
    ids = np.full((len(users), k), -1, np.int32)
    vals = np.full((len(users), k), np.nan)
    for p, u in enumerate(users):
        items, r = kref.history_row(history, order, u)
        score, _, _ = row_scores(B, items, r)
        eligible = ~kref.excluded_mask(exclude, u, cols)
        if mutation == "untouched_dropped":
            eligible &= (B[items] != 0).any(axis=0) if len(items) else np.zeros(cols, bool)
        a, b = kref.select(score[None], eligible[None], k)
        ids[p], vals[p] = a[0], b[0]
    return ids, vals


def neighbours(B, rows, k, mutation=None):
    """The k largest B_ij, j != i, of every listed item i -> (ids, vals)."""
    cols = B.shape[0]
    ids = np.full((len(rows), k), -1, np.int32)
    vals = np.full((len(rows), k), np.nan)
    for p, i in enumerate(rows):
        eligible = np.ones(cols, bool)
        eligible[i] = mutation == "self_listed"
        if mutation == "untouched_dropped":
            eligible &= B[i] != 0
        a, b = kref.select(B[i][None], eligible[None], k)
        ids[p], vals[p] = a[0], b[0]
    return ids, vals


# ---- the float32 restatement in the kernels' order ------------------------------------------------------------------------------
def gram_f32(csr, l2):
    """G as the device folds it: user after user in ascending order, acc = fma(r_ui, r_uj, acc) in float32; l2 added to the finished sum."""
    order, _ = kref.sorted_rows(csr)
    data = np.asarray(csr.data, np.float32)
    acc = np.zeros((csr.cols, csr.cols), np.float32)
    for u in range(csr.rows):
        e = order[csr.indptr[u]:csr.indptr[u + 1]]
        it = np.asarray(csr.indices)[e]
        ix = np.ix_(it, it)
        acc[ix] = kref.fma32(data[e][:, None], data[e][None, :], acc[ix])
    d = np.arange(csr.cols)
    acc[d, d] = acc[d, d] + np.float32(l2)
    return acc


PIVOT_NOISE = 2.0 ** -22  # a pivot must be above the rounding noise of its own diagonal entry, 4 x 2^-24 x G_jj (ease.hip)


class NotPositiveDefinite(Exception):
    pass


def blocked_inverse(G, nb, dtype=np.float32, mutation=None):
    """P = G^-1 the device's way, every operation in `dtype`: the matrix padded with an identity block to whole blocks of nb, the four
    stages in one buffer, the lower triangle only until the mirror."""
    n = G.shape[0]
    T = -(-n // nb)
    N = T * nb
    A = np.eye(N, dtype=dtype)
    A[:n, :n] = G
    A[np.triu_indices(N, 1)] = 77.0  # what the upper triangle holds is nobody's business until the mirror
    g0 = np.diag(A).copy()
    fma = kref.fma32 if dtype == np.float32 else (lambda a, b, c: a * b + c)
    for kb in range(T):
        lo, hi = kb * nb, (kb + 1) * nb
        t = np.tril(A[lo:hi, lo:hi])
        for j in range(nb):
            d = t[j, j]
            if not (np.isfinite(d) and d > 0 and d > PIVOT_NOISE * g0[lo + j]):
                raise NotPositiveDefinite(lo + j)
            t[j, j] = np.sqrt(d)
            t[j + 1:, j] = t[j + 1:, j] / t[j, j]
            c = t[j + 1:, j]
            t[j + 1:, j + 1:] = np.tril(fma(-c[:, None], c[None, :], t[j + 1:, j + 1:]))
        A[lo:hi, lo:hi] = t
        if hi == N:
            break
        x = A[hi:, lo:hi]
        for j in range(nb):
            x[:, j] = (x[:, j] - x[:, :j] @ t[j, :j]) / t[j, j]
        upd = x @ x.T
        if mutation == "tile_skipped" and kb == 0:
            upd[-nb:, -nb:] = 0  # the last diagonal tile misses the first block column's update
        A[hi:, hi:] -= upd
    A = np.tril(A)  # from here on the upper triangle is not read until the mirror fills it
    for j in range(T - 1, -1, -1):
        lo, hi = j * nb, (j + 1) * nb
        l = A[lo:hi, lo:hi].copy()
        x = np.zeros((nb, nb), dtype)
        for i in range(nb):
            x[i, i] = dtype(1) / l[i, i]
            x[i, :i] = -(l[i, :i] @ x[:i, :i]) / l[i, i]
        A[lo:hi, lo:hi] = x
        if hi < N:
            A[hi:, lo:hi] = -((A[hi:, hi:] @ A[hi:, lo:hi]) @ x)
    for r in range(T):  # in place, as on the device: block row r reads the rows from r on and writes row r
        lo, hi = r * nb, (r + 1) * nb
        A[lo:hi, :hi] = A[lo:, lo:hi].T @ A[lo:, :hi]
    if mutation != "upper_not_mirrored":
        iu = np.triu_indices(N, 1)
        A[iu] = A.T[iu]
    return A[:n, :n]


def weights_f32(G32, nb):
    """B as the device makes it from its G: the blocked float32 inverse, then an IEEE division per entry."""
    if not len(G32):
        return np.zeros((0, 0), np.float32)
    P = blocked_inverse(np.asarray(G32, np.float32), nb, np.float32)
    B = -P / np.diag(P)[None, :]
    np.fill_diagonal(B, 0.0)
    return B.astype(np.float32)


def fold_f32(B32, items, r):
    acc = np.zeros(B32.shape[0], np.float32)
    for i, ri in zip(items, np.asarray(r, np.float32)):
        acc = kref.fma32(ri, B32[i], acc)
    return acc


def recommend_f32(B32, history, exclude, users, k):
    """recommend() as the device folds it: the row's entries in ascending id order, acc = fma(r, B_ij, acc) in float32."""
    cols = B32.shape[0]
    order, _ = kref.sorted_rows(history)
    users = range(history.rows) if users is None else users
    ids = np.full((len(users), k), -1, np.int32)
    vals = np.full((len(users), k), np.nan, np.float32)
    seen = {}
    for p, u in enumerate(users):
        if u not in seen:
            items, r = kref.history_row(history, order, u)
            seen[u] = [a[0] for a in kref.select(fold_f32(B32, items, r)[None], ~kref.excluded_mask(exclude, u, cols)[None], k)]
        ids[p], vals[p] = seen[u]
    return ids, vals


def neighbours_f32(B32, rows, k):
    ids, vals = neighbours(np.asarray(B32, np.float64), rows, k)
    return ids, vals.astype(np.float32)
