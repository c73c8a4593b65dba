"""Float64 restatement of the item-neighbourhood recommender (include/cu2rec_amd.h, cu2rec_knn_*): the weights, the similarities,
their truncation to the N best touched neighbours, the recommendation, and the error bounds the device's float32 folds are held to.
Dense per block of items (users x items matrices), so the bundled ML_SMALL takes seconds.

A CSR here is anything with indptr / indices / data / rows / cols (cu2rec_amd.HostCSR).  Rows may be unsorted; everything works on
the row-sorted order, as the library does.  `mutation` names one deliberate mistake (MUTATIONS): the checks of tests/knn_checks.py
must catch each of them on some table.

Also the float32 restatement in the kernels' order (neighbours_f32, recommend_f32): every score the fold acc = fma(alpha, v, acc) from
+0.0f over the partner list -- the users of the query's column in ascending order, or the history row's items in ascending id order.
numpy has no fused multiply-add: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32,
which differs from a true fma only where the float64 sum lands on a float32 tie.
"""
import numpy as np

WEIGHTINGS = ("count", "cosine", "tfidf", "bm25")
MUTATIONS = ("self_listed", "zeros_listed", "norm_over_users", "log_n", "ties_descending", "excluded_listed", "last_partner_dropped",
             "untruncated")
U = 2.0 ** -24  # float32 unit roundoff


def rows_of(csr):
    return np.repeat(np.arange(csr.rows), np.diff(csr.indptr))


def sorted_rows(csr):
    """(order, has_duplicate): the permutation that sorts every row's entries by column, and whether a row repeats a column."""
    rows, idx = rows_of(csr), np.asarray(csr.indices, np.int64)
    order = np.lexsort((idx, rows))
    same = (rows[order][1:] == rows[order][:-1]) & (idx[order][1:] == idx[order][:-1])
    return order, bool(same.any())


def weights(csr, weighting, k1=100.0, b=0.8, mutation=None):
    """w_ui of every stored entry in the CSR's own entry order, float64; k1 and b enter as the float32 the C ABI takes."""
    k1, b = float(np.float32(k1)), float(np.float32(b))
    r = np.asarray(csr.data, np.float64)
    rows, idx = rows_of(csr), np.asarray(csr.indices, np.int64)
    n_u = np.diff(csr.indptr).astype(np.float64)
    with np.errstate(divide="ignore"):  # the mistake's ln(0) of an empty row weighs nothing
        idf_u = np.log(float(csr.cols)) - (np.log(n_u) if mutation == "log_n" else np.log(1.0 + n_u))
    idf = idf_u[rows]

    def column_sum(x):
        return np.bincount(idx, weights=x, minlength=csr.cols)

    def unit(t):
        s = column_sum(t * t)[idx]
        if mutation == "norm_over_users":
            s = np.bincount(rows, weights=t * t, minlength=csr.rows)[rows]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(s > 0, t / np.sqrt(s), 0.0)

    if weighting == "count":
        return r.copy()
    if weighting == "cosine":
        return unit(r)
    if weighting == "tfidf":
        return unit(np.sqrt(r) * idf)
    if weighting == "bm25":
        c = column_sum(r)
        mean = c.sum() / csr.cols
        length = (1.0 - b) + (b * c[idx] / mean if mean != 0 else 0.0)
        den = k1 * length + r
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den != 0, r * (k1 + 1.0) / den * idf, 0.0)
    raise ValueError(weighting)


def weights_f32(csr, weighting, k1=100.0, b=0.8):
    """The device's evaluation: the same formulas in double, rounded to float32 once."""
    return weights(csr, weighting, k1, b).astype(np.float32)


def dense(csr, values):
    """(W, B): users x items float64 weights and the stored pattern."""
    W = np.zeros((csr.rows, csr.cols))
    B = np.zeros((csr.rows, csr.cols), bool)
    rows = rows_of(csr)
    W[rows, csr.indices] = np.asarray(values, np.float64)
    B[rows, csr.indices] = True
    return W, B


def drop_last_partner(W, B):
    """The query-side matrices with every column's last user removed (the mistake `last_partner_dropped`)."""
    Wq, Bq = W.copy(), B.copy()
    for i in range(W.shape[1]):
        users = np.flatnonzero(B[:, i])
        if len(users):
            Wq[users[-1], i], Bq[users[-1], i] = 0.0, False
    return Wq, Bq


def similarity_block(W, B, lo, hi, Wq=None, Bq=None):
    """Rows lo .. hi - 1 of the item x item product -> (S, touched, terms, sum of |terms|); an item is not its own candidate."""
    Wq, Bq = (W, B) if Wq is None else (Wq, Bq)
    S = Wq[:, lo:hi].T @ W
    terms = Bq[:, lo:hi].T.astype(np.float64) @ B.astype(np.float64)
    sabs = np.abs(Wq[:, lo:hi]).T @ np.abs(W)
    touched = terms > 0
    touched[np.arange(hi - lo), np.arange(lo, hi)] = False
    return S, touched, terms, sabs


def select(values, eligible, k, descending_ties=False):
    """The k best eligible candidates of every row, by descending value and then ascending id -> (ids, vals) with -1 / NaN padding."""
    q = values.shape[0]
    ids = np.full((q, k), -1, np.int32)
    vals = np.full((q, k), np.nan)
    for r in range(q):
        idx = np.flatnonzero(eligible[r])
        if not len(idx):
            continue
        v = values[r, idx]
        order = np.lexsort((-idx if descending_ties else idx, -v))[:k]
        ids[r, :len(order)] = idx[order]
        vals[r, :len(order)] = v[order]
    return ids, vals


def neighbours(csr, w, n, mutation=None, block=1024):
    """The N best touched neighbours of every item from entry weights w (float64 arithmetic) -> (ids, vals), items x N."""
    W, B = dense(csr, w)
    Wq, Bq = drop_last_partner(W, B) if mutation == "last_partner_dropped" else (W, B)
    ids = np.full((csr.cols, n), -1, np.int32)
    vals = np.full((csr.cols, n), np.nan)
    for lo in range(0, csr.cols, block):
        hi = min(lo + block, csr.cols)
        S, touched, _, _ = similarity_block(W, B, lo, hi, Wq, Bq)
        if mutation == "zeros_listed":
            touched = np.ones_like(touched)
            touched[np.arange(hi - lo), np.arange(lo, hi)] = False
        if mutation == "self_listed":
            touched[np.arange(hi - lo), np.arange(lo, hi)] = (Bq[:, lo:hi].sum(axis=0) > 0)
        ids[lo:hi], vals[lo:hi] = select(S, touched, n, mutation == "ties_descending")
    return ids, vals


def history_row(history, order, u):
    """(items ascending, raw values) of history row u; order: sorted_rows(history)[0]."""
    e = order[history.indptr[u]:history.indptr[u + 1]]
    return np.asarray(history.indices)[e].astype(np.int64), np.asarray(history.data, np.float64)[e]


def recommend_scores(list_ids, list_vals, items, r, cols):
    """One history row pushed through the lists -> (score, touched, terms, sum of |terms|), each (cols,)."""
    ids = list_ids[items]
    ok = ids >= 0
    contrib = np.where(ok, r[:, None] * np.where(ok, list_vals[items], 0.0), 0.0)
    flat = ids[ok]
    score = np.bincount(flat, weights=contrib[ok], minlength=cols)
    sabs = np.bincount(flat, weights=np.abs(contrib[ok]), minlength=cols)
    terms = np.bincount(flat, minlength=cols).astype(np.float64)
    return score, terms > 0, terms, sabs


def excluded_mask(exclude, u, cols):
    m = np.zeros(cols, bool)
    if exclude is not None and u < exclude.rows:
        m[np.asarray(exclude.indices)[exclude.indptr[u]:exclude.indptr[u + 1]]] = True
    return m


def recommend(list_ids, list_vals, history, exclude, users, k, mutation=None):
    """The k best candidates of every listed history row (float64 arithmetic on the given lists) -> (ids, vals)."""
    cols = list_ids.shape[0]
    order, _ = sorted_rows(history)
    users = range(history.rows) if users is None else users
    ids = np.full((len(users), k), -1, np.int32)
    vals = np.full((len(users), k), np.nan)
    for p, u in enumerate(users):
        items, r = history_row(history, order, u)
        if mutation == "last_partner_dropped":
            items, r = items[:-1], r[:-1]
        score, touched, _, _ = recommend_scores(list_ids, list_vals, items, r, cols)
        if mutation != "excluded_listed":
            touched &= ~excluded_mask(exclude, u, cols)
        ids[p], vals[p] = (a[0] for a in select(score[None], touched[None], k, mutation == "ties_descending"))
    return ids, vals


# ---- the float32 restatement in the kernels' order ------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def neighbours_f32(csr, w32, n):
    """neighbours() as the device folds it: user after user in ascending order, acc = fma(w_ui, w_uj, acc) in float32."""
    w32 = np.asarray(w32, np.float32)
    order, _ = sorted_rows(csr)
    acc = np.zeros((csr.cols, csr.cols), np.float32)
    touched = np.zeros((csr.cols, csr.cols), bool)
    for u in range(csr.rows):
        e = order[csr.indptr[u]:csr.indptr[u + 1]]
        it = np.asarray(csr.indices)[e]
        ix = np.ix_(it, it)
        acc[ix] = fma32(w32[e][:, None], w32[e][None, :], acc[ix])
        touched[ix] = True
    np.fill_diagonal(touched, False)
    ids, vals = select(acc, touched, n)
    return ids, vals.astype(np.float32)


def recommend_f32(list_ids, list_vals32, history, exclude, users, k):
    """recommend() as the device folds it: the row's items in ascending id order, acc = fma(r, s, acc) in float32."""
    cols = list_ids.shape[0]
    order, _ = sorted_rows(history)
    users = range(history.rows) if users is None else users
    ids = np.full((len(users), k), -1, np.int32)
    vals = np.full((len(users), k), np.nan, np.float32)
    for p, u in enumerate(users):
        items, r = history_row(history, order, u)
        acc = np.zeros(cols, np.float32)
        touched = np.zeros(cols, bool)
        for i, ri in zip(items, r.astype(np.float32)):
            j = list_ids[i][list_ids[i] >= 0]
            acc[j] = fma32(ri, list_vals32[i][:len(j)], acc[j])
            touched[j] = True
        touched &= ~excluded_mask(exclude, u, cols)
        a, b = select(acc[None], touched[None], k)
        ids[p], vals[p] = a[0], b[0]
    return ids, vals


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def fold_bound(terms, sabs):
    """What a float32 fma fold of `terms` terms may be away from the exact sum: 1.01 n 2^-24 sum |terms|."""
    return 1.01 * terms * U * sabs


def judge_lists(ids, vals, values, eligible, terms, sabs, k):
    """The checks (a) - (d) of one query's list against float64 `values` over the candidates: every listed value within the fold's
    bound, values non-increasing with equal ones by ascending id, no unlisted eligible candidate above the last listed value by more
    than both bounds, listed ids distinct and eligible, min(k, eligible) of them and padding behind.  -> list of complaints."""
    out = []
    n = int((ids >= 0).sum())
    want = min(k, int(eligible.sum()))
    if n != want or (ids[:n] < 0).any() or (ids[n:] != -1).any() or not np.isnan(vals[n:]).all():
        return ["%d listed, %d eligible for k = %d, or padding inside" % (n, int(eligible.sum()), k)]
    if n == 0:
        return out
    lid, lv = ids[:n].astype(np.int64), np.asarray(vals[:n], np.float64)
    if lid.max() >= len(eligible) or len(np.unique(lid)) != n or not eligible[lid].all():
        return ["a listed id is repeated, untouched, excluded or the query itself"]
    bound = fold_bound(terms, sabs)
    off = np.abs(lv - values[lid])
    if (off > bound[lid]).any():
        w = int(np.argmax(off - bound[lid]))
        out.append("(a) value of %d off by %.3g, bound %.3g" % (lid[w], off[w], bound[lid][w]))
    if (np.diff(lv) > 0).any() or ((np.diff(lv) == 0) & (np.diff(lid) < 0)).any():
        out.append("(b) values increase, or equal values by descending id")
    if n == k:
        rest = eligible.copy()
        rest[lid] = False
        over = values[rest] - (lv[-1] + bound[rest] + bound[lid[-1]])
        if len(over) and over.max() > 0:
            out.append("(c) an unlisted candidate is %.3g above the last listed value and both bounds" % over.max())
    return out


def hits_at(lists, held):
    """How many rows list their one held-out item."""
    target = np.asarray(held.indices)[np.asarray(held.indptr[:-1])]
    return int((lists == target[:, None]).any(axis=1).sum())


def popularity_lists(train, k):
    """The k most stored items outside each row (ties by ascending id): the baseline every recommender is compared against first."""
    count = np.bincount(train.indices, minlength=train.cols).astype(np.float64)
    out = np.full((train.rows, k), -1, np.int32)
    for u in range(train.rows):
        ok = np.ones(train.cols, bool)
        ok[train.indices[train.indptr[u]:train.indptr[u + 1]]] = False
        out[u] = select(count[None], ok[None], k)[0][0]
    return out
