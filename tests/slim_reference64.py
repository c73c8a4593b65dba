"""Float64 restatement of SLIM (include/cu2rec_amd.h, cu2rec_slim_create): cyclic coordinate descent on A = X^T X + l2 I from W = 0,
one coordinate after the other, plainly as the header writes it (sweeps64).  The same iteration carried through R = X W instead of
the items x items residual (sweeps64_rows): row k of C is A[k, :] - X[:, k]^T R - D_k W[k, :] with D = diag(A) - diag(X^T X), which
costs users x items per coordinate instead of items^2 -- what makes 2,049 items and ML_SMALL affordable; tests/test_slim_cpu.py
shows the two agree.

Also the restatement in the device's order (blocked): the matrix padded with an identity block to whole blocks of nb coordinates;
per block the in-block chain rho = fma(A_kk, w, c), c_s = fma(-delta, A_sk, c_s) on a copy of the block's rows of C, then
C -= A[:, block] @ Delta as one matrix product subtracted once.  In float32 the product is numpy's: the device's matrix-core chain
adds the same terms one after the other, so the two differ in the order of the sums inside a tile, which is what the device's margin
over SLIM_DISTANCE (tests/slim_checks.py) is for.  `mutation` names one deliberate mistake (MUTATIONS) of the blocked form: the
judgements of tests/slim_checks.py must catch each of them on some table.
"""
import numpy as np

import knn_reference64 as kref

MUTATIONS = ("no_threshold", "no_l2_in_denominator", "diagonal_kept", "negatives_kept", "in_block_delta_dropped", "own_rows_left_out",
             "tile_skipped", "update_sign")


def threshold(rho, l1, diag, positive):
    """The soft threshold of rho by l1 over diag, one-sided when positive."""
    if positive:
        return np.maximum(rho - l1, 0) / diag
    return np.copysign(np.maximum(np.abs(rho) - l1, 0) / diag, rho)


def sweeps64(A, l1, positive, sweeps, W=None):
    """`sweeps` sweeps in float64 from W (None: zeros) -> (W, [largest |delta| of each sweep]).  A: (items, items) float64."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    l1 = float(np.float32(l1))
    W = np.zeros((n, n)) if W is None else np.array(W, np.float64)
    C = A - A @ W
    tops = []
    for _ in range(sweeps):
        top = 0.0
        for k in range(n):
            rho = C[k] + A[k, k] * W[k]
            new = threshold(rho, l1, A[k, k], positive)
            new[k] = 0.0
            delta = new - W[k]
            W[k] = new
            nz = np.flatnonzero(delta)
            if len(nz):
                C[:, nz] -= A[:, k, None] * delta[None, nz]
                top = max(top, float(np.abs(delta[nz]).max()))
        tops.append(top)
    return W, tops


def sweeps64_rows(csr, diag, l1, positive, sweeps, until=None):
    """The same iteration through E = X - X W (users x items): rho = X[:, k]^T E + (A_kk - D_k) W[k, :], D_k = A_kk - sum_u x_uk^2.
    diag: the diagonal of A (float64 of the float32 sums plus l2, as ease_reference64.gram makes it) -> (W, tops, R = X W).
    until(W): called after every sweep; a true answer ends the run (len(tops) tells after how many)."""
    rows, idx = kref.rows_of(csr), np.asarray(csr.indices, np.int64)
    data = np.asarray(csr.data, np.float64)
    n = csr.cols
    X = np.zeros((csr.rows, n))
    X[rows, idx] = data
    by_item = np.argsort(idx, kind="stable")
    starts = np.searchsorted(idx[by_item], np.arange(n + 1))
    l1 = float(np.float32(l1))
    W = np.zeros((n, n))
    E = X.copy()
    tops = []
    for _ in range(sweeps):
        top = 0.0
        for k in range(n):
            e = by_item[starts[k]:starts[k + 1]]
            if not len(e):
                continue  # an unstored item: rho = 0 throughout
            u, x = rows[e], data[e]
            own = float(x @ x)  # (X^T X)_kk
            rho = x @ E[u] + own * W[k]
            new = threshold(rho, l1, diag[k], positive)
            new[k] = 0.0
            delta = new - W[k]
            W[k] = new
            nz = np.flatnonzero(delta)
            if len(nz):
                E[np.ix_(u, nz)] -= x[:, None] * delta[None, nz]
                top = max(top, float(np.abs(delta[nz]).max()))
        tops.append(top)
        if until is not None and until(W):
            break
    return W, tops, X - E


def blocked(A, l1, positive, sweeps, nb, dtype=np.float32, mutation=None, l2=None, tol=None):
    """The device's order, every operation in `dtype` -> (W, tops): stops after a sweep whose largest |delta| is <= tol (None or 0: never).
    l2 is read by the mutation that needs it alone."""
    n = A.shape[0]
    T = -(-n // nb)
    N = T * nb
    full = np.eye(N, dtype=dtype)
    full[:n, :n] = A
    A = full
    C = A.copy()
    W = np.zeros((N, N), dtype)
    fma = kref.fma32 if dtype == np.float32 else (lambda a, b, c: a * b + c)
    l1 = dtype(0 if mutation == "no_threshold" else np.float32(l1))
    signed = not positive or mutation == "negatives_kept"
    cols = np.arange(N)
    tops = []
    for _ in range(sweeps):
        top = dtype(0)
        for kb in range(T):
            lo, hi = kb * nb, (kb + 1) * nb
            akk = A[lo:hi, lo:hi]
            c = C[lo:hi].copy()
            delta = np.zeros((nb, N), dtype)
            for t in range(nb):
                d_kk = akk[t, t]
                rho = fma(d_kk, W[lo + t], c[t])
                over = d_kk - dtype(np.float32(l2)) if mutation == "no_l2_in_denominator" else d_kk
                with np.errstate(divide="ignore", invalid="ignore"):
                    new = threshold(rho, l1, over, not signed).astype(dtype)
                if mutation != "diagonal_kept":
                    new[lo + t] = 0
                delta[t] = new - W[lo + t]
                W[lo + t] = new
                if mutation != "in_block_delta_dropped" and t + 1 < nb:
                    c[t + 1:] = fma(-delta[t][None, :], akk[t + 1:, t][:, None], c[t + 1:])
            top = max(top, np.abs(delta).max())
            live = np.flatnonzero(delta.any(axis=0))  # the columns of the other tiles would lose an exact zero
            if not len(live):
                continue
            upd = A[:, lo:hi] @ delta[:, live]
            if mutation == "own_rows_left_out":
                upd[lo:hi] = 0
            if mutation == "tile_skipped" and kb == 0:
                upd[-nb:, cols[live] < nb] = 0  # the tile (last block row, first block column) misses the first block's update
            if mutation == "update_sign":
                C[:, live] += upd
            else:
                C[:, live] -= upd
        tops.append(float(top))
        if tol and top <= tol:
            break
    return W[:n, :n], tops


def kkt_residual(A, W, l1, positive):
    """The largest violation of the optimality conditions of W's columns, float64: with g = (A w - a_j)_k for k != j,
    |g + l1 sign(w_k)| on nonzeros, and on zeros the excess of |g| over l1 (positive: of -g over l1, the one-sided form; a negative
    weight under `positive` counts whole)."""
    A = np.asarray(A, np.float64)
    W = np.asarray(W, np.float64)
    l1 = float(np.float32(l1))
    g = A @ W - A
    res = np.where(W != 0, np.abs(g + l1 * np.sign(W)), np.maximum((-g if positive else np.abs(g)) - l1, 0))
    if positive:
        res = np.where(W < 0, np.abs(W) + res, res)
    np.fill_diagonal(res, 0.0)
    return float(res.max(initial=0.0))
