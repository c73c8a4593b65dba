"""PureSVD (include/cu2rec_amd.h: cu2rec_model_svd) restated on the host: the float64 reference of exactly the device's iteration, and
a float32 restatement of it in which every sum is sequential (numpy float32 element by element: no BLAS, so its figures are the same on
every machine).

    start: Q          each sweep: Y = orth(X Q)   Q = orth(X^T Y)          at the end: P = X Q

orth is Cholesky-QR applied twice: G = Y^T Y, G = L L^T, Y <- Y L^-T.  X is the dense users x items matrix of the stored values,
entries that repeat a column within a row summed.
"""
import numpy as np

PIVOT_NOISE = 2.0 ** -22  # the device's rule (EASE's): a pivot must be a finite number above this share of its diagonal entry


class BadPivot(Exception):
    def __init__(self, column):
        super().__init__("pivot %d" % column)
        self.column = column


def dense(csr):
    """X in float64, repeated entries summed."""
    X = np.zeros((csr.rows, csr.cols))
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    np.add.at(X, (rows, np.asarray(csr.indices)), np.asarray(csr.data, np.float64))
    return X


def start(cols, f, seed=42):
    """The item factors of a fresh model: initialize_normal_array(cols * f, f, seed 42), as float32."""
    import cu2rec_amd as cu
    return cu.initialize_normal_array(cols * f, f, seed=seed).reshape(cols, f)


# ---- float64 ----------------------------------------------------------------------------------------------------------------------
def cholesky(G, dtype):
    """Right-looking Cholesky of the lower triangle in `dtype`, with the device's pivot rule -> L."""
    G = np.array(G, dtype)
    f = G.shape[0]
    diag = G.diagonal().copy()
    L = np.zeros_like(G)
    for k in range(f):
        d = G[k, k]
        if not (d > 0 and d > dtype(PIVOT_NOISE) * diag[k] and np.isfinite(d)):
            raise BadPivot(k)
        l = np.sqrt(d)
        L[k, k] = l
        c = (G[k + 1:, k] / l).astype(dtype)
        L[k + 1:, k] = c
        G[k + 1:, k + 1:] = (G[k + 1:, k + 1:] - (c[:, None] * c[None, :]).astype(dtype)).astype(dtype)
    return L


def inverse_lower(L, dtype):
    """W = L^-1 row by row (L W = I), the device's order: row k scaled by 1 / L_kk, then taken off the rows below."""
    f = L.shape[0]
    W = np.array(L, dtype)
    for k in range(f):
        p = dtype(1) / W[k, k]
        m = W[k + 1:, k].copy()
        W[k, :k] = (W[k, :k] * p).astype(dtype)
        W[k, k] = p
        W[k + 1:, :k] = (W[k + 1:, :k] - (m[:, None] * W[k, :k][None, :]).astype(dtype)).astype(dtype)
        W[k + 1:, k] = -(m * p).astype(dtype)
    return np.tril(W)


def orth64(Y):
    Y = np.asarray(Y, np.float64)
    for _ in range(2):
        W = inverse_lower(cholesky(Y.T @ Y, np.float64), np.float64)
        Y = Y @ W.T
    return Y


def iterate64(X, Q, sweeps):
    Q = np.asarray(Q, np.float64)
    for _ in range(sweeps):
        Y = orth64(X @ Q)
        Q = orth64(X.T @ Y)
    return Q


def svd64(X, Q0, sweeps):
    """-> P, Q, captured = |X Q|_F^2, total = |X|_F^2."""
    Q = iterate64(X, Q0, sweeps)
    P = X @ Q
    return P, Q, float((P * P).sum()), float((X * X).sum())


def optimum(X, f):
    """(the top-f projector of numpy.linalg.svd on the item side, sum of the f largest sigma^2)."""
    _, s, Vt = np.linalg.svd(X, full_matrices=False)
    V = Vt[:f].T
    return V @ V.T, float((s[:f] ** 2).sum())


# ---- float32, every sum sequential ------------------------------------------------------------------------------------------------
def multiply32(csr, D, transpose=False):
    """X D (or X^T D) in float32, a row's entries added one after the other in stored order (item-major: ascending row)."""
    D = np.asarray(D, np.float32)
    indptr, indices, data = np.asarray(csr.indptr), np.asarray(csr.indices), np.asarray(csr.data, np.float32)
    n_out = csr.rows
    if transpose:
        rows_of = np.repeat(np.arange(csr.rows), np.diff(indptr))
        order = np.argsort(indices, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=csr.cols))])
        indices, data, n_out = rows_of[order], data[order], csr.cols
    out = np.zeros((n_out, D.shape[1]), np.float32)
    length = np.diff(indptr)
    for k in range(int(length.max(initial=0))):
        rows = np.flatnonzero(length > k)
        e = indptr[rows] + k
        out[rows] = out[rows] + data[e][:, None] * D[indices[e]]
    return out


def gram32(Y):
    G = np.zeros((Y.shape[1],) * 2, np.float32)
    for y in np.asarray(Y, np.float32):
        G = G + y[:, None] * y[None, :]
    return G


def apply32(Y, W):
    """Y W^T in float32, the contraction index ascending."""
    Y, W = np.asarray(Y, np.float32), np.asarray(W, np.float32)
    out = np.zeros_like(Y)
    for k in range(Y.shape[1]):
        out[:, k:] = out[:, k:] + Y[:, k][:, None] * W[k:, k][None, :]
    return out


def orth32(Y):
    Y = np.asarray(Y, np.float32)
    for _ in range(2):
        Y = apply32(Y, inverse_lower(cholesky(gram32(Y), np.float32), np.float32))
    return Y


def svd32(csr, Q0, sweeps):
    """-> P, Q, captured, total: the device's algorithm in float32."""
    Q = np.asarray(Q0, np.float32)
    for _ in range(sweeps):
        Y = orth32(multiply32(csr, Q))
        Q = orth32(multiply32(csr, Y, transpose=True))
    P = multiply32(csr, Q)
    X = dense(csr)
    return P, Q, float((P.astype(np.float64) ** 2).sum()), float((X * X).sum())


# ---- what the judges measure ----------------------------------------------------------------------------------------------------
def orth_error(Q):
    Q = np.asarray(Q, np.float64)
    return float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max())


def span_error(Q, Y):
    """max |Q Q^T Y - Y| / max |Y|: what of Y's columns lies outside the span of Q."""
    Q, Y = np.asarray(Q, np.float64), np.asarray(Y, np.float64)
    return float(np.abs(Q @ (Q.T @ Y) - Y).max() / np.abs(Y).max())


def score_distance(P, Q, P64, Q64):
    S64 = P64 @ Q64.T
    return float(np.abs(np.asarray(P, np.float64) @ np.asarray(Q, np.float64).T - S64).max() / np.abs(S64).max())
