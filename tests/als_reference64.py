"""TEST INFRASTRUCTURE: alternating least squares (cu2rec_model_als) restated in float64 with numpy.

The objective is the one every SGD mode takes stochastic steps on (include/cu2rec_amd.h, "Alternating least squares"):
    L = 1/2 sum_(u,i) (r_ui - gb - ub_u - ib_i - p_u . q_i)^2
      + 1/2 sum_u n_u (P_reg |p_u|^2 + user_bias_reg ub_u^2) + 1/2 sum_i m_i (Q_reg |q_i|^2 + item_bias_reg ib_i^2)
A user half-step solves, for every user with n_u >= 1, x = [p_u; ub_u] from
    (sum_i z_i z_i^T + n_u diag(P_reg, ..., P_reg, user_bias_reg)) x = sum_i (r_ui - gb - ib_i) z_i,   z_i = [q_i; 1];
an item half-step the same with the roles swapped.  Everything is float64, starting from the float32 values of the model as they
are (widened exactly); the hyper-parameters are the float32 values the kernels see, widened.  Rows without ratings keep their
values.  csr: anything with indptr / indices / data / rows / cols (api.HostCSR).

Below the float64 half-step: row_residual() judges one solved row by its backward error (a derived rounding bound on A x - b, so
the judgement holds at any conditioning), and solve_row_f32() restates the row solve in float32 numpy, used on the CPU only to show
that the inputs of the GPU edge tests are fair and that the bound notices deliberate mistakes."""
import numpy as np


def _f32(x):
    return float(np.float32(x))


def transpose(csr):
    """(indptr, indices, data) of the item-major view: item i's users in ascending order, repeats kept."""
    rows_of = np.repeat(np.arange(csr.rows, dtype=np.int64), np.diff(csr.indptr))
    order = np.argsort(csr.indices, kind="stable")
    indptr = np.zeros(csr.cols + 1, np.int64)
    np.cumsum(np.bincount(csr.indices, minlength=csr.cols), out=indptr[1:])
    return indptr, rows_of[order], np.asarray(csr.data, np.float64)[order]


def system(indptr, indices, data, X, xb, gb, reg, reg_b, r):
    """(A, b) of row r: the normal equations of its half-step, float64."""
    f = X.shape[1]
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    n = hi - lo
    idx = indices[lo:hi]
    Z = np.empty((n, f + 1))
    Z[:, :f] = X[idx]
    Z[:, f] = 1.0
    t = np.asarray(data[lo:hi], np.float64) - _f32(gb) - xb[idx]
    diag = np.full(f + 1, _f32(reg))
    diag[f] = _f32(reg_b)
    return Z.T @ Z + n * np.diag(diag), Z.T @ t


def solve_rows(indptr, indices, data, X, xb, Y, yb, gb, reg, reg_b):
    """The half-step for one side: rows of Y / yb solved against partner rows X / xb.  Returns new float64 (Y, yb)."""
    X, xb = np.asarray(X, np.float64), np.asarray(xb, np.float64)
    Y, yb = np.array(Y, np.float64), np.array(yb, np.float64)
    f = X.shape[1]
    for r in range(len(indptr) - 1):
        if indptr[r + 1] == indptr[r]:
            continue
        A, b = system(indptr, indices, data, X, xb, gb, reg, reg_b, r)
        x = np.linalg.solve(A, b)
        Y[r], yb[r] = x[:f], x[f]
    return Y, yb


def half_step(csr, P, Q, ub, ib, gb, hyper, side):
    """One half-step from the given values (float32 or float64 arrays) -> float64 (P, Q, ub, ib).  hyper: (lr, P_reg, Q_reg,
    user_bias_reg, item_bias_reg); side: "users" or "items"."""
    _, P_reg, Q_reg, ubr, ibr = hyper
    P, Q = np.array(P, np.float64), np.array(Q, np.float64)
    ub, ib = np.array(ub, np.float64), np.array(ib, np.float64)
    if side == "users":
        Pn, ubn = solve_rows(np.asarray(csr.indptr, np.int64), np.asarray(csr.indices, np.int64),
                             np.asarray(csr.data, np.float64), Q, ib, P, ub, gb, P_reg, ubr)
        return Pn, Q, ubn, ib
    t_indptr, t_indices, t_data = transpose(csr)
    Qn, ibn = solve_rows(t_indptr, t_indices, t_data, P, ub, Q, ib, gb, Q_reg, ibr)
    return P, Qn, ub, ibn


def objective(csr, P, Q, ub, ib, gb, hyper):
    """L in float64 (the SGD modes' objective at the given parameters)."""
    _, P_reg, Q_reg, ubr, ibr = (_f32(h) for h in hyper)
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    ub, ib = np.asarray(ub, np.float64), np.asarray(ib, np.float64)
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    items = np.asarray(csr.indices, np.int64)
    e = np.asarray(csr.data, np.float64) - _f32(gb) - ub[users] - ib[items] - np.einsum("ij,ij->i", P[users], Q[items])
    nu = np.zeros(P.shape[0])
    nu[:csr.rows] = np.diff(np.asarray(csr.indptr, np.int64))
    mi = np.bincount(items, minlength=Q.shape[0]).astype(np.float64)
    return 0.5 * (e @ e + nu @ (P_reg * np.einsum("ij,ij->i", P, P) + ubr * ub * ub)
                  + mi @ (Q_reg * np.einsum("ij,ij->i", Q, Q) + ibr * ib * ib))


def rmse(csr, P, Q, ub, ib, gb):
    """Root mean squared residual over the ratings of csr, float64."""
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    items = np.asarray(csr.indices, np.int64)
    e = (np.asarray(csr.data, np.float64) - _f32(gb) - np.asarray(ub, np.float64)[users] - np.asarray(ib, np.float64)[items]
         - np.einsum("ij,ij->i", np.asarray(P, np.float64)[users], np.asarray(Q, np.float64)[items]))
    return float(np.sqrt(e @ e / max(len(e), 1)))


def run(csr, P, Q, ub, ib, gb, hyper, sweeps, test=None):
    """`sweeps` full sweeps (users, then items) in float64 -> (P, Q, ub, ib, [test RMSE after each sweep] or None)."""
    state = (P, Q, ub, ib)
    curve = []
    for _ in range(sweeps):
        state = half_step(csr, *state, gb, hyper, "users")
        state = half_step(csr, *state, gb, hyper, "items")
        if test is not None:
            curve.append(rmse(test, *state, gb))
    return state + ((curve if test is not None else None),)


# ---- a solved row judged by its backward error -----------------------------------------------------------------------------
U32 = 2.0 ** -24  # unit roundoff of float32


def _gamma(k):
    return k * U32 / (1.0 - k * U32)


def row_residual(indptr, indices, data, X, xb, gb, reg, reg_b, r, x):
    """(A, b, A x - b, bound) for row r and a given solution x = [factors; bias]: the float64 system of system(), the float64
    residual of x, and an entrywise rounding bound on |A x - b| (a vector of f + 1 entries) that any float32 evaluation of the
    half-step's arithmetic meets; judge a row by residual_ratio().

    Derivation (first order in u = 2^-24; n = the row's ratings, D = f + 1, Z = [X[idx], 1], |.| and <= entrywise):
      * t_i = (r_i - gb) - xb_i is formed by two float subtractions, so |t^_i - t_i| <= 2 u (|r_i| + |gb| + |xb_i|) =: 2 u s_i
        (relative to the terms, not to t).
      * An entry of Z^T Z or Z^T t^ is a float sum of n products: in any order and any grouping (LDS stages, chunks, chunk-order
        summation) its error is at most gamma_n times the sum of the absolute products (Higham, Accuracy and Stability of
        Numerical Algorithms, 2nd ed., eq. 3.5).  n * reg and its addition to the diagonal are two more roundings.  With
        Aabs = |Z|^T |Z| + n diag(reg):
            |A^ - A| <= (n + 2) u Aabs,        |b^ - b| <= n u |Z|^T |t| + 2 u |Z|^T s    (<= (n + 2) u |Z|^T s, as |t| <= s).
      * The Cholesky factorisation with both triangular solves gives x with (A^ + E) x = b^, |E| <= gamma_(3D+1) |R^T| |R|
        (Thm 10.4), R the Cholesky factor of A^ (of A, to first order).  || |R^T| |R| ||_2 <= D ||A||_2 (eq. 10.7) would close
        the bound without R, but at D = 101 that factor D hides a swapped regulariser on a one-rating row, so the entrywise form
        is kept, with R from a float64 factorisation of A (eq. 10.7's form, on every entry, only where float64 cannot factorise
        A either).
      * So A x - b = -(A^ - A) x - E x + (b^ - b), and
            |A x - b| <= (n + 2) u Aabs |x| + n u |Z|^T |t| + 2 u |Z|^T s + gamma_(3D+1) |R^T| |R| |x|.
    The returned bound is twice that (the one safety factor, for the dropped second-order terms).  It is kept entrywise, not
    folded into one norm: a rating dropped from a 1,025-rating row at f = 100 moves single entries by |t q_j|, which the norm of
    the whole bound vector would cover."""
    X, xb = np.asarray(X, np.float64), np.asarray(xb, np.float64)
    x = np.asarray(x, np.float64)
    A, b = system(indptr, indices, data, X, xb, gb, reg, reg_b, r)
    f = X.shape[1]
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    n = hi - lo
    idx = indices[lo:hi]
    Zabs = np.empty((n, f + 1))
    Zabs[:, :f] = np.abs(X[idx])
    Zabs[:, f] = 1.0
    diag = np.full(f + 1, _f32(reg))
    diag[f] = _f32(reg_b)
    D = f + 1
    ax = np.abs(x)
    ratings = np.asarray(data[lo:hi], np.float64)
    s = np.abs(ratings) + abs(_f32(gb)) + np.abs(xb[idx])
    t = np.abs(ratings - _f32(gb) - xb[idx])
    try:
        Rabs = np.abs(np.linalg.cholesky(A))  # lower triangular: A = L L^T, |R^T| |R| = |L| |L|^T
        factor = Rabs @ (Rabs.T @ ax)
    except np.linalg.LinAlgError:
        factor = np.full(D, D * np.linalg.norm(A, 2) * np.linalg.norm(x))
    first = ((n + 2) * U32 * (Zabs.T @ (Zabs @ ax) + n * diag * ax) + n * U32 * (Zabs.T @ t) + 2 * U32 * (Zabs.T @ s)
             + _gamma(3 * D + 1) * factor)
    return A, b, A @ x - b, 2.0 * first


def residual_ratio(res, bound):
    """max_i |res_i| / bound_i: at most 1 for a row solved within rounding (an entry whose bound is 0 must be exactly 0)."""
    res, bound = np.abs(res), np.asarray(bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, res / bound, np.where(res > 0, np.inf, 0.0))
    return float(q.max())


def row_objective(A, b, x):
    """The part of L that depends on the row's own x: 1/2 x^T A x - b^T x (float64; the rest of L is constant in x)."""
    x = np.asarray(x, np.float64)
    return 0.5 * x @ (A @ x) - b @ x


def objective_slack(bound, x_new, x_old):
    """How far the row objective at x_new may lie above the one at x_old: phi is convex with gradient A x - b, so
    phi(x_old) >= phi(x_new) + (A x_new - b)^T (x_old - x_new), i.e. phi(x_new) <= phi(x_old) + |x_new - x_old|^T |res|
    -- and |res| is allowed up to `bound`, entry by entry."""
    return float(np.abs(np.asarray(x_new, np.float64) - np.asarray(x_old, np.float64)) @ np.asarray(bound))


# ---- the row solve restated in float32 (only to show on the CPU that the edge inputs are fair) ------------------------------
def solve_row_f32(indptr, indices, data, X, xb, gb, reg, reg_b, r, mutation=None):
    """Row r's half-step in float32 numpy: Gram and right-hand side by sequential accumulation over the ratings, n * reg onto
    the diagonal, right-looking Cholesky without pivoting, both substitutions.  Returns x (float32, f + 1) or None where a pivot
    is not a finite positive float or the solution is not finite.  mutation (for the tests that show the bound has teeth):
    "swap_reg" (factor and bias regulariser swapped), "n_minus_1" (the regulariser scaled by n - 1), "drop_1024" (the rating at
    position 1,024 of the row left out of the sums)."""
    F = np.float32
    X, xb = np.asarray(X, F), np.asarray(xb, F)
    f = X.shape[1]
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    n = hi - lo
    idx = np.asarray(indices[lo:hi])
    Z = np.empty((n, f + 1), F)
    Z[:, :f] = X[idx]
    Z[:, f] = 1.0
    t = (np.asarray(data[lo:hi], F) - F(gb)) - xb[idx]
    G, b = np.zeros((f + 1, f + 1), F), np.zeros(f + 1, F)
    for k in range(n):
        if mutation == "drop_1024" and k == 1024:
            continue
        G += np.outer(Z[k], Z[k])
        b += Z[k] * t[k]
    if mutation == "swap_reg":
        reg, reg_b = reg_b, reg
    diag = np.full(f + 1, F(reg), F)
    diag[f] = F(reg_b)
    G[np.diag_indices(f + 1)] += F(n - 1 if mutation == "n_minus_1" else n) * diag
    D = f + 1
    y = b.copy()
    for k in range(D):
        d = G[k, k]
        if not (d > 0 and np.isfinite(d)):
            return None
        l = np.sqrt(d)
        G[k, k] = l
        G[k + 1:, k] /= l
        y[k] /= l
        G[k + 1:, k + 1:] -= np.outer(G[k + 1:, k], G[k + 1:, k])
        y[k + 1:] -= G[k + 1:, k] * y[k]
    x = y
    for k in range(D - 1, -1, -1):  # L^T x = y, column by column
        x[k] /= G[k, k]
        x[:k] -= G[k, :k] * x[k]
    return x if np.isfinite(x).all() else None
