"""TEST INFRASTRUCTURE: alternating least squares (cu2rec_model_als) restated in float64 with numpy.

The objective is the one every SGD mode takes stochastic steps on (include/cu2rec_amd.h, "Alternating least squares"):
    L = 1/2 sum_(u,i) (r_ui - gb - ub_u - ib_i - p_u . q_i)^2
      + 1/2 sum_u n_u (P_reg |p_u|^2 + user_bias_reg ub_u^2) + 1/2 sum_i m_i (Q_reg |q_i|^2 + item_bias_reg ib_i^2)
A user half-step solves, for every user with n_u >= 1, x = [p_u; ub_u] from
    (sum_i z_i z_i^T + n_u diag(P_reg, ..., P_reg, user_bias_reg)) x = sum_i (r_ui - gb - ib_i) z_i,   z_i = [q_i; 1];
an item half-step the same with the roles swapped.  Everything is float64, starting from the float32 values of the model as they
are (widened exactly); the hyper-parameters are the float32 values the kernels see, widened.  Rows without ratings keep their
values.  csr: anything with indptr / indices / data / rows / cols (api.HostCSR)."""
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
