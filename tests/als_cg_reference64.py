"""TEST INFRASTRUCTURE: the conjugate-gradient explicit half-step (cu2rec_model_als_cg) restated with numpy.

For a row of 1 .. CHUNK ratings the half-step takes `steps` steps of CG on the row's normal equations A x = b of order f + 1
(als_reference64.system: z_i = [x_i; 1], t_i = r_i - gb - xb_i, A = sum z z^T + n diag(reg, ..., reg, reg_bias), b = sum t z),
warm-started from x0 = [the row's factors; its bias] -- from zero where one of the f + 1 values is not finite.  The iteration is
ials_cg_reference64._cg, imported and not copied: the implicit call's, stops and failures included.  A row is unsolved (NaN here;
the kernel leaves it its bits and counts it) when a rho or a d is not finite, a d is negative or the final x is not finite.  Rows
without ratings keep their values; rows of more than CHUNK ratings are not CG's (the kernels solve them exactly): they come back
as NaN unless the caller leaves them out.

cg_rows() is float64 from the float32 values as they are.  cg_rows_f32() is the same iteration in float32 with A applied as an
operator -- Z^T (Z v) + (n reg) v -- as the kernel applies it (not in its summation order); it runs on the CPU only, to show that
the GPU test sets are fair."""
import numpy as np

import als_reference64 as ref
from ials_cg_reference64 import CHUNK, _cg

MUTATIONS = ("steps_minus_1", "cold_start", "no_reg", "swap_reg", "reg_not_times_n", "no_bias_column", "t_without_partner_bias")


def start(Y, yb):
    """x0 of every row: [factors; bias], float64 (rows, f + 1)."""
    return np.concatenate([np.asarray(Y, np.float64), np.asarray(yb, np.float64)[:, None]], axis=1)


def _start(x0, r, D, cold):
    x = np.zeros(D) if x0 is None else np.asarray(x0[r], np.float64)[:D].copy()
    if cold or not np.isfinite(x).all():
        x[:] = 0.0
    return x


def row_system(indptr, indices, data, X, xb, gb, reg, reg_b, r, mutation=None):
    """(A, b) of row r in float64 -- als_reference64.system, or one of the deliberate mistakes made to it."""
    f = X.shape[1]
    n = int(indptr[r + 1] - indptr[r])
    diag = np.full(f + 1, ref._f32(reg))
    diag[f] = ref._f32(reg_b)
    if mutation == "swap_reg":
        return ref.system(indptr, indices, data, X, xb, gb, reg_b, reg, r)
    if mutation == "t_without_partner_bias":
        return ref.system(indptr, indices, data, X, np.zeros_like(xb), gb, reg, reg_b, r)
    A, b = ref.system(indptr, indices, data, X, xb, gb, reg, reg_b, r)
    if mutation == "no_reg":
        A = A - n * np.diag(diag)
    elif mutation == "reg_not_times_n":
        A = A - (n - 1) * np.diag(diag)
    elif mutation == "no_bias_column":  # z = [x_i; 0]: the bias sees its regulariser alone
        A[f, :f] = 0.0
        A[:f, f] = 0.0
        A[f, f] = n * diag[f]
        b[f] = 0.0
    return A, b


def cg_rows_upto(indptr, indices, data, X, xb, gb, reg, reg_b, x0, steps, mutation=None, rows=None):
    """[x after 1 step, ..., x after `steps` steps], each (len(rows), f + 1) float64: one pass for several step counts.
    x0: start(Y, yb) of the solved side, one row per row of the CSR (None: zeros)."""
    assert mutation is None or mutation in MUTATIONS
    X, xb = np.asarray(X, np.float64), np.asarray(xb, np.float64)
    D = X.shape[1] + 1
    if mutation == "steps_minus_1":
        steps -= 1
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, np.int64)
    out = [np.zeros((len(rows), D)) for _ in range(max(steps, 1))]
    for k, r in enumerate(rows):
        n = int(indptr[r + 1] - indptr[r])
        if n == 0:  # the row keeps its values
            for o in out:
                o[k] = 0.0 if x0 is None else np.asarray(x0[r], np.float64)[:D]
            continue
        if n > CHUNK:
            for o in out:
                o[k] = np.nan
            continue
        A, b = row_system(indptr, indices, data, X, xb, gb, reg, reg_b, int(r), mutation)
        x = _start(x0, r, D, mutation == "cold_start")
        if steps == 0:  # steps_minus_1 at one step: the start itself
            out[0][k] = x
            continue
        for s, xs in enumerate(_cg(lambda v: A @ v, b, x, steps, np.float64)):
            out[s][k] = xs
    return out


def cg_rows(indptr, indices, data, X, xb, gb, reg, reg_b, x0, steps, mutation=None, rows=None):
    """Rows `rows` (default: all) of one CG half-step of `steps` steps in float64 -> (len(rows), f + 1): [factors; bias].
    mutation: one of MUTATIONS -- the deliberate mistakes the GPU sets must be able to see: "steps_minus_1" (one step too few),
    "cold_start" (x0 = 0), "no_reg" (the diagonal term left out of the matvec), "swap_reg" (factor and bias regulariser swapped),
    "reg_not_times_n" (the regulariser not multiplied by the row's length), "no_bias_column" (z without its 1),
    "t_without_partner_bias" (t = r - gb)."""
    return cg_rows_upto(indptr, indices, data, X, xb, gb, reg, reg_b, x0, steps, mutation, rows)[-1]


def cg_rows_f32(indptr, indices, data, X, xb, gb, reg, reg_b, x0, steps, rows=None):
    """cg_rows_upto() in float32 with A applied as an operator."""
    F = np.float32
    X, xb = np.asarray(X, F), np.asarray(xb, F)
    f = X.shape[1]
    D = f + 1
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, np.int64)
    out = [np.zeros((len(rows), D)) for _ in range(steps)]
    for k, r in enumerate(rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            for o in out:
                o[k] = 0.0 if x0 is None else np.asarray(x0[r], np.float64)[:D]
            continue
        if hi - lo > CHUNK:
            for o in out:
                o[k] = np.nan
            continue
        idx = np.asarray(indices[lo:hi])
        Z = np.empty((hi - lo, D), F)
        Z[:, :f] = X[idx]
        Z[:, f] = 1.0
        with np.errstate(all="ignore"):
            t = (np.asarray(data[lo:hi], F) - F(gb)) - xb[idx]
            b = Z.T @ t
            nreg = np.full(D, F(hi - lo) * F(reg), F)
            nreg[f] = F(hi - lo) * F(reg_b)

            def apply_a(v, Z=Z, nreg=nreg):
                return Z.T @ (Z @ v) + nreg * v
            x = _start(x0, r, D, False).astype(F)
            for s, xs in enumerate(_cg(apply_a, b, x, steps, F)):
                out[s][k] = xs
    return out
