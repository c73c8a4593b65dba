"""TEST INFRASTRUCTURE: the conjugate-gradient implicit half-step (cu2rec_model_als_implicit_cg) restated with numpy.

For a row of 1 .. CHUNK entries the half-step takes `steps` steps of CG on A x = b with
    A = G0 + sum_entries w q q^T + reg I,   b = sum_entries (1 + w) q,   w = alpha r
(ials_reference64.row_system), warm-started from the row's current factors -- from zero where one of them is not finite:
    r = b - A x0, p = r, rho = r . r; each step: rho == 0 -> stop; d = p . A p; d == 0 -> stop; a = rho / d; x += a p;
    r -= a A p; rho' = r . r; p = r + (rho' / rho) p; rho = rho'.
A row is unsolved (NaN here; the kernel leaves it its bits and counts it) when a rho or a d is not finite, a d is negative or the
final x is not finite.  Rows without entries are zero rows; rows of more than CHUNK entries are not CG's (the kernels solve them
exactly): they come back as NaN unless the caller leaves them out.

cg_rows() is float64 from the float32 values as they are.  cg_rows_f32() is the same iteration in float32 with A applied as an
operator -- G0 from ials_reference64.gram_f32, the entries' term as Z^T (w (Z v)) -- as the kernel applies it (not in its
summation order); it runs on the CPU only, to show that the GPU test sets are fair."""
import numpy as np

import ials_reference64 as ref

CHUNK = ref.CHUNK
MUTATIONS = ("steps_minus_1", "cold_start", "no_g0", "no_reg", "rhs_w")


def _start(x0, r, f, cold):
    x = np.zeros(f) if x0 is None else np.asarray(x0[r], np.float64)[:f].copy()
    if cold or not np.isfinite(x).all():
        x[:] = 0.0
    return x


def _cg(apply_a, b, x, steps, dtype):
    """The iteration above in `dtype`; returns the iterates after 1 .. steps steps (a stopped iteration repeats its x; an
    unsolved row is NaN from the step that failed on)."""
    out = []
    nan = np.full(len(b), np.nan)
    with np.errstate(all="ignore"):
        r = (b - apply_a(x)).astype(dtype)
        p = r.copy()
        rho = dtype(r @ r)
        failed, stopped = not np.isfinite(rho), False
        for _ in range(steps):
            if not (failed or stopped):
                if rho == 0:
                    stopped = True
                else:
                    ap = apply_a(p).astype(dtype)
                    d = dtype(p @ ap)
                    if not np.isfinite(d) or d < 0:
                        failed = True
                    elif d == 0:
                        stopped = True
                    else:
                        a = dtype(rho / d)
                        x = (x + a * p).astype(dtype)
                        r = (r - a * ap).astype(dtype)
                        rho1 = dtype(r @ r)
                        if not np.isfinite(rho1):
                            failed = True
                        else:
                            p = (r + dtype(rho1 / rho) * p).astype(dtype)
                            rho = rho1
            out.append(nan if failed or not np.isfinite(x).all() else np.asarray(x, np.float64).copy())
    return out


def cg_rows_upto(indptr, indices, data, X, reg, alpha, x0, steps, mutation=None, rows=None, G0=None):
    """[x after 1 step, ..., x after `steps` steps], each (len(rows), f) float64: one pass for several step counts."""
    assert mutation is None or mutation in MUTATIONS
    f = X.shape[1]
    if G0 is None:
        G0 = ref.gram64(X)
    if mutation == "no_g0":
        G0 = np.zeros((f, f))
    if mutation == "steps_minus_1":
        steps -= 1
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, np.int64)
    out = [np.zeros((len(rows), f)) for _ in range(max(steps, 1))]
    for k, r in enumerate(rows):
        n = int(indptr[r + 1] - indptr[r])
        if n == 0:
            continue
        if n > CHUNK:
            for o in out:
                o[k] = np.nan
            continue
        A, b = ref.row_system(indptr, indices, data, X, reg, alpha, r, G0, "rhs_w" if mutation == "rhs_w" else None)
        if mutation == "no_reg":
            A = A - ref._f32(reg) * np.eye(f)
        x = _start(x0, r, f, mutation == "cold_start")
        if steps == 0:  # steps_minus_1 at one step: the start itself
            out[0][k] = x
            continue
        for s, xs in enumerate(_cg(lambda v: A @ v, b, x, steps, np.float64)):
            out[s][k] = xs
    return out


def cg_rows(indptr, indices, data, X, reg, alpha, x0, steps, mutation=None, rows=None, G0=None):
    """Rows `rows` (default: all) of one CG half-step of `steps` steps in float64 against the partner rows X -> (len(rows), f).
    x0: the side's current factors, one row per row of the CSR (None: zeros).  G0: X^T X in float64 where the caller has it.
    mutation: one of MUTATIONS -- the five deliberate mistakes the GPU sets must be able to see: "steps_minus_1" (one step too
    few), "cold_start" (x0 = 0), "no_g0" / "no_reg" (the all-pairs Gram / the regulariser left out of the matvec), "rhs_w" (the
    right-hand side weighted by w)."""
    return cg_rows_upto(indptr, indices, data, X, reg, alpha, x0, steps, mutation, rows, G0)[-1]


def cg_rows_f32(indptr, indices, data, X, reg, alpha, x0, steps, rows=None, G0=None):
    """cg_rows_upto() in float32 with A applied as an operator; G0: ials_reference64.gram_f32(X) where the caller has it."""
    F = np.float32
    X = np.asarray(X, F)
    f = X.shape[1]
    G0 = ref.gram_f32(X) if G0 is None else np.asarray(G0, F)
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, np.int64)
    out = [np.zeros((len(rows), f)) for _ in range(steps)]
    for k, r in enumerate(rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            continue
        if hi - lo > CHUNK:
            for o in out:
                o[k] = np.nan
            continue
        Z = X[indices[lo:hi]]
        with np.errstate(all="ignore"):
            w = F(alpha) * np.asarray(data[lo:hi], F)
            b = Z.T @ (F(1) + w)

            def apply_a(v, Z=Z, w=w):
                return (G0 @ v + Z.T @ (w * (Z @ v))) + F(reg) * v
            x = _start(x0, r, f, False).astype(F)
            for s, xs in enumerate(_cg(apply_a, b, x, steps, F)):
                out[s][k] = xs
    return out
