"""TEST INFRASTRUCTURE: logistic matrix factorization (cu2rec_model_lmf, include/cu2rec_amd.h) restated with numpy.

float64: gradient(), objective(), step(), run() -- the judge.  sigma and softplus come from tanh / logaddexp, so they hold at any
score.  float32: gradient_f32() restates the kernels of csrc/lmf.hip operation by operation in their order -- the score as the
fused-multiply-add chain score_tile.hpp's contract() runs over the factors (the two halves of the slots interleaved), the bias
expression ((gb + b_own) + b_partner) + dot, the all-pairs sum as one chain from zero per wavefront share (partner blocks of 32 dealt
round robin to four wavefronts, within a block the accumulator-row order of the MFMA) with the four added in wave order, the entries'
sum per group of 16 lanes in entry order with the groups added in group order -- and step_f32() the AdaGrad step.  It is what shows
that the bound below is fair; the device's expf is not numpy's, so it is a restatement, not a bit-for-bit prediction.

bound(): entrywise on |g - g*| for any float32 evaluation in any order.  With u = 2^-24, K = partners + the row's entries, f factors:
  * a score is f products and three bias additions: |s^ - s| <= (f + 4) u (|x| . |y| + |xb| + |yb| + |gb|) =: ds;  sigma' <= 1/4, so
    sigma moves by at most ds / 4, and so does 1 - sigma;
  * sigma itself (an exponential, an addition, a division) and the product with w and y are a handful of roundings, the sum of K
    terms in any order gamma_K times the sum of the absolute terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
    eq. 3.5), the regulariser's product and two subtractions a few more: (K + 8) u times the absolute terms.
  bound_e = (K + 8) u (sum_i sigma_i |y_ie| + sum_entries w (1 - sigma) |y_ie| + reg |x_e|) + sum_i 1/4 ds_i (1 + w_i) |y_ie|
and the bias' bound is the same with |y_ie| -> 1.  A single partner dropped from 1,000 is about 20 bounds."""
import numpy as np

from ials_reference64 import own_major

U = 2.0 ** -24

MUTATIONS = ("drop-last-partner", "unobserved-only", "w-sigma", "no-bias-column", "no-global-bias", "repeats-once", "reg-times-n",
             "regs-swapped")


def sigma(s):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(s, np.float64)))


def softplus(s):
    return np.logaddexp(0.0, np.asarray(s, np.float64))


def sides(csr, state, hyper, side):
    """(indptr, indices, data, X, xb, Y, yb, reg, reg_bias): the half-step of `side` as it reads the problem, rows inside the CSR."""
    P, Q, ub, ib = state
    indptr, indices, data, _ = own_major(csr, side)
    P, Q, ub, ib = P[:csr.rows], Q[:csr.cols], ub[:csr.rows], ib[:csr.cols]
    if side == "users":
        return indptr, indices, data, P, ub, Q, ib, hyper[1], hyper[3]
    return indptr, indices, data, Q, ib, P, ub, hyper[2], hyper[4]


def gradient(csr, state, gb, hyper, alpha, side, mutation=None):
    """float64 (g [n x f], gb [n]) of every own row inside the CSR.  mutation: one of MUTATIONS, a deliberate mistake."""
    indptr, indices, data, X, xb, Y, yb, reg, reg_b = sides(csr, state, hyper, side)
    X, xb, Y, yb = (np.asarray(a, np.float64) for a in (X, xb, Y, yb))
    n, f = X.shape
    g0 = 0.0 if mutation == "no-global-bias" else float(gb)
    if mutation == "regs-swapped":
        reg, reg_b = reg_b, reg
    rows = np.repeat(np.arange(n), np.diff(indptr))
    w = float(alpha) * np.asarray(data, np.float64)
    if mutation == "repeats-once":
        _, first = np.unique(rows * (len(Y) + 1) + indices, return_index=True)
        first = np.sort(first)
        rows, indices, w = rows[first], indices[first], w[first]
    Y1 = np.concatenate([Y, np.ones((len(Y), 1))], axis=1)
    if mutation == "no-bias-column":
        Y1[:, f] = 0.0
    S = g0 + xb[:, None] + yb[None, :] + X @ Y.T
    sg = sigma(S)
    if mutation == "drop-last-partner":
        sg[:, -1] = 0.0
    if mutation == "unobserved-only":
        sg[rows, indices] = 0.0
    dense = sg @ Y1
    s_e = g0 + xb[rows] + yb[indices] + np.einsum("ij,ij->i", X[rows], Y[indices])
    c = w * (sigma(s_e) if mutation == "w-sigma" else sigma(-s_e))
    sparse = np.zeros((n, f + 1))
    Ye = np.concatenate([Y[indices], np.ones((len(indices), 1))], axis=1)
    np.add.at(sparse, rows, c[:, None] * Ye)
    own = np.concatenate([X, xb[:, None]], axis=1)
    regs = np.concatenate([np.full(f, float(reg)), [float(reg_b)]])
    if mutation == "reg-times-n":
        regs = regs[None, :] * np.bincount(rows, minlength=n)[:, None]
    g = sparse - dense - regs * own
    return g[:, :f], g[:, f]


def bound(csr, state, gb, hyper, alpha, side):
    """The entrywise rounding bound of the module docstring -> (bound [n x f], bias bound [n])."""
    indptr, indices, data, X, xb, Y, yb, reg, reg_b = sides(csr, state, hyper, side)
    X, xb, Y, yb = (np.asarray(a, np.float64) for a in (X, xb, Y, yb))
    n, f = X.shape
    rows = np.repeat(np.arange(n), np.diff(indptr))
    w = np.abs(float(alpha) * np.asarray(data, np.float64))
    Y1 = np.concatenate([np.abs(Y), np.ones((len(Y), 1))], axis=1)
    S = float(gb) + xb[:, None] + yb[None, :] + X @ Y.T
    ds = (f + 4) * U * (np.abs(X) @ np.abs(Y).T + np.abs(xb)[:, None] + np.abs(yb)[None, :] + abs(float(gb)))
    absterms = sigma(S) @ Y1
    slope = 0.25 * ds @ Y1
    s_e = S[rows, indices]
    np.add.at(absterms, rows, (w * sigma(-s_e))[:, None] * Y1[indices])
    np.add.at(slope, rows, (0.25 * ds[rows, indices] * w)[:, None] * Y1[indices])
    own = np.abs(np.concatenate([X, xb[:, None]], axis=1))
    regs = np.concatenate([np.full(f, float(reg)), [float(reg_b)]])
    K = len(Y) + np.diff(indptr)
    b = (K + 8)[:, None] * U * (absterms + regs * own) + slope
    return b[:, :f], b[:, f]


def ratio(got, want, bnd):
    """max |got - want| / bound (inf where got is not finite)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / bnd
    return float(np.where(np.isfinite(got), np.nan_to_num(r, nan=0.0, posinf=np.inf), np.inf).max())


def objective(csr, state, gb, hyper, alpha):
    """The float64 log-posterior over the rows inside the CSR."""
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in state)
    P, Q, ub, ib = P[:csr.rows], Q[:csr.cols], ub[:csr.rows], ib[:csr.cols]
    S = float(gb) + ub[:, None] + ib[None, :] + P @ Q.T
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    s_e = S[rows, np.asarray(csr.indices)]
    w = float(alpha) * np.asarray(csr.data, np.float64)
    return float((w * (s_e - softplus(s_e))).sum() - softplus(S).sum()
                 - 0.5 * (hyper[1] * (P * P).sum() + hyper[2] * (Q * Q).sum() + hyper[3] * (ub * ub).sum() + hyper[4] * (ib * ib).sum()))


def step(x, a, g, lr):
    """The AdaGrad step in float64 -> (x', a')."""
    x, a, g = (np.asarray(v, np.float64) for v in (x, a, g))
    a2 = a + g * g
    with np.errstate(invalid="ignore", divide="ignore"):
        x2 = np.where(a2 > 0, x + (float(lr) * g) / np.sqrt(a2), x)
    return x2, a2


def step_f32(x, a, g, lr):
    """The AdaGrad step as lmf_step_kernel runs it: four float32 operations, each correctly rounded -> (x', a')."""
    x, a, g = (np.asarray(v, np.float32) for v in (x, a, g))
    a2 = a + g * g
    with np.errstate(invalid="ignore", divide="ignore"):
        x2 = np.where(a2 > 0, x + (np.float32(lr) * g) / np.sqrt(a2), x)
    return x2.astype(np.float32), a2.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the kernels' order, float32

def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def sigma_f32(s):
    """lmf_sigmoid: 1 / (1 + exp(-s)) for s >= 0, e / (1 + e) otherwise, in float32."""
    s = np.asarray(s, np.float32)
    one = np.float32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(s))
        return np.where(s >= 0, one / (one + e), e / (one + e)).astype(np.float32)


def contract_order(f):
    """The factor columns in the order contract() multiplies them in: slot c of the first half, then of the second, element-wise."""
    nslots = (f + 3) // 4
    s0 = (nslots + 1) // 2
    order = []
    for c in range(s0):
        for k in range(4):
            for slot in (c, s0 + c):
                if slot < nslots and 4 * slot + k < f:
                    order.append(4 * slot + k)
    return order


BLOCK_ORDER = [(reg & 3) + 8 * (reg >> 2) + 4 * h for reg in range(16) for h in range(2)]  # acc_row(reg, h), k = 0 before k = 1


def scores_f32(X, xb, Y, yb, gb):
    acc = np.zeros((len(X), len(Y)), np.float32)
    for c in contract_order(X.shape[1]):
        acc = _fma(X[:, c][:, None], Y[:, c][None, :], acc)
    return ((np.float32(gb) + xb)[:, None] + yb[None, :]) + acc


def gradient_f32(csr, state, gb, hyper, alpha, side):
    """float32 (g, gb) in the kernels' order (module docstring)."""
    indptr, indices, data, X, xb, Y, yb, reg, reg_b = sides(csr, state, hyper, side)
    X, xb, Y, yb = (np.ascontiguousarray(a, np.float32) for a in (X, xb, Y, yb))
    n, f = X.shape
    m = len(Y)
    Y1 = np.concatenate([Y, np.ones((m, 1), np.float32)], axis=1)
    sg = sigma_f32(scores_f32(X, xb, Y, yb, gb))
    part = np.zeros((4, n, f + 1), np.float32)
    for b0 in range(0, m, 32):
        wave = (b0 // 32) % 4
        for o in BLOCK_ORDER:
            if b0 + o < m:
                part[wave] = _fma(sg[:, b0 + o][:, None], Y1[b0 + o][None, :], part[wave])
    dense = ((part[0] + part[1]) + part[2]) + part[3]
    # the entries: group g = position % 4, each group's entries in ascending order
    nnz = len(indices)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    pos = np.arange(nnz) - indptr[rows]
    E = (f + 1 + 63) // 64
    Xp = np.zeros((n, 64 * E), np.float32)
    Xp[:, :f] = X
    Yp = np.zeros((m, 64 * E), np.float32)
    Yp[:, :f + 1] = Y1
    q = Yp[indices].reshape(nnz, E, 16, 4)  # [entry][k][lane16][component]: column 64 k + 4 lane16 + component
    v = Xp[rows].reshape(nnz, E, 16, 4)
    d = np.zeros((nnz, 16), np.float32)
    for k in range(E):
        for comp in range(4):
            d = _fma(q[:, k, :, comp], v[:, k, :, comp], d)
    lanes = np.arange(16)
    for mask in (8, 4, 2, 1):
        d = d + d[:, lanes ^ mask]
    s = ((np.float32(gb) + xb[rows]) + yb[indices]) + d[:, 0]
    c = (np.float32(alpha) * np.asarray(data, np.float32)) * sigma_f32(-s)
    acc = np.zeros((n, 4, f + 1), np.float32)
    Ye = Y1[indices]
    for t in range(int(pos.max()) // 4 + 1 if nnz else 0):
        sel = np.flatnonzero(pos // 4 == t)
        acc[rows[sel], pos[sel] % 4] = _fma(c[sel][:, None], Ye[sel], acc[rows[sel], pos[sel] % 4])
    sparse = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    own = np.concatenate([X, xb[:, None]], axis=1)
    regs = np.concatenate([np.full(f, np.float32(reg)), [np.float32(reg_b)]]).astype(np.float32)
    g = (sparse - dense) - regs * own
    return g[:, :f], g[:, f]


def objective_f32(csr, state, gb, hyper, alpha):
    """The log-posterior as cu2rec_model_lmf_objective forms it: the all-pairs scores in float32 (the kernel's chain), everything
    else in float64."""
    P, Q, ub, ib = (np.ascontiguousarray(a, np.float32) for a in state)
    P, Q, ub, ib = P[:csr.rows], Q[:csr.cols], ub[:csr.rows], ib[:csr.cols]
    dense = softplus(scores_f32(P, ub, Q, ib, gb).astype(np.float64)).sum()
    P, Q, ub, ib = (a.astype(np.float64) for a in (P, Q, ub, ib))
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    idx = np.asarray(csr.indices)
    s_e = ((float(gb) + ub[rows]) + ib[idx]) + np.einsum("ij,ij->i", P[rows], Q[idx])
    w = (np.float32(alpha) * np.asarray(csr.data, np.float32)).astype(np.float64)
    return float((w * (s_e - softplus(s_e))).sum() - dense
                 - 0.5 * (hyper[1] * (P * P).sum() + hyper[2] * (Q * Q).sum() + hyper[3] * (ub * ub).sum() + hyper[4] * (ib * ib).sum()))


def run(csr, state, gb, hyper, alpha, sweeps, f32=False):
    """`sweeps` sweeps (users, then items) from `state` with zeroed accumulators -> (state, [objective after every half-step]).
    f32: the float32 restatement (gradient_f32, step_f32) on float32 state; the objectives are float64 values at that state."""
    dt = np.float32 if f32 else np.float64
    P, Q, ub, ib = (np.array(a, dt) for a in state)
    aP, aQ, aub, aib = (np.zeros_like(a) for a in (P, Q, ub, ib))
    grad, stp = (gradient_f32, step_f32) if f32 else (gradient, step)
    objectives = []
    for _ in range(sweeps):
        g, gbias = grad(csr, (P, Q, ub, ib), gb, hyper, alpha, "users")
        P[:csr.rows], aP[:csr.rows] = stp(P[:csr.rows], aP[:csr.rows], g, hyper[0])
        ub[:csr.rows], aub[:csr.rows] = stp(ub[:csr.rows], aub[:csr.rows], gbias, hyper[0])
        objectives.append(objective(csr, (P, Q, ub, ib), gb, hyper, alpha))
        g, gbias = grad(csr, (P, Q, ub, ib), gb, hyper, alpha, "items")
        Q[:csr.cols], aQ[:csr.cols] = stp(Q[:csr.cols], aQ[:csr.cols], g, hyper[0])
        ib[:csr.cols], aib[:csr.cols] = stp(ib[:csr.cols], aib[:csr.cols], gbias, hyper[0])
        objectives.append(objective(csr, (P, Q, ub, ib), gb, hyper, alpha))
    return (P, Q, ub, ib), objectives
