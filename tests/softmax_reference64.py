"""TEST INFRASTRUCTURE: softmax matrix factorization (cu2rec_model_softmax, include/cu2rec_amd.h) restated with numpy.

float64: lse(), mass(), gradient(), objective(), run() -- the judge; the step is lmf_reference64.step.  The log-sum-exp subtracts the
row's maximum, so it holds at any score.  float32: lse_f32(), mass_f32() and gradient_f32() restate the kernels of csrc/softmax.hip
operation by operation in their order -- the score chain is lmf_reference64.scores_f32; the online (m, l) of the log-sum-exp per lane
(16 scores in register order), the two halves of a wavefront, the wavefront's steps (partner blocks of 32 dealt round robin to four
wavefronts), the four wavefronts in order; the push as one chain from zero per wavefront share in BLOCK_ORDER with the four added in
wave order; the entries' sum per group of 16 lanes in entry order with the groups added in group order; W_u in entry order.  The
device's expf / logf are not numpy's, so it is a restatement, not a bit-for-bit prediction.

The bounds, entrywise, first order in u = 2^-24, for any float32 evaluation of this form.  I partners, f factors, n the row's entries:
  * a score is f products and three bias additions (lmf_reference64): |s^ - s| <= (f + 4) u (|p| . |q| + |ub| + |ib| + |gb|) =: ds_ui;
  * expf and logf are allowed ULPS = 2 units in the last place each, a relative 2 ULPS u = 4u (the HIP math tables and the OpenCL
    specification, which the device library follows, list 1 ulp for both in their accurate forms: a factor 2 to spare);
  * log-sum-exp is convex with a gradient on the simplex, so the scores' errors move it by at most max_i ds_ui;
  * in the online sum a term exp(s_i - m) is formed with its argument rounded and is then carried through at most
    M = 5 + ceil(I / 128) merges, each one product with expf(m_old - m_new) and one addition, after at most 16 additions in its lane.
    The arguments along a term's path are all <= 0 and telescope to s_i - m, so their roundings add up to at most u (m - s_i)
    relative; the products, additions and expf's to (16 + M (2 + 2 ULPS)) u.  Weighted by pi_i:
      |l^ - l| / l <= (16 + M (2 + 2 ULPS)) u + u sum_i pi_i (m - s_i) =: dl_u;
  * lse = m + logf(l):  b_lse = max_i ds_ui + dl_u + 2 ULPS u |lse - m| + u |lse|;
  * pi^_ui = expf(s^ - lse^): the exponent is off by de_ui = ds_ui + b_lse_u + u |s_ui - lse_u|, so
      |pi^ - pi| <= pi (expm1(de_ui) + 2 ULPS u) =: pi e_ui;
  * a sum of K terms in any order is within gamma_K of the sum of the absolute terms (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., eq. 3.5); W_u is a sum of n_u terms, relative n_u u; the products with W, the regulariser's product and the
    two subtractions are a few roundings more, taken as 8 u.
  mass:   |sum_i pi^ - 1| <= sum_i pi_i e_ui + (I + 8) u
  users:  b_e = (I + n_u + 8) u (sum_entries |w| |q_ie| + Wabs_u sum_i pi_ui |q_ie| + P_reg |p_ue|) + Wabs_u sum_i pi_ui |q_ie| e_ui
  items:  b_e = (U + n_i + 8) u (sum_entries |w| |p_ue| + sum_u Wabs_u pi_ui |p_ue| + Q_reg |q_ie|)
                + sum_u Wabs_u pi_ui |p_ue| (e_ui + (n_u + 1) u)          (bias: |p_ue| -> 1, Q_reg |q_ie| -> item_bias_reg |ib_i|)
The users' bias gradient is an exact zero and is judged as one."""
import numpy as np

import lmf_reference64 as lref
from lmf_reference64 import BLOCK_ORDER, U, _fma, ratio, scores_f32, sides, step, step_f32  # noqa: F401 (ratio, step: the callers')

ULPS = 2.0

MUTATIONS = ("stored-items-only", "drop-last-partner", "no-max-subtraction", "no-W", "W-entry-count", "lse-model-shape",
             "no-bias-column", "repeats-once", "regs-swapped", "reg-times-n")


def _inside(csr, state):
    P, Q, ub, ib = state
    return P[:csr.rows], Q[:csr.cols], ub[:csr.rows], ib[:csr.cols]


def _scores(csr, state, gb):
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in _inside(csr, state))
    return float(gb) + ub[:, None] + ib[None, :] + P @ Q.T


def _lse_rows(S):
    """log sum exp over axis 1, the maximum subtracted; -inf for a row without columns."""
    if S.shape[1] == 0:
        return np.full(S.shape[0], -np.inf)
    m = S.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return m + np.log(np.exp(S - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(axis=1))


def lse(csr, state, gb):
    """float64 lse_u of every user inside the CSR, over every item inside it."""
    return _lse_rows(_scores(csr, state, gb))


def _pi(S, l):
    with np.errstate(invalid="ignore"):
        return np.exp(S - l[:, None])


def mass(csr, state, gb):
    S = _scores(csr, state, gb)
    return _pi(S, _lse_rows(S)).sum(axis=1)


def weights(csr):
    """W_u in float64."""
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    return np.bincount(rows, weights=np.asarray(csr.data, np.float64), minlength=csr.rows)[:csr.rows]


def gradient(csr, state, gb, hyper, side, mutation=None):
    """float64 (g [n x f], gb [n]) of every own row inside the CSR (csr: user-major).  mutation: one of MUTATIONS, a deliberate
    mistake."""
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in _inside(csr, state))
    nu, f = P.shape
    ni = len(Q)
    rows = np.repeat(np.arange(nu), np.diff(csr.indptr))
    idx = np.asarray(csr.indices, np.int64)
    w = np.asarray(csr.data, np.float64)
    S = float(gb) + ub[:, None] + ib[None, :] + P @ Q.T
    W = np.bincount(rows, weights=w, minlength=nu)[:nu] if len(w) else np.zeros(nu)
    if mutation == "no-W":
        W = np.ones(nu)
    if mutation == "W-entry-count":
        W = np.diff(csr.indptr).astype(np.float64)
    if mutation == "repeats-once":
        _, first = np.unique(rows * (ni + 1) + idx, return_index=True)
        first = np.sort(first)
        rows, idx, w = rows[first], idx[first], w[first]
    Sl = S
    if mutation == "stored-items-only":
        Sl = np.full(S.shape, -np.inf)
        Sl[rows, idx] = S[rows, idx]
    if mutation == "drop-last-partner" and side == "users":
        Sl = S.copy()
        Sl[:, -1] = -np.inf
    if mutation == "lse-model-shape":  # every item of the model, not of the CSR
        Pm, Qm, ubm, ibm = (np.asarray(a, np.float64) for a in state)
        l = _lse_rows(float(gb) + ubm[:nu, None] + ibm[None, :] + Pm[:nu] @ Qm.T)
    elif mutation == "no-max-subtraction":  # float32 exponentials of the raw scores
        with np.errstate(over="ignore", divide="ignore"):
            l = np.log(np.exp(S.astype(np.float32)).sum(axis=1, dtype=np.float32)).astype(np.float64)
    else:
        l = _lse_rows(Sl)
    with np.errstate(invalid="ignore", over="ignore"):
        pi = np.where(np.isneginf(Sl), 0.0, np.exp(Sl - l[:, None]))
    if mutation == "drop-last-partner" and side == "items":
        pi[-1, :] = 0.0
    if side == "users":
        reg = hyper[2] if mutation == "regs-swapped" else hyper[1]
        sparse = np.zeros((nu, f))
        np.add.at(sparse, rows, w[:, None] * Q[idx])
        regs = float(reg) * (np.bincount(rows, minlength=nu)[:nu, None] if mutation == "reg-times-n" else 1.0)
        with np.errstate(invalid="ignore"):
            g = sparse - W[:, None] * (pi @ Q) - regs * P
        return g, np.zeros(nu)
    reg, reg_b = (hyper[4], hyper[2]) if mutation == "regs-swapped" else (hyper[2], hyper[4])
    P1 = np.concatenate([P, np.ones((nu, 1))], axis=1)
    sparse = np.zeros((ni, f + 1))
    np.add.at(sparse, idx, w[:, None] * P1[rows])
    Pd = P1.copy()
    if mutation == "no-bias-column":
        Pd[:, f] = 0.0
    own = np.concatenate([Q, ib[:, None]], axis=1)
    regs = np.concatenate([np.full(f, float(reg)), [float(reg_b)]])
    if mutation == "reg-times-n":
        regs = regs[None, :] * np.bincount(idx, minlength=ni)[:ni, None]
    with np.errstate(invalid="ignore"):
        g = sparse - (W[:, None] * pi).T @ Pd - regs * own
    return g[:, :f], g[:, f]


def objective(csr, state, gb, hyper):
    """The float64 objective over the rows inside the CSR."""
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in _inside(csr, state))
    S = float(gb) + ub[:, None] + ib[None, :] + P @ Q.T
    l = _lse_rows(S)
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    idx = np.asarray(csr.indices, np.int64)
    w = np.asarray(csr.data, np.float64)
    return float((w * (S[rows, idx] - l[rows])).sum() - 0.5 * (hyper[1] * (P * P).sum() + hyper[2] * (Q * Q).sum() + hyper[4] * (ib * ib).sum()))


# ------------------------------------------------------------------------------------------------------------------------ the bounds

def _terms(csr, state, gb):
    """(S, lse, pi, e, b_lse): the scores, the log-sum-exp, pi, the relative bound e_ui on pi and the bound on lse."""
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in _inside(csr, state))
    f, ni = P.shape[1], len(Q)
    S = float(gb) + ub[:, None] + ib[None, :] + P @ Q.T
    l = _lse_rows(S)
    pi = _pi(S, l)
    ds = (f + 4) * U * (np.abs(P) @ np.abs(Q).T + np.abs(ub)[:, None] + np.abs(ib)[None, :] + abs(float(gb)))
    m = S.max(axis=1)
    M = 5 + (ni + 127) // 128
    dl = (16 + M * (2 + 2 * ULPS)) * U + U * (pi * (m[:, None] - S)).sum(axis=1)
    b_lse = ds.max(axis=1) + dl + 2 * ULPS * U * np.abs(l - m) + U * np.abs(l)
    de = ds + b_lse[:, None] + U * np.abs(S - l[:, None])
    return S, l, pi, np.expm1(de) + 2 * ULPS * U, b_lse


def lse_bound(csr, state, gb):
    return _terms(csr, state, gb)[4]


def mass_bound(csr, state, gb):
    _, _, pi, e, _ = _terms(csr, state, gb)
    return (pi * e).sum(axis=1) + (pi.shape[1] + 8) * U


def bound(csr, state, gb, hyper, side):
    """The entrywise rounding bound of the module docstring -> (bound [n x f], bias bound [n]; the users': zeros)."""
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in _inside(csr, state))
    nu, f = P.shape
    ni = len(Q)
    _, _, pi, e, _ = _terms(csr, state, gb)
    rows = np.repeat(np.arange(nu), np.diff(csr.indptr))
    idx = np.asarray(csr.indices, np.int64)
    w = np.abs(np.asarray(csr.data, np.float64))
    Wabs = np.bincount(rows, weights=w, minlength=nu)[:nu] if len(w) else np.zeros(nu)
    n_u = np.diff(csr.indptr)
    if side == "users":
        sparse = np.zeros((nu, f))
        np.add.at(sparse, rows, w[:, None] * np.abs(Q)[idx])
        dense = Wabs[:, None] * (pi @ np.abs(Q))
        slope = Wabs[:, None] * ((pi * e) @ np.abs(Q))
        b = (ni + n_u + 8)[:, None] * U * (sparse + dense + hyper[1] * np.abs(P)) + slope
        return b, np.zeros(nu)
    P1 = np.concatenate([np.abs(P), np.ones((nu, 1))], axis=1)
    sparse = np.zeros((ni, f + 1))
    np.add.at(sparse, idx, w[:, None] * P1[rows])
    c = Wabs[:, None] * pi
    dense = c.T @ P1
    slope = (c * (e + ((n_u + 1) * U)[:, None])).T @ P1
    own = np.abs(np.concatenate([Q, ib[:, None]], axis=1))
    regs = np.concatenate([np.full(f, float(hyper[2])), [float(hyper[4])]])
    n_i = np.bincount(idx, minlength=ni)[:ni]
    b = (nu + n_i + 8)[:, None] * U * (sparse + dense + regs * own) + slope
    return b[:, :f], b[:, f]


def bias_ratio(got, want, bnd):
    """ratio() where a bound of zero asks for the exact value."""
    got, want, bnd = (np.asarray(a, np.float64) for a in (got, want, bnd))
    exact = bnd == 0
    if (got[exact] != want[exact]).any():
        return np.inf
    return ratio(got[~exact], want[~exact], bnd[~exact])


# ---------------------------------------------------------------------------------------------------- the kernels' order, float32

def _exp_below(x, m):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(x == m, np.float32(1), np.exp((x - m).astype(np.float32))).astype(np.float32)


def _merge(m, l, m2, l2):
    mn = np.fmax(m, m2)
    with np.errstate(invalid="ignore"):
        return mn, ((l * _exp_below(m, mn)).astype(np.float32) + (l2 * _exp_below(m2, mn)).astype(np.float32)).astype(np.float32)


def _acc_row(reg, h):
    return (reg & 3) + 8 * (reg >> 2) + 4 * h


def online_lse_f32(S):
    """softmax_lse_kernel's (m, l) walk over the float32 scores S [own x partners] -> float32 lse."""
    S = np.asarray(S, np.float32)
    n, ni = S.shape
    run = [(np.full(n, -np.inf, np.float32), np.zeros(n, np.float32)) for _ in range(4)]
    for b0 in range(0, ni, 32):
        wave = (b0 // 32) % 4
        pair = []
        for h in (0, 1):
            cols = [b0 + _acc_row(reg, h) for reg in range(16) if b0 + _acc_row(reg, h) < ni]
            m, l = np.full(n, -np.inf, np.float32), np.zeros(n, np.float32)
            for c in cols:
                m = np.fmax(m, S[:, c])
            for c in cols:
                l = (l + _exp_below(S[:, c], m)).astype(np.float32)
            pair.append((m, l))
        ms, ls = _merge(pair[0][0], pair[0][1], pair[1][0], pair[1][1])
        run[wave] = _merge(run[wave][0], run[wave][1], ms, ls)
    m, l = run[0]
    for wv in (1, 2, 3):
        m, l = _merge(m, l, run[wv][0], run[wv][1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (m + np.log(l).astype(np.float32)).astype(np.float32)


def _f32_inside(csr, state):
    return tuple(np.ascontiguousarray(a, np.float32) for a in _inside(csr, state))


def lse_f32(csr, state, gb):
    P, Q, ub, ib = _f32_inside(csr, state)
    return online_lse_f32(scores_f32(P, ub, Q, ib, gb))


def weights_f32(csr):
    """softmax_weights_kernel: the row's values added in entry order."""
    n = csr.rows
    counts = np.diff(csr.indptr)
    W = np.zeros(n, np.float32)
    data = np.asarray(csr.data, np.float32)
    for t in range(int(counts.max()) if n and csr.nnz else 0):
        sel = np.flatnonzero(counts > t)
        W[sel] = W[sel] + data[csr.indptr[sel] + t]
    return W


def _push(coef, Y1):
    """sum over partners of coef[own, partner] Y1[partner], in the second product's order -> [own x (f + 1)]."""
    n, m = coef.shape
    part = np.zeros((4, n, Y1.shape[1]), np.float32)
    for b0 in range(0, m, 32):
        wave = (b0 // 32) % 4
        for o in BLOCK_ORDER:
            if b0 + o < m:
                part[wave] = _fma(coef[:, b0 + o][:, None], Y1[b0 + o][None, :], part[wave])
    return ((part[0] + part[1]) + part[2]) + part[3]


def _entries(indptr, indices, data, Y1, n):
    """sum over the own row's entries of w [y | 1]: group g = position % 4 in ascending order, the groups added in group order."""
    nnz = len(indices)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    pos = np.arange(nnz) - indptr[rows]
    acc = np.zeros((n, 4, Y1.shape[1]), np.float32)
    w = np.asarray(data, np.float32)
    Ye = Y1[indices]
    for t in range(int(pos.max()) // 4 + 1 if nnz else 0):
        sel = np.flatnonzero(pos // 4 == t)
        acc[rows[sel], pos[sel] % 4] = _fma(w[sel][:, None], Ye[sel], acc[rows[sel], pos[sel] % 4])
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def mass_f32(csr, state, gb):
    """Column f of the users' dense pass: sum_i expf(s - lse)."""
    P, Q, ub, ib = _f32_inside(csr, state)
    S = scores_f32(P, ub, Q, ib, gb)
    l = online_lse_f32(S)
    with np.errstate(invalid="ignore", over="ignore"):
        coef = np.exp((S - l[:, None]).astype(np.float32)).astype(np.float32)
    return _push(coef, np.ones((len(Q), 1), np.float32))[:, 0]


def gradient_f32(csr, state, gb, hyper, side):
    """float32 (g, gb) in the kernels' order (module docstring)."""
    P, Q, ub, ib = _f32_inside(csr, state)
    nu, f = P.shape
    ni = len(Q)
    S = scores_f32(P, ub, Q, ib, gb)  # [users x items]; the item side scores the same pairs with the same chain
    l = online_lse_f32(S)
    W = weights_f32(csr)
    with np.errstate(invalid="ignore", over="ignore"):
        pi = np.exp((S - l[:, None]).astype(np.float32)).astype(np.float32)
    if side == "users":
        Q1 = np.concatenate([Q, np.ones((ni, 1), np.float32)], axis=1)
        dense = _push(pi, Q1)
        sparse = _entries(csr.indptr, csr.indices, csr.data, Q1, nu)
        g = (sparse[:, :f] - (W[:, None] * dense[:, :f]).astype(np.float32)) - (np.float32(hyper[1]) * P).astype(np.float32)
        return g.astype(np.float32), np.zeros(nu, np.float32)
    t = csr.transpose()
    P1 = np.concatenate([P, np.ones((nu, 1), np.float32)], axis=1)
    dense = _push(np.ascontiguousarray(((W[:, None] * pi).astype(np.float32)).T), P1)
    sparse = _entries(t.indptr, t.indices, t.data, P1, ni)
    own = np.concatenate([Q, ib[:, None]], axis=1)
    regs = np.concatenate([np.full(f, np.float32(hyper[2])), [np.float32(hyper[4])]]).astype(np.float32)
    g = ((sparse - dense) - (regs * own).astype(np.float32)).astype(np.float32)
    return g[:, :f], g[:, f]


def objective_f32(csr, state, gb, hyper):
    """The objective as cu2rec_model_softmax_objective forms it: lse in float32 (the kernel's walk), everything else in float64."""
    l = lse_f32(csr, state, gb).astype(np.float64)
    P, Q, ub, ib = (a.astype(np.float64) for a in _f32_inside(csr, state))
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    idx = np.asarray(csr.indices, np.int64)
    s_e = ((float(gb) + ub[rows]) + ib[idx]) + np.einsum("ij,ij->i", P[rows], Q[idx])
    w = np.asarray(csr.data, np.float32).astype(np.float64)
    return float((w * (s_e - l[rows])).sum() - 0.5 * (hyper[1] * (P * P).sum() + hyper[2] * (Q * Q).sum() + hyper[4] * (ib * ib).sum()))


def run(csr, state, gb, hyper, sweeps, f32=False):
    """`sweeps` sweeps (users, then items) from `state` with zeroed accumulators -> (state, [objective after every half-step]).
    f32: the float32 restatement (gradient_f32, step_f32) on float32 state; the objectives are float64 values at that state.  The
    user biases are never stepped."""
    dt = np.float32 if f32 else np.float64
    P, Q, ub, ib = (np.array(a, dt) for a in state)
    aP, aQ, aib = (np.zeros_like(a) for a in (P, Q, ib))
    grad, stp = (gradient_f32, step_f32) if f32 else (gradient, step)
    objectives = []
    for _ in range(sweeps):
        g, _ = grad(csr, (P, Q, ub, ib), gb, hyper, "users")
        P[:csr.rows], aP[:csr.rows] = stp(P[:csr.rows], aP[:csr.rows], g, hyper[0])
        objectives.append(objective(csr, (P, Q, ub, ib), gb, hyper))
        g, gbias = grad(csr, (P, Q, ub, ib), gb, hyper, "items")
        Q[:csr.cols], aQ[:csr.cols] = stp(Q[:csr.cols], aQ[:csr.cols], g, hyper[0])
        ib[:csr.cols], aib[:csr.cols] = stp(ib[:csr.cols], aib[:csr.cols], gbias, hyper[0])
        objectives.append(objective(csr, (P, Q, ub, ib), gb, hyper))
    return (P, Q, ub, ib), objectives
