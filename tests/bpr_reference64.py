"""TEST INFRASTRUCTURE: Bayesian Personalized Ranking (cu2rec_model_bpr, include/cu2rec_amd.h) restated with numpy.

negatives(): every draw from api.sampler_index (the library's host copy of the kernels' sampler), the membership test a Python set.
float64: gradient(), objective(), run() -- the judge; lmf_reference64's sigma, softplus and step().  float32: gradient_f32() restates
csrc/bpr.hip operation by operation in its order -- the difference q_i - q_j rounded once, the dot product as 16 lanes' fused
multiply-add chains over their columns (4 l .. 4 l + 3, + 64 k) folded by the butterfly 8, 4, 2, 1, the score (ib_i - ib_j) + dot,
an entry's term added by fused multiply-add to the sum of group (position mod 4) in ascending position (on the item side the
positives in item-major position, then the negatives in ascending entry, the groups counted from each list's start), the four
groups added in order, reg x subtracted as a product and a difference.  The device's expf is not numpy's: a restatement, not a
bit-for-bit prediction.

bound(): entrywise on |g - g*| for any float32 evaluation in any order.  u = 2^-24, f factors, K = the own row's terms:
  * x_e is f differences, f products and sums and two bias operations: |x^ - x| <= (f + 4) u (|p| . (|q_i| + |q_j|) + |ib_i| + |ib_j|)
    =: dx;  sigma' <= 1/4, so c_e = sigma(-x_e) moves by at most dx / 4;
  * sigma itself, the difference and the product with c are a handful of roundings, the sum of K terms in any order gamma_K times the
    sum of the absolute terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5), the regulariser's product
    and difference a few more: (K + 8) u times the absolute terms.
  users: bound = (K + 8) u (sum c_e (|q_i| + |q_j|) + P_reg |p_u|) + sum dx_e / 4 (|q_i| + |q_j|); the bias' gradient is exactly 0.
  items: bound = (K + 8) u (sum_(pos, neg) c_e |p_u| + Q_reg |q_i|) + sum_(pos, neg) dx_e / 4 |p_u|, the bias' with |p_u| -> 1."""
import numpy as np

from cu2rec_amd import api

from lmf_reference64 import U, ratio, sigma, sigma_f32, softplus, step, step_f32, _fma  # noqa: F401 (re-exported)

ATTEMPTS = 8
MAX_SWEEP = 1 << 29

NEGATIVE_MUTATIONS = ("stored-accepted", "failed-counted")
MUTATIONS = NEGATIVE_MUTATIONS + ("sigma-x", "neg-dropped", "neg-sign", "no-item-bias", "drop-last-entry", "repeats-once", "regs-swapped",
                                  "reg-times-n")

_NEG = {}


def negatives(csr, seed, sweep, mutation=None):
    """int32 [nnz]: the negative of every entry in sweep `sweep`, -1 where all ATTEMPTS draws were items the row stores.  Cached per
    (csr, seed, sweep, mutation); the CSR is kept alive by the cache.  mutation: "stored-accepted" takes the first draw whatever it
    is, "failed-counted" keeps the last draw where every attempt failed."""
    key = (id(csr), int(seed), int(sweep), mutation)
    if key in _NEG:
        return _NEG[key][1]
    assert 0 <= sweep < MAX_SWEEP
    draw = api.sampler_index
    indptr, indices, cols = csr.indptr, csr.indices, int(csr.cols)
    neg = np.full(csr.nnz, -1, np.int32)
    for u in range(csr.rows):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        stored = set(indices[lo:hi].tolist())
        for k in range(hi - lo):
            for a in range(ATTEMPTS):
                j = draw(seed, u, ((sweep * ATTEMPTS + a) << 32) | k, 0, cols)
                if j not in stored or mutation == "stored-accepted":
                    neg[lo + k] = j
                    break
            else:
                if mutation == "failed-counted":
                    neg[lo + k] = j
    _NEG[key] = (csr, neg)
    return neg


def _entries(csr, neg, mutation):
    """(rows, items, negatives, on): the entries and which of them have a triple."""
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    items = np.asarray(csr.indices, np.int64)
    on = np.asarray(neg) >= 0
    if mutation == "repeats-once":
        _, first = np.unique(rows * (csr.cols + 1) + items, return_index=True)
        keep = np.zeros(len(items), bool)
        keep[first] = True
        on = on & keep
    return rows, items, np.where(np.asarray(neg) >= 0, neg, 0).astype(np.int64), on


def _last_of_own_rows(csr, side):
    """The user-major position of the last entry of every non-empty own row (a user's last entry; an item's last positive)."""
    if side == "users":
        ends = np.asarray(csr.indptr[1:], np.int64) - 1
        return ends[np.diff(csr.indptr) > 0]
    order = np.argsort(csr.indices, kind="stable")
    counts = np.bincount(csr.indices, minlength=csr.cols)
    ends = np.cumsum(counts) - 1
    return order[ends[counts > 0]]


def scores(csr, state, neg, mutation=None):
    """float64 x_e of every entry (arbitrary where the entry has no triple)."""
    P, Q, _, ib = (np.asarray(a, np.float64) for a in state)
    rows, items, negs, _ = _entries(csr, neg, None)
    x = np.einsum("ij,ij->i", P[rows], Q[items] - Q[negs])
    return x if mutation == "no-item-bias" else (ib[items] - ib[negs]) + x


def gradient(csr, state, hyper, neg, side, mutation=None):
    """float64 (g [n x f], gb [n]) of every own row inside the CSR.  mutation: one of MUTATIONS past the first two (those change
    `neg`), a deliberate mistake."""
    P, Q, _, ib = (np.asarray(a, np.float64) for a in state)
    P, Q, ib = P[:csr.rows], Q[:csr.cols], ib[:csr.cols]
    _, P_reg, Q_reg, _, ib_reg = (float(np.float32(h)) for h in hyper)
    if mutation == "regs-swapped":
        P_reg, Q_reg = Q_reg, P_reg
    rows, items, negs, on = _entries(csr, neg, mutation)
    x = scores(csr, state, neg, mutation)
    c = np.where(on, sigma(x) if mutation == "sigma-x" else sigma(-x), 0.0)
    if mutation == "drop-last-entry":
        c[_last_of_own_rows(csr, side)] = 0.0
    f = P.shape[1]
    if side == "users":
        g = np.zeros((csr.rows, f))
        np.add.at(g, rows, c[:, None] * (Q[items] - Q[negs]))
        reg = P_reg * (np.diff(csr.indptr)[:, None] if mutation == "reg-times-n" else 1.0)
        return g - reg * P, np.zeros(csr.rows)
    g = np.zeros((csr.cols, f + 1))
    P1 = np.concatenate([P, np.ones((csr.rows, 1))], axis=1)
    np.add.at(g, items, c[:, None] * P1[rows])
    if mutation != "neg-dropped":
        np.add.at(g, negs, (c if mutation == "neg-sign" else -c)[:, None] * P1[rows])
    n = np.bincount(csr.indices, minlength=csr.cols).astype(np.float64) if mutation == "reg-times-n" else np.ones(csr.cols)
    return g[:, :f] - (Q_reg * n)[:, None] * Q, g[:, f] - ib_reg * n * ib


def bound(csr, state, hyper, neg, side):
    """The entrywise rounding bound of the module docstring -> (bound [n x f], bias bound [n])."""
    P, Q, _, ib = (np.asarray(a, np.float64) for a in state)
    P, Q, ib = P[:csr.rows], Q[:csr.cols], ib[:csr.cols]
    _, P_reg, Q_reg, _, ib_reg = (float(np.float32(h)) for h in hyper)
    rows, items, negs, on = _entries(csr, neg, None)
    f = P.shape[1]
    c = np.where(on, sigma(-scores(csr, state, neg)), 0.0)
    aq = np.abs(Q[items]) + np.abs(Q[negs])
    dx = np.where(on, (f + 4) * U * (np.einsum("ij,ij->i", np.abs(P[rows]), aq) + np.abs(ib[items]) + np.abs(ib[negs])), 0.0)
    if side == "users":
        absterms, slope = np.zeros((csr.rows, f)), np.zeros((csr.rows, f))
        np.add.at(absterms, rows, c[:, None] * aq)
        np.add.at(slope, rows, (0.25 * dx)[:, None] * aq)
        K = np.diff(csr.indptr)
        return (K + 8)[:, None] * U * (absterms + P_reg * np.abs(P)) + slope, np.zeros(csr.rows)
    P1 = np.concatenate([np.abs(P), np.ones((csr.rows, 1))], axis=1)
    absterms, slope = np.zeros((csr.cols, f + 1)), np.zeros((csr.cols, f + 1))
    for idx in (items, negs):
        np.add.at(absterms, idx, c[:, None] * P1[rows])
        np.add.at(slope, idx, (0.25 * dx)[:, None] * P1[rows])
    K = np.bincount(items, minlength=csr.cols) + np.bincount(negs[on], minlength=csr.cols)
    own = np.abs(np.concatenate([Q, ib[:, None]], axis=1))
    regs = np.concatenate([np.full(f, Q_reg), [ib_reg]])
    b = (K + 8)[:, None] * U * (absterms + regs * own) + slope
    return b[:, :f], b[:, f]


def objective(csr, state, hyper, neg):
    """float64 (L, triples, triples with x_e > 0) over the rows inside the CSR."""
    P, Q, _, ib = (np.asarray(a, np.float64) for a in state)
    P, Q, ib = P[:csr.rows], Q[:csr.cols], ib[:csr.cols]
    x = scores(csr, state, neg)[np.asarray(neg) >= 0]
    P_reg, Q_reg, ib_reg = (float(np.float32(hyper[k])) for k in (1, 2, 4))  # as cu2rec_hyper holds them
    L = -softplus(-x).sum() - 0.5 * (P_reg * (P * P).sum() + Q_reg * (Q * Q).sum() + ib_reg * (ib * ib).sum())
    return float(L), int(len(x)), int((x > 0).sum())


# ---------------------------------------------------------------------------------------------------- the kernels' order

def _group_sums(acc, own, pos, c, Y):
    """acc[own row][position mod 4] = fma(c, Y, acc), the entries of every own row in ascending position (pos), all rows at once."""
    for t in range(int(pos.max()) // 4 + 1 if len(pos) else 0):
        sel = np.flatnonzero((pos // 4 == t) & np.isfinite(c))
        acc[own[sel], pos[sel] % 4] = _fma(c[sel][:, None], Y[sel], acc[own[sel], pos[sel] % 4])


def coefficients_f32(csr, state, neg):
    """float32 (c_e, q_i - q_j) as bpr_user_kernel forms them; c_e is NaN where the entry has no triple."""
    P, Q, _, ib = (np.ascontiguousarray(a, np.float32) for a in state)
    rows, items, negs, on = _entries(csr, neg, None)
    f = P.shape[1]
    E = (f + 1 + 63) // 64
    diff = Q[items] - Q[negs]
    q = np.zeros((len(items), 64 * E), np.float32)
    q[:, :f] = diff
    v = np.zeros((len(items), 64 * E), np.float32)
    v[:, :f] = P[rows]
    q, v = q.reshape(-1, E, 16, 4), v.reshape(-1, E, 16, 4)
    d = np.zeros((len(items), 16), np.float32)
    for k in range(E):
        for comp in range(4):
            d = _fma(q[:, k, :, comp], v[:, k, :, comp], d)
    lanes = np.arange(16)
    for mask in (8, 4, 2, 1):
        d = d + d[:, lanes ^ mask]
    x = (ib[items] - ib[negs]) + d[:, 0]
    return np.where(on, sigma_f32(-x), np.float32(np.nan)).astype(np.float32), diff


def gradient_f32(csr, state, hyper, neg, side):
    """float32 (g, gb) in the kernels' order (module docstring)."""
    P, Q, _, ib = (np.ascontiguousarray(a, np.float32) for a in state)
    P, Q, ib = P[:csr.rows], Q[:csr.cols], ib[:csr.cols]
    _, P_reg, Q_reg, _, ib_reg = (np.float32(h) for h in hyper)
    rows, items, negs, on = _entries(csr, neg, None)
    c, diff = coefficients_f32(csr, state, neg)
    f = P.shape[1]
    if side == "users":
        acc = np.zeros((csr.rows, 4, f), np.float32)
        _group_sums(acc, rows, np.arange(csr.nnz) - np.asarray(csr.indptr, np.int64)[rows], c, diff)
        g = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
        return g - P_reg * P, np.zeros(csr.rows, np.float32)
    P1 = np.concatenate([P, np.ones((csr.rows, 1), np.float32)], axis=1)
    acc = np.zeros((csr.cols, 4, f + 1), np.float32)
    order = np.argsort(items, kind="stable")  # the item-major view: an item's entries in ascending e
    starts = np.concatenate([[0], np.cumsum(np.bincount(items, minlength=csr.cols))])
    _group_sums(acc, items[order], np.arange(csr.nnz) - starts[items[order]], c[order], P1[rows[order]])
    key = np.where(on, negs, csr.cols)
    order = np.argsort(key, kind="stable")[:int(on.sum())]  # by (j_e, e), the entries without a triple past the end
    starts = np.concatenate([[0], np.cumsum(np.bincount(negs[on], minlength=csr.cols))])
    _group_sums(acc, negs[order], np.arange(len(order)) - starts[negs[order]], -c[order], P1[rows[order]])
    g = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    own = np.concatenate([Q, ib[:, None]], axis=1)
    regs = np.concatenate([np.full(f, Q_reg), [ib_reg]]).astype(np.float32)
    g = g - regs * own
    return g[:, :f], g[:, f]


def objective_blocked(csr, state, hyper, neg, threads=256, group=16, max_blocks=4096):
    """The objective as cu2rec_model_bpr_objective adds it up, all in float64: a dot product as 16 lanes' sums over their columns
    folded by the butterfly, entry e and row r dealt to group e mod (16 blocks), a group's terms added in ascending order, a
    workgroup's 256 threads by a tree of halves, the workgroups in order -> L."""
    P, Q, _, ib = (np.asarray(a, np.float64) for a in state)
    P, Q, ib = P[:csr.rows], Q[:csr.cols], ib[:csr.cols]
    rows, items, negs, on = _entries(csr, neg, None)
    f = P.shape[1]
    pad = -f % 64

    def dot(A, B):
        prod = np.pad(A * B, ((0, 0), (0, pad))).reshape(len(A), -1, 16, 4)
        d = np.zeros((len(A), 16))
        for k in range(prod.shape[1]):
            for comp in range(4):
                d = d + prod[:, k, :, comp]
        for mask in (8, 4, 2, 1):
            d = d + d[:, np.arange(16) ^ mask]
        return d[:, 0]

    work = max(csr.nnz, csr.rows, csr.cols)
    per_block = (threads // group) * 8
    blocks = min(max((work + per_block - 1) // per_block, 1), max_blocks)
    groups = blocks * (threads // group)

    def dealt(terms, index):
        s = np.zeros(groups)
        for t in range((int(index.max()) // groups + 1) if len(index) else 0):
            sel = index // groups == t
            s[index[sel] % groups] += terms[sel]
        red = np.zeros((blocks, threads))
        red[:, ::group] = s.reshape(blocks, threads // group)
        stride = threads // 2
        while stride:
            red[:, :stride] += red[:, stride:2 * stride]
            stride //= 2
        total = 0.0
        for b in range(blocks):
            total += red[b, 0]
        return total

    e = np.flatnonzero(on)
    x = (ib[items[e]] - ib[negs[e]]) + (dot(P[rows[e]], Q[items[e]]) - dot(P[rows[e]], Q[negs[e]]))
    s0 = dealt(-softplus(-x), e)
    s1 = dealt(dot(P, P), np.arange(csr.rows))
    s2 = dealt(dot(Q, Q), np.arange(csr.cols))
    s3 = dealt(ib * ib, np.arange(csr.cols))
    P_reg, Q_reg, ib_reg = (float(np.float32(hyper[k])) for k in (1, 2, 4))
    return s0 - 0.5 * (P_reg * s1 + Q_reg * s2 + ib_reg * s3)


def run(csr, state, hyper, seed, sweeps, f32=False, sweep0=0):
    """`sweeps` sweeps (users, then items) from `state` with zeroed accumulators -> (state, [(L, triples, ordered) after every
    half-step, over that sweep's triples]).  f32: the float32 restatement (gradient_f32, step_f32) on float32 state; the objectives are
    float64 values at that state.  User biases never move."""
    dt = np.float32 if f32 else np.float64
    P, Q, ub, ib = (np.array(a, dt) for a in state)
    aP, aQ, aib = (np.zeros_like(a) for a in (P, Q, ib))
    grad, stp = (gradient_f32, step_f32) if f32 else (gradient, step)
    lr = float(np.float32(hyper[0]))
    objectives = []
    for t in range(sweep0, sweep0 + sweeps):
        neg = negatives(csr, seed, t)
        g, _ = grad(csr, (P, Q, ub, ib), hyper, neg, "users")
        P[:csr.rows], aP[:csr.rows] = stp(P[:csr.rows], aP[:csr.rows], g, lr)
        objectives.append(objective(csr, (P, Q, ub, ib), hyper, neg))
        g, gbias = grad(csr, (P, Q, ub, ib), hyper, neg, "items")
        Q[:csr.cols], aQ[:csr.cols] = stp(Q[:csr.cols], aQ[:csr.cols], g, lr)
        ib[:csr.cols], aib[:csr.cols] = stp(ib[:csr.cols], aib[:csr.cols], gbias, lr)
        objectives.append(objective(csr, (P, Q, ub, ib), hyper, neg))
    return (P, Q, ub, ib), objectives
