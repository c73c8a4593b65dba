"""TEST INFRASTRUCTURE: implicit-feedback alternating least squares (cu2rec_model_als_implicit) restated with numpy.

The model (include/cu2rec_amd.h, "Implicit feedback"): U = csr.rows, I = csr.cols, every stored entry (u, i, r) an observation of
weight w = alpha r (repeated pairs count separately), s_ui = p_u . q_i, no biases:
    L = 1/2 sum_(u<U, i<I) s_ui^2 + 1/2 sum_entries (w (1 - s_ui)^2 + 1 - 2 s_ui) + 1/2 P_reg sum_(u<U) |p_u|^2
      + 1/2 Q_reg sum_(i<I) |q_i|^2
A user half-step solves, for EVERY u < U with Y = Q[0:I]:
    (Y^T Y + sum_entries w q_i q_i^T + P_reg I_f) p_u = sum_entries (1 + w) q_i
(a user without entries gets the zero row); the item half-step is the mirror image with X = P[0:U] and Q_reg.

half_step() / objective() are float64 from the float32 values as they are (alpha and the regularisers are the float32 values the
kernels see, widened; w is their exact product with r).  solve_rows_f32() restates the device arithmetic in float32 -- G0 summed
tile by tile, a row's Gram chunk by chunk, every sum a chain in entry order, the right-looking Cholesky -- and objective_f32() the
objective with float32 Grams; they run on the CPU only, to show that the GPU test sets are fair and to measure the objective's
tolerance.
csr: anything with indptr / indices / data / rows / cols (api.HostCSR)."""
import numpy as np

STEP, CHUNK, MAX_CHUNKS = 32, 1024, 64  # CU2REC_ALS_STEP, CU2REC_ALS_CHUNK, CU2REC_ALS_MAX_CHUNKS (tests/test_ials_cpu.py pins them)
MUTATIONS = ("n_reg", "no_g0", "gram_1_plus_w", "rhs_w", "tile_pair")
GRAM_BLOCK = 1 << 16  # partner rows widened to float64 at a time by gram64()


def _f32(x):
    return float(np.float32(x))


def own_major(csr, side):
    """(indptr, indices, data, n_partners) as the half-step of `side` reads the entries: the CSR, or its item-major view (an
    item's users ascending, repeats kept)."""
    if side == "users":
        return np.asarray(csr.indptr, np.int64), np.asarray(csr.indices, np.int64), np.asarray(csr.data, np.float64), csr.cols
    rows_of = np.repeat(np.arange(csr.rows, dtype=np.int64), np.diff(csr.indptr))
    order = np.argsort(csr.indices, kind="stable")
    indptr = np.zeros(csr.cols + 1, np.int64)
    np.cumsum(np.bincount(csr.indices, minlength=csr.cols), out=indptr[1:])
    return indptr, rows_of[order], np.asarray(csr.data, np.float64)[order], csr.rows


def ials_tiles(f):
    """32-column tiles of the staged operands: f factor columns and the right-hand side's weight (als.hpp: ials_tiles)."""
    return (f + 1 + 31) // 32


def gram64(X):
    """X^T X in float64, GRAM_BLOCK rows at a time: a float32 X of many rows is never widened as a whole."""
    f = X.shape[1]
    G = np.zeros((f, f))
    for lo in range(0, len(X), GRAM_BLOCK):
        B = np.asarray(X[lo:lo + GRAM_BLOCK], np.float64)
        G += B.T @ B
    return G


def row_system(indptr, indices, data, X, reg, alpha, r, G0, mutation=None):
    """(A, b) of row r in float64: A = G0 + sum w q q^T + reg I, b = sum (1 + w) q; `mutation` as in solve_rows."""
    f = X.shape[1]
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    Z = np.asarray(X[indices[lo:hi]], np.float64)
    w = _f32(alpha) * np.asarray(data[lo:hi], np.float64)
    gw = 1.0 + w if mutation == "gram_1_plus_w" else w
    bw = w if mutation == "rhs_w" else 1.0 + w
    W, b = (Z * gw[:, None]).T @ Z, Z.T @ bw
    if mutation == "tile_pair":
        nt = ials_tiles(f)
        r0 = 32 * (nt - 1)
        if nt == 1:
            block = (slice(0, f), slice(0, f))
        else:
            block = (slice(r0, f), slice(0, 32))
        if W[block].size and W[block].any():
            W[block] = 0.0
            W[block[1], block[0]] = 0.0
        else:
            b[:32] = 0.0
    return G0 + W + (hi - lo if mutation == "n_reg" else 1) * _f32(reg) * np.eye(f), b


def solve_rows(indptr, indices, data, X, reg, alpha, rows=None, mutation=None, G0=None):
    """Rows `rows` (default: all) of one half-step in float64 against the partner rows X (all of them enter G0) -> (len(rows), f).
    G0: X^T X in float64 where the caller has it already (gram64).
    mutation: one of MUTATIONS -- the five deliberate mistakes the tests must be able to see: "n_reg" (n reg on the diagonal, the
    explicit objective's regulariser), "no_g0" (the all-pairs Gram left out), "gram_1_plus_w" (weights 1 + w in the Gram),
    "rhs_w" (the right-hand side weighted by w), and "tile_pair", an error confined to ONE accumulator of the kernel: of the
    row's own sums [sum w q q^T ; sum (1 + w) q] (row f is the right-hand side, as in als.hip) tile pair (NT - 1, 0) -- rows
    32 (NT - 1) .. and columns 0 .. 31 -- holds the Gram block of rows 32 (NT - 1) .. f - 1, which is zeroed (with its mirror
    image: the kernel reads the lower triangle of a symmetric system); at NT = 1 the whole own Gram is.  Where that changes
    nothing -- f a multiple of 32: the last tile holds no Gram row; alpha = 0: the own Gram is zero -- the other thing the same
    accumulator holds, the right-hand side's entries 0 .. 31, is zeroed instead."""
    assert mutation is None or mutation in MUTATIONS
    f = X.shape[1]
    if mutation == "no_g0":
        G0 = np.zeros((f, f))
    elif G0 is None:
        G0 = gram64(X)
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, np.int64)
    out = np.zeros((len(rows), f))
    for k, r in enumerate(rows):
        if indptr[r + 1] == indptr[r]:
            continue
        out[k] = np.linalg.solve(*row_system(indptr, indices, data, X, reg, alpha, r, G0, mutation))
    return out


def half_step(csr, P, Q, hyper, alpha, side):
    """One half-step from the given values -> float64 (P, Q): the rows of the side inside the CSR solved, everything else as it
    is.  hyper: (lr, P_reg, Q_reg, user_bias_reg, item_bias_reg), of which P_reg / Q_reg are read."""
    P, Q = np.array(P, np.float64), np.array(Q, np.float64)
    indptr, indices, data, n_part = own_major(csr, side)
    if side == "users":
        P[:csr.rows] = solve_rows(indptr, indices, data, Q[:n_part], hyper[1], alpha)
    else:
        Q[:csr.cols] = solve_rows(indptr, indices, data, P[:n_part], hyper[2], alpha)
    return P, Q


def _entries(csr, P, Q):
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    return np.einsum("ij,ij->i", P[users], Q[np.asarray(csr.indices, np.int64)])


def objective(csr, P, Q, hyper, alpha):
    """L in float64, term by term as written above (the all-pairs term through the two f x f Grams: the same number)."""
    P, Q = np.asarray(P, np.float64)[:csr.rows], np.asarray(Q, np.float64)[:csr.cols]
    s = _entries(csr, P, Q)
    w = _f32(alpha) * np.asarray(csr.data, np.float64)
    return 0.5 * (np.sum((P.T @ P) * (Q.T @ Q)) + np.sum(w * (1.0 - s) ** 2 + 1.0 - 2.0 * s)
                  + _f32(hyper[1]) * np.sum(P * P) + _f32(hyper[2]) * np.sum(Q * Q))


def run(csr, P, Q, hyper, alpha, sweeps):
    """`sweeps` sweeps (users, then items) in float64 -> [(P, Q) after every half-step], the initial state first."""
    states = [(np.array(P, np.float64), np.array(Q, np.float64))]
    for _ in range(sweeps):
        for side in ("users", "items"):
            states.append(half_step(csr, *states[-1], hyper, alpha, side))
    return states


# ---- the device arithmetic restated in float32 -------------------------------------------------------------------------------
def _chain(acc, A, B):
    """acc += sum_k A[k]^T B[k] in float32, one entry after the other in k order: the matrix cores' accumulation (there each
    step is one fused multiply-add; here the product is rounded first)."""
    for k in range(len(A)):
        acc += np.outer(A[k], B[k])
    return acc


def _chain_vec(A, z):
    """sum_k z[k] A[k] in float32 in k order (the right-hand side: row f of the same product)."""
    return np.add.accumulate(A * z[:, None], axis=0, dtype=np.float32)[-1]


def gram_f32(X):
    """X^T X in float32 as the G0 kernels form it: per tile of CHUNK rows a chain from zero, the tiles added in tile order."""
    X = np.asarray(X, np.float32)
    G = np.zeros((X.shape[1], X.shape[1]), np.float32)
    for t in range(0, len(X), CHUNK):
        G += _chain(np.zeros_like(G), X[t:t + CHUNK], X[t:t + CHUNK])
    return G


def chunk_len(n):
    c = min(-(-n // CHUNK), MAX_CHUNKS)
    return -(-(-(-n // c)) // STEP) * STEP


def cholesky_solve_f32(G, b):
    """G x = b by the kernel's right-looking Cholesky without pivoting and both substitutions, float32; None where a pivot is not
    a finite positive float or the solution is not finite."""
    G, y = np.array(G, np.float32), np.array(b, np.float32)
    for k in range(len(y)):
        d = G[k, k]
        if not (d > 0 and np.isfinite(d)):
            return None
        l = np.sqrt(d)
        G[k, k] = l
        G[k + 1:, k] /= l
        y[k] /= l
        G[k + 1:, k + 1:] -= np.outer(G[k + 1:, k], G[k + 1:, k])
        y[k + 1:] -= G[k + 1:, k] * y[k]
    for k in range(len(y) - 1, -1, -1):
        y[k] /= G[k, k]
        y[:k] -= G[k, :k] * y[k]
    return y if np.isfinite(y).all() else None


def solve_rows_f32(indptr, indices, data, X, reg, alpha, rows=None, G0=None):
    """solve_rows() in float32, in the kernels' order: G0 by gram_f32 (or as given: gram_f32(X) computed before); a row of at
    most CHUNK entries adds (w q) q^T and (1 + w) q to G0 entry by entry; a longer row is cut into chunks whose sums, each from
    zero, are added to G0 in chunk order; reg on the diagonal; cholesky_solve_f32.  A row that cannot be solved comes back as NaN."""
    F = np.float32
    X = np.asarray(X, F)
    f = X.shape[1]
    G0 = gram_f32(X) if G0 is None else np.asarray(G0, F)
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, np.int64)
    out = np.zeros((len(rows), f), F)
    for k, r in enumerate(rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        n = hi - lo
        if n == 0:
            continue
        Z = X[indices[lo:hi]]
        w = F(alpha) * np.asarray(data[lo:hi], F)
        A, ones = Z * w[:, None], F(1) + w
        if n <= CHUNK:  # one chain that starts from G0
            G, b = _chain(G0.copy(), A, Z), _chain_vec(Z, ones)
        else:  # the chunks' chains start from zero and are added to G0 in chunk order
            G, b, cut = G0.copy(), np.zeros(f, F), chunk_len(n)
            for c in range(0, n, cut):
                G += _chain(np.zeros_like(G0), A[c:c + cut], Z[c:c + cut])
                b += _chain_vec(Z[c:c + cut], ones[c:c + cut])
        G[np.diag_indices(f)] += F(reg)
        x = cholesky_solve_f32(G, b)
        out[k] = np.nan if x is None else x
    return out


def objective_f32(csr, P, Q, hyper, alpha):
    """The objective as cu2rec_model_implicit_objective forms it: the two Grams in float32 (gram_f32), their inner product, the
    entries term (w rounded to float32) and the norms in float64."""
    P, Q = np.asarray(P, np.float32)[:csr.rows], np.asarray(Q, np.float32)[:csr.cols]
    s = _entries(csr, P.astype(np.float64), Q.astype(np.float64))
    w = (np.float32(alpha) * np.asarray(csr.data, np.float32)).astype(np.float64)
    gram = np.sum(gram_f32(P).astype(np.float64) * gram_f32(Q).astype(np.float64))
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    return 0.5 * (gram + np.sum(w * (1.0 - s) ** 2 + 1.0 - 2.0 * s) + _f32(hyper[1]) * np.sum(P * P) + _f32(hyper[2]) * np.sum(Q * Q))
