"""Python mirror of the reference's host interface for the hot path, on top of the C ABI.

Names follow the reference (matrix_factorization/): readCSV, createSparseMatrix,
initialize_normal_array, writeToFile, Config.read_config, train(), calculate_loss_gpu /
get_error_metrics_gpu, sgd_update -- same argument meaning and error behaviour, numpy arrays in
place of raw host pointers.  All GPU work happens inside libcu2rec_amd.so.
"""
import ctypes as C
import os

import numpy as np

from ._lib import Config, Cu2recError, Hyper, RankMetrics, SlimReport, SvdReport, TrainStats, check, lib

SGD_HOGWILD, SGD_SERIAL, SGD_ORDERED, SGD_PINGPONG, SGD_BLOCKSOLVE = 0, 1, 2, 3, 4
ALS = 5  # alternating least squares: a training method of train() / cu2rec_train only (Model.sgd refuses it)
# length thresholds of the ALS half-step (include/cu2rec_amd.h, CU2REC_ALS_*): ratings staged per step, the longest row one
# workgroup solves alone, the most chunks a long row is cut into, and the bound of the partial-Gram workspace in bytes
ALS_MAX_FACTORS, ALS_STEP, ALS_CHUNK, ALS_MAX_CHUNKS, ALS_WORKSPACE_BYTES = 252, 32, 1024, 64, 64 << 20
SIDE_USERS, SIDE_ITEMS = 0, 1
SIM_DOT, SIM_COSINE = 0, 1
SIDES = {"users": SIDE_USERS, "items": SIDE_ITEMS}
METRICS = {"dot": SIM_DOT, "cosine": SIM_COSINE}
MODES = {"hogwild": SGD_HOGWILD, "serial": SGD_SERIAL, "ordered": SGD_ORDERED, "pingpong": SGD_PINGPONG,
         "blocksolve": SGD_BLOCKSOLVE, "als": ALS}
KNN_COUNT, KNN_COSINE, KNN_TFIDF, KNN_BM25 = 0, 1, 2, 3
KNN_WEIGHTINGS = {"count": KNN_COUNT, "cosine": KNN_COSINE, "tfidf": KNN_TFIDF, "bm25": KNN_BM25}
KNN_WORKSPACE_BYTES = 64 << 20  # CU2REC_KNN_WORKSPACE_BYTES: the bound of the product's workspace per batch of queries
EASE_MAX_ITEMS, EASE_MAX_K = 65536, 256  # CU2REC_EASE_MAX_ITEMS, CU2REC_EASE_MAX_K
EASE_WORKSPACE_BYTES = 64 << 20  # CU2REC_EASE_WORKSPACE_BYTES: the bound of the lists' workspace per batch of queries
ALS_SIDES = {"users": (SIDE_USERS,), "items": (SIDE_ITEMS,), "both": (SIDE_USERS, SIDE_ITEMS)}
IALS_SOLVERS = ("cholesky", "cg")  # Model.als / Model.ials / train(mode="als" | "ials"): the exact solver, or conjugate-gradient steps per row
ALS_CG_MAX_STEPS = 256             # CU2REC_ALS_CG_MAX_STEPS


def _mode(mode):
    return MODES[mode] if isinstance(mode, str) else int(mode)


def _solver(solver):
    if solver not in IALS_SOLVERS:
        raise ValueError("solver must be one of %s, not %r" % (list(IALS_SOLVERS), solver))


def _hyper(hyper):
    """Hyper, or (learning_rate, P_reg, Q_reg, user_bias_reg, item_bias_reg) -> Hyper."""
    return hyper if isinstance(hyper, Hyper) else Hyper(*[float(x) for x in hyper])


def _half_steps(side, sweeps, call, numbered=False):
    """`sweeps` times over the half-steps of side "users", "items" or "both" (users, then items): call(side code, byref(count))
    is one library call's status -- numbered: call(side code, byref(count), k), k = 0 .. sweeps - 1 the sweep; returns the counts
    summed."""
    if side not in ALS_SIDES:
        raise ValueError("side must be one of %s, not %r" % (sorted(ALS_SIDES), side))
    total = 0
    for k in range(int(sweeps)):
        for s in ALS_SIDES[side]:
            n = C.c_int()
            check(call(s, C.byref(n), k) if numbered else call(s, C.byref(n)))
            total += n.value
    return total


def _choice(table, value, what):
    if not isinstance(value, str):
        return int(value)
    if value not in table:
        raise ValueError("%s must be one of %s, not %r" % (what, sorted(table), value))
    return table[value]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return a


# ------------------------------------------------------------------------------------------ config

def default_config(**overrides):
    cfg = Config()
    check(lib().cu2rec_config_default(C.byref(cfg)))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError("Config has no field " + k)
        setattr(cfg, k, v)
    return cfg


def read_config(path, cfg=None):
    """Config::read_config (config.cu:7-13)."""
    cfg = cfg or default_config()
    check(lib().cu2rec_config_read(os.fsencode(path), C.byref(cfg)))
    return cfg


def write_config(path, cfg):
    """Config::write_config (config.cu:15-22)."""
    check(lib().cu2rec_config_write(os.fsencode(path), C.byref(cfg)))


def print_config(cfg):
    check(lib().cu2rec_config_print(C.byref(cfg)))


# ------------------------------------------------------------------------------------------ host data

class Ratings:
    """std::vector<Rating> of readCSV: 0-based user / item ids and ratings, plus rows, cols, global_bias."""

    def __init__(self, user, item, rating, rows, cols, global_bias):
        self.user, self.item, self.rating = user, item, rating
        self.rows, self.cols, self.global_bias = rows, cols, global_bias

    def __len__(self):
        return len(self.user)


class HostCSR:
    """Host CSR in the reference layout (matrix.h:11-19)."""

    def __init__(self, indptr, indices, data, rows, cols, global_bias=0.0):
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        self.rows, self.cols, self.nnz = int(rows), int(cols), int(self.indices.shape[0])
        self.global_bias = float(np.float32(global_bias))
        if self.indptr.shape[0] != self.rows + 1:
            raise ValueError("indptr must have rows + 1 entries")

    def slice_users(self, u0, u1):
        """Rows [u0, u1) as their own CSR (user-sharding; item ids unchanged)."""
        out = np.empty(u1 - u0 + 1, np.int32)
        off, nnz = C.c_int(), C.c_int()
        check(lib().cu2rec_csr_slice(_ptr(self.indptr), self.rows, u0, u1, _ptr(out), C.byref(off), C.byref(nnz)))
        return HostCSR(out, self.indices[off.value:off.value + nnz.value], self.data[off.value:off.value + nnz.value],
                       u1 - u0, self.cols, self.global_bias)

    def transpose(self):
        """The column-major view as its own CSR: row i holds the rows that name column i (for a rating matrix, the users of
        item i -- Model.top_users' exclusion), in ascending row order, repeats kept, data carried along."""
        rows_of = np.repeat(np.arange(self.rows, dtype=np.int32), np.diff(self.indptr))
        order = np.argsort(self.indices, kind="stable")
        indptr = np.zeros(self.cols + 1, np.int64)
        np.cumsum(np.bincount(self.indices, minlength=self.cols), out=indptr[1:])
        return HostCSR(indptr, rows_of[order], self.data[order], self.cols, self.rows, self.global_bias)


def readCSV(path):
    """readCSV (util.cu:17-45) -> Ratings.  Raises Cu2recError(CU2REC_EIO) if the file cannot be opened."""
    h = C.c_void_p()
    check(lib().cu2rec_ratings_read_csv(os.fsencode(path), C.byref(h)))
    try:
        n, rows, cols, gb = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        check(lib().cu2rec_ratings_info(h, C.byref(n), C.byref(rows), C.byref(cols), C.byref(gb)))
        pu, pi, pr = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
        check(lib().cu2rec_ratings_view(h, C.byref(pu), C.byref(pi), C.byref(pr)))
        if n.value:
            user = np.ctypeslib.as_array(pu, (n.value,)).copy()
            item = np.ctypeslib.as_array(pi, (n.value,)).copy()
            rating = np.ctypeslib.as_array(pr, (n.value,)).copy()
        else:
            user, item, rating = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
        return Ratings(user, item, rating, rows.value, cols.value, gb.value)
    finally:
        lib().cu2rec_ratings_free(h)


def createSparseMatrix(path_or_ratings, rows=None):
    """readCSV + createSparseMatrix's host half (util.cu:152-179) -> HostCSR."""
    if isinstance(path_or_ratings, Ratings):
        r = path_or_ratings
        # rebuild through the library from the COO arrays (same code path as a file)
        return _csr_from_coo(r.user, r.item, r.rating, rows if rows is not None else r.rows, r.cols, r.global_bias)
    h = C.c_void_p()
    check(lib().cu2rec_ratings_read_csv(os.fsencode(path_or_ratings), C.byref(h)))
    try:
        n, nrows, cols, gb = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        check(lib().cu2rec_ratings_info(h, C.byref(n), C.byref(nrows), C.byref(cols), C.byref(gb)))
        R = nrows.value if rows is None else rows
        indptr = np.zeros(R + 1, np.int32)
        indices = np.zeros(n.value, np.int32)
        data = np.zeros(n.value, np.float32)
        check(lib().cu2rec_csr_build(h, R, _ptr(indptr), _ptr(indices), _ptr(data)))
        return HostCSR(indptr, indices, data, R, cols.value, gb.value)
    finally:
        lib().cu2rec_ratings_free(h)


def _csr_from_coo(user, item, rating, rows, cols, global_bias):
    user = np.asarray(user, np.int64)
    if len(user) and np.any(np.diff(user) < 0):
        raise Cu2recError(-1, "ratings must be sorted by userId")
    counts = np.bincount(user, minlength=rows) if len(user) else np.zeros(rows, np.int64)
    indptr = np.zeros(rows + 1, np.int32)
    np.cumsum(counts, out=indptr[1:])
    return HostCSR(indptr, np.asarray(item, np.int32), np.asarray(rating, np.float32), rows, cols, global_bias)


def initialize_normal_array(size, n_factors, mean=0.0, stddev=1.0, seed=42):
    """initialize_normal_array (util.cu:124-144): mt19937(seed), normal(mean, stddev / n_factors)."""
    out = np.empty(int(size), np.float32)
    check(lib().cu2rec_init_normal(_ptr(out), int(size), int(n_factors), float(mean), float(stddev), int(seed)))
    return out


def writeToFile(parent_dir, base_filename, component, data, rows, cols, factors):
    """writeToFile (util.cu:99-103) with extension csv."""
    data = _f32(data).reshape(rows, cols)
    check(lib().cu2rec_write_component(os.fsencode(parent_dir), os.fsencode(base_filename), os.fsencode(component),
                                       _ptr(data), rows, cols, factors))


def writeCSV(path, data):
    data = _f32(data)
    data = data.reshape(data.shape[0], -1)
    check(lib().cu2rec_write_csv(os.fsencode(path), _ptr(data), data.shape[0], data.shape[1]))


def read_array(path):
    """read_array (util.cu:52-81) -> 2-D float32 array."""
    p = C.POINTER(C.c_float)()
    rows, cols = C.c_int(), C.c_int()
    check(lib().cu2rec_read_array(os.fsencode(path), C.byref(p), C.byref(rows), C.byref(cols)))
    try:
        n = rows.value * cols.value
        return np.ctypeslib.as_array(p, (n,)).copy().reshape(rows.value, cols.value) if n else np.zeros((0, 0), np.float32)
    finally:
        lib().cu2rec_free(p)


def sampler_index(seed, user, iteration, low, high):
    return lib().cu2rec_sampler_index(seed, user, iteration, low, high)


def item_update_rates(csr):
    """Expected SGD updates per iteration on each item from the users of `csr` (sum over raters of 1 / degree)."""
    out = np.zeros(csr.cols, np.float64)
    check(lib().cu2rec_item_update_rates(_ptr(csr.indptr), _ptr(csr.indices), csr.rows, csr.cols, _ptr(out)))
    return out


def shard_plan(rows, nranks):
    out = np.zeros(nranks + 1, np.int32)
    check(lib().cu2rec_shard_plan(rows, nranks, _ptr(out)))
    return out


# ------------------------------------------------------------------------------------------ device objects

def device_count():
    return lib().cu2rec_device_count()


class DeviceCSR:
    """CudaCSRMatrix (matrix.h:11-19): device copy of a HostCSR."""

    def __init__(self, host):
        self.host = host
        self._h = C.c_void_p()
        check(lib().cu2rec_csr_create(host.rows, host.cols, host.nnz, _ptr(host.indptr), _ptr(host.indices),
                                      _ptr(host.data), C.byref(self._h)))
        self.rows, self.cols, self.nnz = host.rows, host.cols, host.nnz

    def device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().cu2rec_csr_device_ptrs(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def bpr_negatives(self, seed, sweep):
        """The negative item Model.bpr() pairs with every stored entry in sweep `sweep` (cu2rec_csr_bpr_negatives) -> int32 (nnz,),
        -1 where all eight draws were items the row stores."""
        neg = np.empty(self.nnz, np.int32)
        check(lib().cu2rec_csr_bpr_negatives(self._h, int(seed), int(sweep), _ptr(neg)))
        return neg

    def knn_weights(self, weighting, k1=100.0, b=0.8):
        """The weight ItemKNN gives every stored entry (cu2rec_csr_knn_weights) -> float32 (nnz,), in the CSR's own entry order.
        weighting: "count", "cosine", "tfidf" or "bm25" (k1 and b are bm25's)."""
        weighting = _choice(KNN_WEIGHTINGS, weighting, "weighting")
        w = np.empty(self.nnz, np.float32)
        check(lib().cu2rec_csr_knn_weights(self._h, weighting, float(k1), float(b), _ptr(w)))
        return w

    def ease_gram(self, l2):
        """EASE's regularised Gram matrix (cu2rec_csr_ease_gram) -> float32 (cols, cols): ItemKNN's "count" similarities off the
        diagonal, the columns' sums of squares plus l2 on it."""
        g = np.empty((self.cols, self.cols), np.float32)
        check(lib().cu2rec_csr_ease_gram(self._h, float(l2), _ptr(g)))
        return g

    def multiply(self, D, transpose=False, padded=False):
        """X D, or X^T D with transpose (cu2rec_csr_multiply): PureSVD's sparse x dense-skinny product -> float32 (rows, f), or
        (cols, f) with transpose.  D: (cols, f), or (rows, f) with transpose; 1 <= f <= ALS_MAX_FACTORS.  padded: the rows as the
        device wrote them at the model's stride (f rounded up to 4 for user rows, to 32 for item rows), the padding columns zero."""
        D = np.ascontiguousarray(D, dtype=np.float32)
        n_in, n_out = (self.rows, self.cols) if transpose else (self.cols, self.rows)
        if D.ndim != 2 or D.shape[0] != n_in:
            raise ValueError("D must have shape (%d, f), not %s" % (n_in, D.shape))
        f = D.shape[1]
        ld = max(lib().cu2rec_csr_multiply_stride(1 if transpose else 0, f), f)
        out = np.empty((n_out, ld), np.float32)
        check(lib().cu2rec_csr_multiply(self._h, 1 if transpose else 0, _ptr(D), f, _ptr(out)))
        return out if padded else np.ascontiguousarray(out[:, :f])

    def blocksolve_items(self):
        """cu2rec_csr_blocksolve_items: how many items the block-solve mode solves block-wise here (0: it is the ordered walk)."""
        n = lib().cu2rec_csr_blocksolve_items(self._h)
        if n < 0:
            check(-1)
        return n

    def close(self):
        if self._h:
            lib().cu2rec_csr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """Device-resident P, Q, user_bias, item_bias (+ global_bias).  None = the reference's
    seed-42 normal initialisation (training.cu:28,54,212-213)."""

    def __init__(self, rows, cols, n_factors, global_bias, P=None, Q=None, user_bias=None, item_bias=None):
        self.rows, self.cols, self.n_factors, self.global_bias = int(rows), int(cols), int(n_factors), float(global_bias)
        P, Q = _f32(P, (rows, n_factors)), _f32(Q, (cols, n_factors))
        user_bias, item_bias = _f32(user_bias, (rows,)), _f32(item_bias, (cols,))
        self._h = C.c_void_p()
        check(lib().cu2rec_model_create(rows, cols, n_factors, _ptr(P), _ptr(Q), _ptr(user_bias), _ptr(item_bias),
                                        float(global_bias), C.byref(self._h)))

    def sgd(self, train, hyper, seed, iter0, n_iters, mode=SGD_HOGWILD, update_items=True):
        """n_iters reference iterations of sgd_update (sgd.cu:22-75) starting at global iteration iter0."""
        h = _hyper(hyper)
        check(lib().cu2rec_model_sgd(self._h, train._h, C.byref(h), int(seed), int(iter0), int(n_iters), _mode(mode),
                                     1 if update_items else 0))

    def als(self, train, hyper, side="both", sweeps=1, solver="cholesky", cg_steps=3):
        """Alternating-least-squares half-steps on the SGD modes' objective (cu2rec_model_als): side "users" solves P and
        user_bias against the frozen items, "items" the reverse, "both" a sweep (users, then items); repeated `sweeps` times.
        hyper: Hyper or (learning_rate, P_reg, Q_reg, user_bias_reg, item_bias_reg) -- the learning rate is ignored.
        solver "cholesky" solves every row exactly; "cg" gives the rows of at most ALS_CHUNK ratings cg_steps conjugate-gradient
        steps from their current factors and bias (cu2rec_model_als_cg; cg_steps is not read otherwise).
        Returns the number of rows left unchanged (a failed pivot; a non-finite or negative curvature), summed over the half-steps."""
        h = _hyper(hyper)
        _solver(solver)
        if solver == "cg":
            return _half_steps(side, sweeps, lambda s, n: lib().cu2rec_model_als_cg(self._h, train._h, C.byref(h), s, int(cg_steps), n))
        return _half_steps(side, sweeps, lambda s, n: lib().cu2rec_model_als(self._h, train._h, C.byref(h), s, n))

    def ials(self, train, hyper, alpha=40.0, side="both", sweeps=1, solver="cholesky", cg_steps=3):
        """Implicit-feedback half-steps (cu2rec_model_als_implicit): every user x item pair of train's shape counts, a stored entry
        (u, i, r) with confidence weight alpha * r; no biases.  side and sweeps as in als(); of hyper only P_reg and Q_reg are read.
        Rows without entries become zero rows.  solver "cholesky" solves every row exactly; "cg" gives the rows of at most
        ALS_CHUNK entries cg_steps conjugate-gradient steps from their current factors (cu2rec_model_als_implicit_cg; cg_steps is
        not read otherwise).  Returns the number of rows left unchanged (a failed pivot; a non-finite or negative curvature)."""
        h = _hyper(hyper)
        _solver(solver)
        if solver == "cg":
            return _half_steps(side, sweeps, lambda s, n: lib().cu2rec_model_als_implicit_cg(self._h, train._h, C.byref(h), float(alpha), s,
                                                                                             int(cg_steps), n))
        return _half_steps(side, sweeps, lambda s, n: lib().cu2rec_model_als_implicit(self._h, train._h, C.byref(h), float(alpha), s, n))

    def implicit_objective(self, train, hyper, alpha):
        """The objective ials() minimises, at the model's current values (cu2rec_model_implicit_objective) -> float."""
        h = _hyper(hyper)
        L = C.c_double()
        check(lib().cu2rec_model_implicit_objective(self._h, train._h, C.byref(h), float(alpha), C.byref(L)))
        return L.value

    def lmf(self, train, hyper, alpha=1.0, side="both", sweeps=1):
        """Logistic matrix factorization half-steps (cu2rec_model_lmf; Johnson 2014, full batch): the gradient of the log-posterior
        over every user x item pair of train's shape, a stored entry (u, i, r) with weight alpha * r, then an AdaGrad step at
        hyper's learning rate.  The score includes both biases and the global bias; all four regularisers are read.  side and
        sweeps as in als().  alpha defaults to 1.0, not ials()'s 40: here the weight multiplies a log-odds gradient, and 40 x a
        5-star rating saturates it.  The AdaGrad accumulators stay with the model (lmf_state, lmf_reset).
        Returns the number of rows left unchanged (a non-finite gradient or step), summed over the half-steps."""
        h = _hyper(hyper)
        return _half_steps(side, sweeps, lambda s, n: lib().cu2rec_model_lmf(self._h, train._h, C.byref(h), float(alpha), s, n))

    def _gradient_out(self, train, side):
        """What lmf_gradient() and bpr_gradient() hand to the library for side "users" or "items" -> (its constant, grad, bias_grad)."""
        if side not in ("users", "items"):
            raise ValueError("side must be 'users' or 'items', not %r" % (side,))
        n = train.rows if side == "users" else train.cols
        return ALS_SIDES[side][0], np.empty((n, self.n_factors), np.float32), np.empty(n, np.float32)

    def lmf_gradient(self, train, hyper, alpha, side):
        """The gradient lmf() would step along for side "users" or "items" (cu2rec_model_lmf_gradient) -> (grad, bias_grad),
        float32 of shapes (n, n_factors) and (n,), n = train's rows or cols.  The model and the accumulators are untouched."""
        h = _hyper(hyper)
        s, grad, bias = self._gradient_out(train, side)
        check(lib().cu2rec_model_lmf_gradient(self._h, train._h, C.byref(h), float(alpha), s, _ptr(grad), _ptr(bias)))
        return grad, bias

    def lmf_objective(self, train, hyper, alpha):
        """The log-posterior lmf() climbs, at the model's current values (cu2rec_model_lmf_objective) -> float."""
        h = _hyper(hyper)
        L = C.c_double()
        check(lib().cu2rec_model_lmf_objective(self._h, train._h, C.byref(h), float(alpha), C.byref(L)))
        return L.value

    def lmf_state(self):
        """The AdaGrad accumulators of lmf() -> aP, aQ, a_user_bias, a_item_bias, shaped like download(); zeros before the first call."""
        aP = np.empty((self.rows, self.n_factors), np.float32)
        aQ = np.empty((self.cols, self.n_factors), np.float32)
        aub, aib = np.empty(self.rows, np.float32), np.empty(self.cols, np.float32)
        check(lib().cu2rec_model_lmf_state(self._h, _ptr(aP), _ptr(aQ), _ptr(aub), _ptr(aib)))
        return aP, aQ, aub, aib

    def lmf_reset(self):
        """Zeroes the AdaGrad accumulators of lmf()."""
        check(lib().cu2rec_model_lmf_reset(self._h))

    def bpr(self, train, hyper, seed=42, sweep0=0, side="both", sweeps=1):
        """Bayesian Personalized Ranking half-steps (cu2rec_model_bpr; Rendle et al. 2009, deterministic and full batch): sweep
        sweep0 + k pairs every stored entry (u, i) with one negative item j drawn from the counter-based sampler (seed; see
        DeviceCSR.bpr_negatives), a half-step is the gradient of sum ln sigma((ib_i - ib_j) + p_u . (q_i - q_j)) minus the
        regularisers over those triples, then lmf()'s AdaGrad step at hyper's learning rate.  Stored values are not read; user
        biases never move.  side and sweeps as in als().  The AdaGrad accumulators are lmf()'s (lmf_state, lmf_reset): the model
        has one set, reset it between the two trainers.
        Returns the number of rows left unchanged (a non-finite gradient or step), summed over the half-steps."""
        h = _hyper(hyper)
        return _half_steps(side, sweeps, lambda s, n, k: lib().cu2rec_model_bpr(self._h, train._h, C.byref(h), int(seed), int(sweep0) + k, s, n),
                           numbered=True)

    def bpr_gradient(self, train, hyper, seed, sweep, side):
        """The gradient bpr() would step along for side "users" or "items" in sweep `sweep` (cu2rec_model_bpr_gradient) ->
        (grad, bias_grad) shaped as lmf_gradient()'s; the users' bias_grad is all zeros.  The model and the accumulators are
        untouched."""
        h = _hyper(hyper)
        s, grad, bias = self._gradient_out(train, side)
        check(lib().cu2rec_model_bpr_gradient(self._h, train._h, C.byref(h), int(seed), int(sweep), s, _ptr(grad), _ptr(bias)))
        return grad, bias

    def bpr_objective(self, train, hyper, seed, sweep):
        """The objective bpr() climbs over sweep `sweep`'s triples, at the model's current values (cu2rec_model_bpr_objective) ->
        (L, n_triples, n_ordered); n_ordered / n_triples is the sampled AUC."""
        h = _hyper(hyper)
        L, n, m = C.c_double(), C.c_longlong(), C.c_longlong()
        check(lib().cu2rec_model_bpr_objective(self._h, train._h, C.byref(h), int(seed), int(sweep), C.byref(L), C.byref(n), C.byref(m)))
        return L.value, n.value, m.value

    def softmax(self, train, hyper, side="both", sweeps=1):
        """Softmax matrix factorization half-steps (cu2rec_model_softmax; the multinomial likelihood of Liang et al. 2018, full
        batch): a user's items form one distribution pi_ui = softmax_i(s_ui) over every item of train's shape, a stored entry
        (u, i, r) is r draws from it, and a half-step is the gradient of sum w log pi_ui minus the regularisers, then lmf()'s AdaGrad
        step at hyper's learning rate.  There is no alpha; user biases and the global bias cancel and never move; of hyper's
        regularisers P_reg, Q_reg and item_bias_reg are read.  side and sweeps as in als().  The AdaGrad accumulators are lmf()'s
        (lmf_state, lmf_reset): the model has one set, reset it between trainers.  New users are fitted with side="users" on a model
        that shares Q.  Returns the number of rows left unchanged (a non-finite gradient or step), summed over the half-steps."""
        h = _hyper(hyper)
        return _half_steps(side, sweeps, lambda s, n: lib().cu2rec_model_softmax(self._h, train._h, C.byref(h), s, n))

    def softmax_gradient(self, train, hyper, side):
        """The gradient softmax() would step along for side "users" or "items" (cu2rec_model_softmax_gradient) -> (grad, bias_grad)
        shaped as lmf_gradient()'s; the users' bias_grad is all zeros.  The model and the accumulators are untouched."""
        h = _hyper(hyper)
        s, grad, bias = self._gradient_out(train, side)
        check(lib().cu2rec_model_softmax_gradient(self._h, train._h, C.byref(h), s, _ptr(grad), _ptr(bias)))
        return grad, bias

    def softmax_objective(self, train, hyper):
        """The objective softmax() climbs, at the model's current values (cu2rec_model_softmax_objective) -> float."""
        h = _hyper(hyper)
        L = C.c_double()
        check(lib().cu2rec_model_softmax_objective(self._h, train._h, C.byref(h), C.byref(L)))
        return L.value

    def softmax_lse(self, train):
        """log sum_i exp(s_ui) over every item of train's shape, for every user of train (cu2rec_model_softmax_lse) -> float32
        (train.rows,), as the half-steps form it."""
        lse = np.empty(train.rows, np.float32)
        check(lib().cu2rec_model_softmax_lse(self._h, train._h, _ptr(lse)))
        return lse

    def softmax_mass(self, train):
        """sum_i pi_ui of every user of train as the user half-step's matrix-core product forms it (cu2rec_model_softmax_mass) ->
        float32 (train.rows,): 1 within rounding."""
        mass = np.empty(train.rows, np.float32)
        check(lib().cu2rec_model_softmax_mass(self._h, train._h, _ptr(mass)))
        return mass

    def svd(self, train, sweeps=4):
        """PureSVD (cu2rec_model_svd; Cremonesi, Koren, Turrin 2010): `sweeps` sweeps of block subspace iteration on the matrix
        `train` stores, from the model's current item factors -- Y = orth(X Q), Q = orth(X^T Y), orth being Cholesky-QR twice --
        then P = X Q and both biases 0, so that P Q^T = X Q Q^T.  No learning rate, no regulariser; create the model with
        global_bias 0 for the scores to be p . q.  Q is the only carried state: svd(sweeps=2) twice is svd(sweeps=4) once, bit
        for bit.  n_factors above the matrix's numerical rank is refused (Cu2recError, CU2REC_EUNSUPPORTED) and leaves the model
        as it was.  Returns dict(sweeps, captured = |X Q|_F^2, total = |X|_F^2)."""
        rep = SvdReport()
        check(lib().cu2rec_model_svd(self._h, train._h, int(sweeps), C.byref(rep)))
        return {"sweeps": rep.sweeps, "captured": rep.captured, "total": rep.total}

    def project(self, history):
        """H Q for the rows of `history` (cu2rec_model_project) -> float32 (history.rows, n_factors): the fold-in of new users by
        projection, p = r Q.  history: DeviceCSR with the model's column count.  project(train) is svd(train)'s P bit for bit."""
        out = np.empty((history.rows, self.n_factors), np.float32)
        check(lib().cu2rec_model_project(self._h, history._h, _ptr(out)))
        return out

    def loss(self, ratings):
        """calculate_loss_gpu + get_error_metrics_gpu (loss.cu:40-49,195-200) -> dict(mae, rmse, sum_abs, sum_sq)."""
        sa, ss, mae, rmse = C.c_double(), C.c_double(), C.c_float(), C.c_float()
        check(lib().cu2rec_model_loss(self._h, ratings._h, C.byref(sa), C.byref(ss), C.byref(mae), C.byref(rmse)))
        return {"mae": mae.value, "rmse": rmse.value, "sum_abs": sa.value, "sum_sq": ss.value}

    def download(self):
        """-> P, Q, user_bias, item_bias as dense numpy arrays (training.cu:180-185)."""
        P = np.empty((self.rows, self.n_factors), np.float32)
        Q = np.empty((self.cols, self.n_factors), np.float32)
        ub, ib = np.empty(self.rows, np.float32), np.empty(self.cols, np.float32)
        check(lib().cu2rec_model_download(self._h, _ptr(P), _ptr(Q), _ptr(ub), _ptr(ib)))
        return P, Q, ub, ib

    def scores(self):
        """predict_ratings (predict.cu:17-30) for every user against every item -> (rows, cols) float32."""
        out = np.empty((self.rows, self.cols), np.float32)
        check(lib().cu2rec_model_scores_host(self._h, _ptr(out)))
        return out

    def recommend(self, rated, k):
        """get_recommendations (predict.cu:49-65) for every user: the k best unrated items -> (items, scores), each
        (rows, k); -1 / NaN where a user has fewer than k unrated items.  rated: DeviceCSR (row u = user u) or None."""
        items, scores = np.empty((self.rows, k), np.int32), np.empty((self.rows, k), np.float32)
        check(lib().cu2rec_model_recommend(self._h, rated._h if rated is not None else None, int(k), _ptr(items), _ptr(scores)))
        return items, scores

    def topk(self, exclude, k, users=None):
        """The k best non-excluded items of each user, without the dense score matrix (cu2rec_model_topk) -> (items,
        scores), each (n, k): recommend's scores and order bit for bit (equal scores by ascending item; -inf never listed);
        -1 / NaN where a user has fewer than k candidates.  exclude: DeviceCSR (row u = user u's excluded items) or None.
        users: model row ids (duplicates allowed), or None for every row.  1 <= k <= 256."""
        ids = None if users is None else np.ascontiguousarray(users, dtype=np.int32).reshape(-1)
        n = self.rows if ids is None else len(ids)
        items, scores = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_model_topk(self._h, exclude._h if exclude is not None else None, _ptr(ids), int(n), int(k),
                                      _ptr(items), _ptr(scores)))
        return items, scores

    def similar(self, ids=None, k=10, side="items", metric="cosine", exclude=None):
        """Nearest neighbours among the rows of one factor matrix (cu2rec_model_similar) -> (ids, scores), each (n, k).
        side: "items" (rows of Q) or "users" (rows of P); metric: "cosine" or "dot" (no biases).  Cosine is the dot product of
        the unit rows x / |x| (computed in double, rounded to float), so it holds at any row magnitude; a zero row has cosine
        0 with everything, and a row holding an inf or a NaN scores +NaN with everything (listed first).  ids: rows of that side
        (duplicates allowed), or None for every row; a query row is never its own neighbour.  exclude: DeviceCSR whose row a
        holds the rows excluded for row a, or None.  Order, ties and -1 / NaN padding are topk's.  1 <= k <= 256."""
        side, metric = _choice(SIDES, side, "side"), _choice(METRICS, metric, "metric")
        q = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n = (self.rows if side == SIDE_USERS else self.cols) if q is None else len(q)
        out, scores = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_model_similar(self._h, side, metric, exclude._h if exclude is not None else None, _ptr(q), int(n),
                                         int(k), _ptr(out), _ptr(scores)))
        return out, scores

    def top_users(self, exclude, k, items=None):
        """The k users with the best predicted rating for each item (cu2rec_model_top_users) -> (users, scores), each (n, k):
        the floats of scores()[:, i], in topk's order (equal scores by ascending user; -inf never listed; -1 / NaN padding).
        exclude: DeviceCSR whose row i holds item i's excluded users (e.g. DeviceCSR(train.transpose())), or None.  items:
        item ids (duplicates allowed), or None for every item.  1 <= k <= 256."""
        ids = None if items is None else np.ascontiguousarray(items, dtype=np.int32).reshape(-1)
        n = self.cols if ids is None else len(ids)
        users, scores = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_model_top_users(self._h, exclude._h if exclude is not None else None, _ptr(ids), int(n), int(k),
                                           _ptr(users), _ptr(scores)))
        return users, scores

    def rank_metrics(self, test, k, exclude=None, threshold=None, per_user=False):
        """Ranking quality at k of the top-k lists (topk over every row, excluding `exclude`) against `test`
        (cu2rec_model_rank_metrics; definitions in include/cu2rec_amd.h) -> dict(precision, recall, ndcg, map, hit_rate,
        users_evaluated, users_skipped, k), and with per_user=True also a (rows, 5) float64 array {precision, recall, ndcg,
        ap, hit}, NaN for skipped users.  R_u = distinct items of test row u rated >= threshold (None: every rating);
        users with an empty R_u are skipped.  test / exclude: DeviceCSR."""
        out = RankMetrics()
        per = np.empty((self.rows, 5), np.float64) if per_user else None
        thr = -np.inf if threshold is None else float(threshold)
        check(lib().cu2rec_model_rank_metrics(self._h, exclude._h if exclude is not None else None, test._h, int(k), thr,
                                              C.byref(out), _ptr(per)))
        res = {name: getattr(out, name) for name, _ in RankMetrics._fields_}
        return (res, per) if per_user else res

    def device_ptrs(self):
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().cu2rec_model_device_ptrs(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    @property
    def ld(self):
        ld = C.c_int()
        check(lib().cu2rec_model_info(self._h, None, None, None, C.byref(ld), None))
        return ld.value

    def close(self):
        if self._h:
            lib().cu2rec_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ItemKNN:
    """Item-based nearest-neighbour recommender (cu2rec_knn_*; include/cu2rec_amd.h): every stored entry of `train` is weighted
    ("count", "cosine", "tfidf" or "bm25", the last with k1 and b), the similarity of two items is the sum of the weight products over
    the users that store both, and every item keeps its `neighbours` best touched neighbours (1 .. 256).  No factors, no learning
    rate, no seed; results are bit-identical run to run.  Rows may be unsorted; a row that stores a column twice is refused."""

    def __init__(self, train, weighting="cosine", neighbours=20, k1=100.0, b=0.8):
        self._h = None
        code = _choice(KNN_WEIGHTINGS, weighting, "weighting")
        self.weighting, self.items, self.neighbours = weighting, train.cols, int(neighbours)
        h = C.c_void_p()
        check(lib().cu2rec_knn_create(train._h, code, float(k1), float(b), int(neighbours), C.byref(h)))
        self._h = h

    def neighbors(self, ids=None, k=None):
        """The k best neighbours of each listed item (cu2rec_knn_neighbors) -> (ids, sims), each (n, k); topk's order, ties and
        -1 / NaN padding.  ids: item ids (duplicates allowed), or None for every item; k: at most `neighbours` (None: all)."""
        k = self.neighbours if k is None else int(k)
        q = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n = self.items if q is None else len(q)
        out, sims = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_knn_neighbors(self._h, _ptr(q), int(n), k, _ptr(out), _ptr(sims)))
        return out, sims

    def recommend(self, history, exclude, k, users=None):
        """The k best items for each listed row of `history` (cu2rec_knn_recommend) -> (items, scores), each (n, k): the row's raw
        values pushed through the truncated neighbour lists, the candidates being the items some history item lists, outside row
        u of `exclude` (DeviceCSR or None).  users: row ids of history (duplicates allowed), or None for every row.  1 <= k <= 256."""
        k = int(k)
        q = None if users is None else np.ascontiguousarray(users, dtype=np.int32).reshape(-1)
        n = history.rows if q is None else len(q)
        items, scores = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_knn_recommend(self._h, history._h, exclude._h if exclude is not None else None, _ptr(q), int(n), k,
                                         _ptr(items), _ptr(scores)))
        return items, scores

    def rank_metrics(self, history, test, k, exclude=None, threshold=None, per_user=False):
        """Model.rank_metrics' figures over recommend()'s lists of every row of `history` (cu2rec_knn_rank_metrics)."""
        out = RankMetrics()
        per = np.empty((history.rows, 5), np.float64) if per_user else None
        thr = -np.inf if threshold is None else float(threshold)
        check(lib().cu2rec_knn_rank_metrics(self._h, history._h, exclude._h if exclude is not None else None, test._h, int(k), thr,
                                            C.byref(out), _ptr(per)))
        res = {name: getattr(out, name) for name, _ in RankMetrics._fields_}
        return (res, per) if per_user else res

    def close(self):
        if self._h:
            lib().cu2rec_knn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EASE:
    """EASE (Steck 2019; cu2rec_ease_*; include/cu2rec_amd.h): the closed-form item x item weights B_ij = -P_ij / P_jj, B_ii = 0, from
    P = (X^T X + l2 I)^-1 of the values `train` stores, inverted in float32 on the device.  One hyper-parameter, no factors, no seed, no
    iterations; results are bit-identical run to run.  At most 65,536 items on one GPU; rows may be unsorted; a train row that stores
    a column twice is refused, and so is an l2 too small for the matrix to be positive definite in float32."""

    def __init__(self, train, l2=500.0):
        self._h = None
        self.items, self.l2 = train.cols, float(l2)
        h = C.c_void_p()
        check(lib().cu2rec_ease_create(train._h, float(l2), C.byref(h)))
        self._h = h

    @staticmethod
    def _ids(ids):
        return None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)

    def weights(self, ids=None):
        """Rows of B (cu2rec_ease_weights) -> float32 (n, items).  ids: item ids (duplicates allowed), or None for every item."""
        q = self._ids(ids)
        n = self.items if q is None else len(q)
        out = np.empty((n, self.items), np.float32)
        check(lib().cu2rec_ease_weights(self._h, _ptr(q), int(n), _ptr(out)))
        return out

    def neighbors(self, ids=None, k=10):
        """The k largest B_ij, j != i, of each listed item i (cu2rec_ease_neighbors) -> (ids, vals), each (n, k); topk's order, ties
        and -1 / NaN padding.  ids: item ids (duplicates allowed), or None for every item.  1 <= k <= 256."""
        k = int(k)
        q = self._ids(ids)
        n = self.items if q is None else len(q)
        out, vals = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_ease_neighbors(self._h, _ptr(q), int(n), k, _ptr(out), _ptr(vals)))
        return out, vals

    def recommend(self, history, exclude, k, users=None):
        """The k best items for each listed row of `history` (cu2rec_ease_recommend) -> (items, scores), each (n, k): the row's raw
        values pushed through B; EVERY item outside row u of `exclude` (DeviceCSR or None) is a candidate.  users: row ids of
        history (duplicates allowed), or None for every row.  1 <= k <= 256."""
        k = int(k)
        q = self._ids(users)
        n = history.rows if q is None else len(q)
        items, scores = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
        check(lib().cu2rec_ease_recommend(self._h, history._h, exclude._h if exclude is not None else None, _ptr(q), int(n), k,
                                          _ptr(items), _ptr(scores)))
        return items, scores

    def rank_metrics(self, history, test, k, exclude=None, threshold=None, per_user=False):
        """Model.rank_metrics' figures over recommend()'s lists of every row of `history` (cu2rec_ease_rank_metrics)."""
        out = RankMetrics()
        per = np.empty((history.rows, 5), np.float64) if per_user else None
        thr = -np.inf if threshold is None else float(threshold)
        check(lib().cu2rec_ease_rank_metrics(self._h, history._h, exclude._h if exclude is not None else None, test._h, int(k), thr,
                                             C.byref(out), _ptr(per)))
        res = {name: getattr(out, name) for name, _ in RankMetrics._fields_}
        return (res, per) if per_user else res

    def close(self):
        if self._h:
            lib().cu2rec_ease_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SLIM(EASE):
    """SLIM (Ning & Karypis 2011; cu2rec_slim_create; include/cu2rec_amd.h): sparse item x item weights W -- EASE's least-squares
    problem with an L1 penalty `l1` and, when `positive`, non-negative weights -- by at most `sweeps` sweeps of blocked cyclic
    coordinate descent in float32 on the device, stopping after a sweep whose largest change is <= tol.  `.report` holds the sweeps
    run, the last sweep's largest |delta| and the nonzeros of W.  The lists are EASE's, from W in B's place; results are bit-identical
    run to run.  EASE's limits; while it is built the model holds three items x items matrices instead of one."""

    def __init__(self, train, l1=5.0, l2=500.0, positive=True, sweeps=10, tol=1e-3):
        self._h = None
        self.items, self.l1, self.l2, self.positive = train.cols, float(l1), float(l2), bool(positive)
        h, rep = C.c_void_p(), SlimReport()
        check(lib().cu2rec_slim_create(train._h, float(l1), float(l2), int(bool(positive)), int(sweeps), float(tol), C.byref(rep), C.byref(h)))
        self._h = h
        self.report = {"sweeps": rep.sweeps, "last_delta": rep.last_delta, "nonzeros": rep.nonzeros}


def orthonormalize(Y):
    """orth(Y) of PureSVD alone (cu2rec_orthonormalize): Cholesky-QR twice on the device -> float32 (n, f) with orthonormal columns
    that span Y's.  A pivot that is not a finite number above 2^-22 of its diagonal entry (dependent columns, n < f, a NaN) raises
    Cu2recError (CU2REC_EUNSUPPORTED) with .bad_column set."""
    Y = np.array(Y, dtype=np.float32, order="C", ndmin=2)
    bad = C.c_int(-1)
    try:
        check(lib().cu2rec_orthonormalize(_ptr(Y), Y.shape[0], Y.shape[1], C.byref(bad)))
    except Cu2recError as e:
        e.bad_column = bad.value
        raise
    return Y


def default_mode(n_factors):
    """The default SGD mode of train(), bin/mf and bench.py: block-solve (mf_sequential.cu's result within float rounding, the mode
    certified against the 1e-4 RMSE bar); above 252 factors, where it is not compiled, `ordered` (the same result bit for bit)."""
    return SGD_BLOCKSOLVE if n_factors <= 252 else SGD_ORDERED


def train(train_matrix, test_matrix, cfg, Q=None, item_bias=None, global_bias=None, mode=None, verbose=True,
          P=None, user_bias=None, return_stats=False, alpha=None, solver="cholesky", cg_steps=3):
    """train() (training.h:12-15).  mode None = default_mode(cfg.n_factors); "hogwild" opts into sgd.cu's racy semantics; "als"
    trains by alternating least squares (one iteration = one sweep; no learning rate, so no decay); "ials" by its implicit-feedback
    form with confidence weight alpha * r (cu2rec_train_implicit: test_matrix is not read and may be None, and the third element
    returned is the objective at the checked sweeps, float64, NaN elsewhere; solver="cg" runs the sweeps with cg_steps conjugate-gradient
    steps per row, cu2rec_train_implicit_cg; with mode "als" it is cu2rec_train_als_cg -- solver and cg_steps are read in these two modes
    only); "lmf" by logistic matrix factorization (cu2rec_train_lmf: like "ials", test_matrix may be None and the third element is the
    log-posterior at the checked sweeps; cfg.learning_rate is AdaGrad's and does not decay); "bpr" by Bayesian Personalized Ranking
    (cu2rec_train_bpr: like "lmf", with cfg.seed drawing the negatives and no alpha); "softmax" by softmax matrix factorization
    (cu2rec_train_softmax: like "lmf" without an alpha, the third element its objective); "svd" builds PureSVD (cu2rec_train_svd:
    cfg.total_iterations sweeps from the item factors, which a cfg.seed other than 42 draws again; test_matrix may be None, the model
    is created with global_bias 0 unless one is given, and the third element is [captured, total] of Model.svd's report).  alpha None is 40.0 for "ials" and 1.0 for
    "lmf", where the weight multiplies a log-odds gradient and 40 x a 5-star rating saturates it.
    train_matrix / test_matrix: DeviceCSR (or HostCSR, uploaded here).
    Q / item_bias given = the 11-argument overload (caller-initialised item side, predict.cu:126);
    otherwise everything starts from the seed-42 normal init.  Returns (P, Q, losses, user_bias,
    item_bias) like the reference's out-pointers; cfg.learning_rate / cfg.cur_iterations are
    updated in place."""
    if mode in ("als", "ials"):
        _solver(solver)
    if alpha is None:
        alpha = 1.0 if mode == "lmf" else 40.0
    tr = train_matrix if isinstance(train_matrix, DeviceCSR) else DeviceCSR(train_matrix)
    gb = (0.0 if mode == "svd" else tr.host.global_bias) if global_bias is None else global_bias
    model = Model(tr.rows, tr.cols, cfg.n_factors, gb, P=P, Q=Q, user_bias=user_bias, item_bias=item_bias)
    stats = TrainStats()
    if mode in ("bpr", "lmf", "softmax", "ials"):  # the objective-driven modes
        losses = np.empty(max(cfg.total_iterations, 1), np.float64)
    if mode == "svd":
        rep = SvdReport()
        check(lib().cu2rec_train_svd(tr._h, C.byref(cfg), model._h, 1 if verbose else 0, C.byref(rep)))
        Pn, Qn, ub, ib = model.download()
        model.close()
        out = (Pn, Qn, np.array([rep.captured, rep.total], np.float64), ub, ib)
        return out + (stats,) if return_stats else out
    if mode == "bpr":
        check(lib().cu2rec_train_bpr(tr._h, C.byref(cfg), model._h, 1 if verbose else 0, _ptr(losses), C.byref(stats)))
    elif mode == "lmf":
        check(lib().cu2rec_train_lmf(tr._h, C.byref(cfg), model._h, float(alpha), 1 if verbose else 0, _ptr(losses), C.byref(stats)))
    elif mode == "softmax":
        check(lib().cu2rec_train_softmax(tr._h, C.byref(cfg), model._h, 1 if verbose else 0, _ptr(losses), C.byref(stats)))
    elif mode == "ials":
        if solver == "cg":
            check(lib().cu2rec_train_implicit_cg(tr._h, C.byref(cfg), model._h, float(alpha), int(cg_steps), 1 if verbose else 0,
                                                 _ptr(losses), C.byref(stats)))
        else:
            check(lib().cu2rec_train_implicit(tr._h, C.byref(cfg), model._h, float(alpha), 1 if verbose else 0, _ptr(losses),
                                              C.byref(stats)))
    else:
        te = test_matrix if isinstance(test_matrix, DeviceCSR) else DeviceCSR(test_matrix)
        losses = np.empty(max(cfg.total_iterations, 1), np.float32)
        mode = default_mode(cfg.n_factors) if mode is None else mode
        if mode == "als" and solver == "cg":
            check(lib().cu2rec_train_als_cg(tr._h, te._h, C.byref(cfg), model._h, int(cg_steps), 1 if verbose else 0, _ptr(losses),
                                            C.byref(stats)))
        else:
            check(lib().cu2rec_train(tr._h, te._h, C.byref(cfg), model._h, _mode(mode), 1 if verbose else 0, _ptr(losses),
                                     C.byref(stats)))
    Pn, Qn, ub, ib = model.download()
    model.close()
    out = (Pn, Qn, losses[:cfg.total_iterations], ub, ib)
    return out + (stats,) if return_stats else out


# ------------------------------------------------------------------------------------------ raw device pointers

def sgd_update(indptr, indices, data, n_rows, n_cols, P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors,
               hyper, seed, iter0, n_iters, mode=SGD_HOGWILD, update_items=True, user_offset=0, stream=None,
               sample_pairs=None):
    """cu2rec_sgd_update(_ex) on raw device addresses (ints); sample_pairs: the optional side-by-side sample array."""
    h = _hyper(hyper)
    check(lib().cu2rec_sgd_update_ex(indptr, indices, data, n_rows, n_cols, P, ldp, Q, ldq, user_bias, item_bias,
                                     float(global_bias), n_factors, C.byref(h), int(seed), int(iter0), int(n_iters),
                                     _mode(mode), 1 if update_items else 0, int(user_offset), sample_pairs, stream))


def sample_pairs_build(indices, data, nnz, pairs, stream=None):
    """cu2rec_sample_pairs_build on raw device addresses: pairs[k] = {indices[k], data[k]}."""
    check(lib().cu2rec_sample_pairs_build(indices, data, int(nnz), pairs, stream))


class Schedule:
    """Workspace of the ordered mode for one device CSR (cu2rec_schedule)."""

    def __init__(self, indptr, indices, n_rows, n_cols, nnz):
        self._h = C.c_void_p()
        check(lib().cu2rec_schedule_create(indptr, indices, n_rows, n_cols, nnz, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().cu2rec_schedule_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sgd_update_ordered(schedule, indptr, indices, data, n_rows, n_cols, P, ldp, Q, ldq, user_bias, item_bias,
                       global_bias, n_factors, hyper, seed, iter0, n_iters, update_items=True, user_offset=0,
                       stream=None):
    """cu2rec_sgd_update_ordered on raw device addresses."""
    h = _hyper(hyper)
    check(lib().cu2rec_sgd_update_ordered(schedule._h, indptr, indices, data, n_rows, n_cols, P, ldp, Q, ldq, user_bias,
                                          item_bias, float(global_bias), n_factors, C.byref(h), int(seed), int(iter0),
                                          int(n_iters), 1 if update_items else 0, int(user_offset), stream))


def sgd_update_blocksolve(schedule, indptr, indices, data, n_rows, n_cols, P, ldp, Q, ldq, user_bias, item_bias,
                          global_bias, n_factors, hyper, seed, iter0, n_iters, update_items=True, user_offset=0,
                          stream=None):
    """cu2rec_sgd_update_blocksolve on raw device addresses."""
    h = _hyper(hyper)
    check(lib().cu2rec_sgd_update_blocksolve(schedule._h, indptr, indices, data, n_rows, n_cols, P, ldp, Q, ldq,
                                             user_bias, item_bias, float(global_bias), n_factors, C.byref(h), int(seed),
                                             int(iter0), int(n_iters), 1 if update_items else 0, int(user_offset), stream))


def blocksolve_min_rate(rate=0.0):
    """cu2rec_blocksolve_min_rate: expected updates per iteration from which an item's chain is solved block-wise.
    rate > 0 sets it, rate < 0 returns to the automatic threshold, 0 queries; returns what was in force before (-1: automatic),
    so blocksolve_min_rate(previous) restores either state."""
    return lib().cu2rec_blocksolve_min_rate(float(rate))


def blocksolve_lookahead_blocks(blocks=-1):
    """cu2rec_blocksolve_lookahead_blocks: items expected to collect at least this many 64-update blocks per iteration run phase 2
    in the look-ahead form (default 24: the top chains; 0: off; read when a DeviceCSR's schedule is created)."""
    return lib().cu2rec_blocksolve_lookahead_blocks(int(blocks))


def blocksolve_topology():
    """cu2rec_blocksolve_topology -> ("device" | "events" | None before the first block-solve call, the reason)."""
    buf = C.create_string_buffer(512)
    mode = lib().cu2rec_blocksolve_topology(buf, len(buf))
    return {2: "device", 0: "events"}.get(mode), buf.value.decode(errors="replace")


def loss_raw(indptr, indices, data, n_rows, nnz, P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors,
             workspace, errors_out=None, stream=None):
    sa, ss, mae, rmse = C.c_double(), C.c_double(), C.c_float(), C.c_float()
    check(lib().cu2rec_loss(indptr, indices, data, n_rows, nnz, P, ldp, Q, ldq, user_bias, item_bias,
                            float(global_bias), n_factors, errors_out, workspace, C.byref(sa), C.byref(ss),
                            C.byref(mae), C.byref(rmse), stream))
    return {"mae": mae.value, "rmse": rmse.value, "sum_abs": sa.value, "sum_sq": ss.value}


def error_metrics_raw(errors, n, workspace, stream=None):
    """get_error_metrics_gpu (loss.cu:195-200) on a device array of residuals -> (mae, rmse)."""
    mae, rmse = C.c_float(), C.c_float()
    check(lib().cu2rec_error_metrics(errors, n, workspace, C.byref(mae), C.byref(rmse), stream))
    return mae.value, rmse.value
