"""TEST INFRASTRUCTURE shared by tests/test_gpu_als.py, tests/test_gpu_als_edges.py and tests/test_als_cpu.py: the judgement of
one GPU half-step against the float64 reference (tests/als_reference64.py), and the rating sets of the edge tests, which the CPU
suite also solves with the float32 restatement to show that they are fair.  Nothing here needs a GPU to be imported."""
import ctypes as C

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib

import als_reference64 as ref

HYPER = (0.01, 0.05, 0.04, 0.02, 0.03)  # (learning rate: ignored, P_reg, Q_reg, user_bias_reg, item_bias_reg)
_CACHE = {}


def hip():
    if "hip" not in _CACHE:
        lib()
        h = C.CDLL("libamdhip64.so.7")
        h.hipMemcpy.restype = C.c_int
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _CACHE["hip"] = h
    return _CACHE["hip"]


def q_padding(model, f):
    _, Q, _, _ = model.device_ptrs()
    ldq = lib().cu2rec_model_item_stride(model._h)
    out = np.empty((model.cols, ldq), np.float32)
    assert hip().hipMemcpy(out.ctypes.data, Q, out.nbytes, 2) == 0
    return out[:, f:]


def als(model, d_csr, hyper, side):
    n = C.c_int(-1)
    h = cu.Hyper(*[float(x) for x in hyper])
    rc = lib().cu2rec_model_als(model._h, d_csr._h, C.byref(h), api.SIDES[side], C.byref(n))
    return rc, n.value


def rows_with_ratings(csr, side):
    counts = np.diff(csr.indptr) if side == "users" else np.bincount(csr.indices, minlength=csr.cols)
    return np.flatnonzero(counts > 0)


def own_major(csr, side):
    """(indptr, indices, data) as the half-step of `side` reads the ratings: the CSR itself, or its item-major view."""
    if side == "users":
        return np.asarray(csr.indptr, np.int64), np.asarray(csr.indices, np.int64), np.asarray(csr.data, np.float64)
    return ref.transpose(csr)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_half_step(model, d_csr, csr, side, hyper=HYPER, *, forward=True, residual=False, rows=None, singular=None,
                    row_objective=False, label=None, report=None):
    """One GPU half-step against the float64 reference from the same float32 state; returns the state after it.

    Always: return code 0; the other side, rows without ratings, model rows past the CSR and Q's padding floats keep their bits.
    forward: every judged row within 1e-3 max(1, |x*|_inf) of the float64 optimum x* (True, False, or a boolean mask over the
        side's rows), and -- when every row is judged -- the float64 objective at most the optimum's (1 + 1e-6).
    residual: every judged row's |A x - b| within ref.row_residual's entrywise rounding bound.
    rows: judge only these rows in float64 (every other owned row with ratings must still be finite); None: all of them.
    singular: None -- `unsolved` must be 0, and every rated row is judged, one that kept its bits included (a row the kernel
        skipped without counting it misses the bars like any wrong row).  Otherwise the rows (ids of this side) that are allowed to be left unsolved:
        `unsolved` must equal the number of rated rows that kept their bits, and each of them must be listed here; the
        rows that changed are judged.
    row_objective: every judged, solved row's own objective is not above its value before the half-step plus
        ref.objective_slack.
    label: row id -> text for assertion messages (the class of a row); report: a dict that receives the worst ratios."""
    f = model.n_factors
    before = model.download()
    pad_before = q_padding(model, f)
    rc, unsolved = als(model, d_csr, hyper, side)
    assert rc == 0, (rc, lib().cu2rec_last_error())
    got = model.download()
    own = (0, 2) if side == "users" else (1, 3)
    other = (1, 3) if side == "users" else (0, 2)
    name = (lambda r: (int(r), label(int(r)))) if label else int
    for k in other:
        assert same_bits(got[k], before[k]), "the other side moved (%s half-step, f=%d)" % (side, f)
    rated = rows_with_ratings(csr, side)
    untouched = np.setdiff1d(np.arange(len(before[own[1]])), rated)
    for k in own:  # rows without ratings, and model rows past the CSR, keep their values bit for bit
        assert same_bits(got[k][untouched], before[k][untouched]), (side, f)
    assert same_bits(q_padding(model, f), pad_before) and not pad_before.any()
    x_all = np.concatenate([got[own[0]], got[own[1]][:, None]], axis=1)
    x0_all = np.concatenate([before[own[0]], before[own[1]][:, None]], axis=1)
    kept = rated[(np.ascontiguousarray(x_all[rated]).view(np.uint32) == np.ascontiguousarray(x0_all[rated]).view(np.uint32)).all(axis=1)]
    if singular is None:
        assert unsolved == 0, (side, f, unsolved, [name(r) for r in kept[:8]])
    else:
        assert unsolved == len(kept), (side, f, unsolved, [name(r) for r in kept[:8]])
        stray = np.setdiff1d(kept, np.asarray(list(singular), np.int64))
        assert len(stray) == 0, ("rows left unsolved outside the singular class", side, f, [name(r) for r in stray[:8]])
    assert np.isfinite(x_all[rated]).all(), (side, f, [name(r) for r in rated[~np.isfinite(x_all[rated]).all(axis=1)][:8]])
    judged = rated if rows is None else np.intersect1d(rated, np.asarray(rows, np.int64))
    if singular is not None:  # (otherwise a row that kept its bits is judged like any other: it was not solved unless it was the solution)
        judged = np.setdiff1d(judged, kept)
    fmask = np.zeros(len(x_all), bool)
    fmask[judged] = True
    if forward is False:
        fmask[:] = False
    elif forward is not True:
        fmask &= np.asarray(forward, bool)
    indptr, indices, data = own_major(csr, side)
    X, xb = before[other[0]], before[other[1]]
    _, P_reg, Q_reg, ubr, ibr = hyper
    reg, reg_b = (P_reg, ubr) if side == "users" else (Q_reg, ibr)
    want = None
    if rows is None and forward is True and singular is None:  # the whole half-step in float64, as before the edge tests
        want = ref.half_step(csr, *before, csr.global_bias, hyper, side)
        xs_all = np.concatenate([want[own[0]], want[own[1]][:, None]], axis=1)
    worst_f, worst_r = 0.0, 0.0
    for r in judged:
        x = x_all[r].astype(np.float64)
        if residual or row_objective or (fmask[r] and want is None):
            A, b, res, bound = ref.row_residual(indptr, indices, data, X, xb, csr.global_bias, reg, reg_b, int(r), x)
        if residual:
            ratio = ref.residual_ratio(res, bound)
            worst_r = max(worst_r, ratio)
            assert ratio <= 1.0, ("residual above the rounding bound", side, f, name(r), int(indptr[r + 1] - indptr[r]), ratio)
        if fmask[r]:
            xs = xs_all[r] if want is not None else np.linalg.solve(A, b)
            err, bar = float(np.abs(x - xs).max()), 1e-3 * max(1.0, float(np.abs(xs).max()))
            worst_f = max(worst_f, err / bar)
            assert err <= bar, (side, f, name(r), int(indptr[r + 1] - indptr[r]), err, bar)
        if row_objective:
            slack = ref.objective_slack(bound, x, x0_all[r])
            phi, phi0 = ref.row_objective(A, b, x), ref.row_objective(A, b, x0_all[r])
            assert phi <= phi0 + slack, ("the row's objective rose", side, f, name(r), phi0, phi, slack)
    if want is not None:
        L_got = ref.objective(csr, *got, csr.global_bias, hyper)
        L_opt = ref.objective(csr, *want, csr.global_bias, hyper)
        assert L_got <= L_opt * (1 + 1e-6), (side, f, L_got, L_opt)
    if report is not None:
        report["forward"] = max(report.get("forward", 0.0), worst_f)
        report["residual"] = max(report.get("residual", 0.0), worst_r)
        report["unsolved"] = report.get("unsolved", 0) + unsolved
    return got


def bigger_model(csr, f, extra_rows=3, extra_cols=5):
    """A model with rows / items past the CSR (they must stay as they are)."""
    return cu.Model(csr.rows + extra_rows, csr.cols + extra_cols, f, csr.global_bias)


def random_state(rows, cols, f, seed, factor_scale=0.3, bias_scale=0.1):
    """Factors of O(0.3) and biases of O(0.1): against the tiny seed-42 initial values a wrong Gram hides behind the regulariser."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, factor_scale, (rows, f)).astype(np.float32), rng.normal(0, factor_scale, (cols, f)).astype(np.float32),
            rng.normal(0, bias_scale, rows).astype(np.float32), rng.normal(0, bias_scale, cols).astype(np.float32))


def model_from(state, gb, f=None):
    P, Q, ub, ib = state
    return cu.Model(P.shape[0], Q.shape[0], P.shape[1] if f is None else f, gb, P=P, Q=Q, user_bias=ub, item_bias=ib)


def same_state(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def interplay(steps, tr, f, state=None, objects=None):
    """`steps` on one Model and one DeviceCSR against the same steps with the model downloaded and re-created, and the
    DeviceCSR uploaded afresh, between every two of them: after every step the two states are equal bit for bit, and so is
    what the step returned (a count of unsolved rows, an objective).  state: the float32 values to start from (default: the
    seed-42 initial model); objects: a list that receives the kept Model and DeviceCSR.  Returns the last state."""
    kept_model = cu.Model(tr.rows, tr.cols, f, tr.global_bias) if state is None else model_from(state, tr.global_bias)
    kept_csr = cu.DeviceCSR(tr)
    if objects is not None:
        objects += [kept_model, kept_csr]
    state = kept_model.download()
    for k, step in enumerate(steps):
        on_kept = step(kept_model, kept_csr)
        fresh = model_from(state, tr.global_bias)
        on_fresh = step(fresh, cu.DeviceCSR(tr))
        state = fresh.download()
        assert same_state(kept_model.download(), state), ("step %d differs on the shared objects" % k)
        assert on_kept == on_fresh, ("step %d returns something else on the shared objects" % k, on_kept, on_fresh)
    return state


# ---- rating sets -----------------------------------------------------------------------------------------------------------
def csr_from_rows(per_row, cols, ratings_rng, gb=None, ratings=None):
    """per_row: one array of partner ids per row (in the order given).  Ratings: half stars 0.5 .. 5 unless given."""
    lengths = [len(p) for p in per_row]
    indptr = np.zeros(len(per_row) + 1, np.int64)
    indptr[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.asarray(p, np.int32) for p in per_row]) if per_row else np.zeros(0, np.int32)
    if ratings is None:
        ratings = ratings_rng.integers(1, 11, len(idx)).astype(np.float32) / 2
    if gb is None:
        gb = float(np.float32(ratings.astype(np.float64).mean())) if len(idx) else 0.0
    return api.HostCSR(indptr, idx, ratings, len(per_row), cols, gb)


WIDTH_LENGTHS = [1, 2, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
SHORT_ROWS = 200


def width_length_set(extra_long=False):
    """Row-major set of section B.1: row i has WIDTH_LENGTHS[i] ratings of distinct partners (ascending), then SHORT_ROWS rows of
    1 .. 64 ratings; with extra_long one more row of 64 x 1024 + 1 ratings (chunks longer than 1,024)."""
    key = ("wl", extra_long)
    if key not in _CACHE:
        rng = np.random.default_rng(71 + extra_long)
        lengths = WIDTH_LENGTHS + ([64 * 1024 + 1] if extra_long else []) + [1 + (i % 64) for i in range(SHORT_ROWS)]
        cols = max(lengths) + 40
        per_row = [np.sort(rng.choice(cols, n, replace=False)) for n in lengths]
        _CACHE[key] = csr_from_rows(per_row, cols, rng)
    return _CACHE[key]


def batch_set(n_long, chunks_each):
    """Section B.4, row-major: n_long rows of exactly `chunks_each` chunks, then 64 rows of 1 .. 64 ratings."""
    key = ("batch", n_long, chunks_each)
    if key not in _CACHE:
        rng = np.random.default_rng(91 + chunks_each)
        n = chunks_each * api.ALS_CHUNK if chunks_each == api.ALS_MAX_CHUNKS else (chunks_each - 1) * api.ALS_CHUNK + 1
        cols = n + 100
        per_row = [np.sort(rng.choice(cols, n, replace=False)) for _ in range(n_long)]
        per_row += [np.sort(rng.choice(cols, 1 + i, replace=False)) for i in range(64)]
        _CACHE[key] = csr_from_rows(per_row, cols, rng)
    return _CACHE[key]


def chunks_of(n):
    """How many chunks a row of n ratings is cut into (the arithmetic of the header's CU2REC_ALS_* constants)."""
    if n <= api.ALS_CHUNK:
        return 0
    c = min(-(-n // api.ALS_CHUNK), api.ALS_MAX_CHUNKS)
    per = -(-(-(-n // c)) // api.ALS_STEP) * api.ALS_STEP
    return -(-n // per)


class Case:
    """One half-step of section B.3 in row-major form: `csr` has the solved side as rows and the partners as columns."""

    def __init__(self, name, csr, X, xb, Y, yb, reg, reg_b, other_regs, classes, singular=False):
        self.name, self.csr, self.X, self.xb, self.Y, self.yb = name, csr, X, xb, Y, yb
        self.reg, self.reg_b, self.other_regs, self.classes, self.singular = reg, reg_b, other_regs, classes, singular
        self.class_of = {int(r): c for c, rs in classes.items() for r in rs}

    def well_conditioned(self):
        """Rows on which the forward bar is in force beside the residual bound: the classes of ordinary partners (short,
        f_plus_5, long) of every case but `singular`.  Two exceptions, both by conditioning and not by what any code returns:
        at factor regulariser 1e-4 a row with fewer ratings than factors has cond(A) ~ |z|^2 / reg ~ 1e5, so u cond(A) is
        several 1e-3 and the 1e-3 bar cannot be promised (the float32 restatement reaches 0.77 of it at f = 100): there the bar
        holds on f_plus_5 and long only.  The classes built to be badly conditioned or badly scaled (same_row, repeat_40, down,
        up) are judged by the residual bound alone in every case.  tests/test_als_cpu.py shows that the float32 restatement
        meets the bar on exactly this mask."""
        mask = np.zeros(self.csr.rows, bool)
        if self.singular:
            return mask
        for c in ("f_plus_5", "long") if self.name == "reg_1e-4" else ("short", "f_plus_5", "long"):
            mask[list(self.classes.get(c, ()))] = True
        return mask

    def for_side(self, side):
        """(csr, state, hyper, gb) for a GPU half-step of `side`: row-major as it is for users, transposed for items."""
        lr = 0.01
        if side == "users":
            hyper = (lr, self.reg, self.other_regs[0], self.reg_b, self.other_regs[1])
            return self.csr, (self.Y, self.X, self.yb, self.xb), hyper
        hyper = (lr, self.other_regs[0], self.reg, self.other_regs[1], self.reg_b)
        return self.csr.transpose(), (self.X, self.Y, self.xb, self.yb), hyper


def conditioning_cases(f):
    """The labelled row classes of section B.3 at width f, one Case per regulariser / magnitude setting.

    Partners 0 .. 3999 are ordinary (factors O(0.3), biases O(0.1)); 4000 .. 4099 are 100 ids that share ONE factor row;
    4100 .. 4299 are ordinary rows scaled by 2^-20; 4300 .. 4499 by 2^10.  Classes (every one with rows of 1 .. 64 ratings next
    to its long ones):
      short      1, 2, ..., 64 ratings of distinct ordinary partners (fewer ratings than factors at f = 100)
      f_plus_5   f + 5 ratings;  long: 1,025 and 2,049 ratings
      same_row   1, 2, 7, 40, 64, 100 ratings of distinct ids that all hold the same factor row (a rank-1 factor Gram)
      repeat_40  one partner named 40 times (and 1, 2, 64, 1,100 times), with different ratings
      down / up  1, 2, 33, 64, 200 ratings of partners scaled by 2^-20 / 2^10
    Cases: base (four regularisers pairwise a factor >= 3 apart); bias0 (bias regulariser exactly 0); reg_1e-4 and reg_10 (the
    factor regulariser); cancel (ratings of 1e4 with global bias 1e4 - 3); singular (f = 100 only: factor regulariser 1e-7 on
    same_row / repeat rows with partner entries of O(1)).
    Every case holds every class, with one exception found with the float32 restatement (als_reference64.solve_row_f32), not
    assumed: `up` is solved only under reg_10.  At factor regulariser 0.05 (base, bias0, cancel) its 1- and 2-rating rows at
    f = 100 have |z|^2 ~ 1e7 against n reg ~ 0.05 -- u cond(A) > 1 -- and the restatement meets a non-positive pivot; at 1e-4
    so do the rows of up to 64 ratings, and the 1- and 2-rating rows at f = 8 as well.  Those are singular systems to float32, not
    the finite-Gram magnitude check the class is for, so they are left to reg_10 (cond(A) ~ 1e6)."""
    if ("cond", f) in _CACHE:
        return _CACHE[("cond", f)]
    rng = np.random.default_rng(300 + f)
    n_part = 4500
    X = rng.normal(0, 0.3, (n_part, f)).astype(np.float32)
    xb = rng.normal(0, 0.1, n_part).astype(np.float32)
    X[4000:4100] = X[4000]
    X[4100:4300] *= np.float32(2.0 ** -20)
    X[4300:4500] *= np.float32(2.0 ** 10)

    def pick(lo, hi, n):
        return np.sort(rng.choice(np.arange(lo, hi), n, replace=False))

    groups = {
        "short": [pick(0, 4000, n) for n in range(1, 65)],
        "f_plus_5": [pick(0, 4000, f + 5) for _ in range(3)],
        "long": [pick(0, 4000, n) for n in (1025, 2049)],
        "same_row": [pick(4000, 4100, n) for n in (1, 2, 7, 40, 64, 100)],
        "repeat_40": [np.full(n, p) for n, p in ((40, 17), (1, 18), (2, 19), (64, 20), (1100, 21))],
        "down": [pick(4100, 4300, n) for n in (1, 2, 33, 64, 200)],
        "up": [pick(4300, 4500, n) for n in (1, 2, 33, 64, 200)],
    }

    def build(names, seed, ratings=None, gb=None):
        per_row, classes = [], {}
        for c in names:
            classes[c] = list(range(len(per_row), len(per_row) + len(groups[c])))
            per_row += groups[c]
        r = np.random.default_rng(seed)
        csr = csr_from_rows(per_row, n_part, r, gb=gb,
                            ratings=None if ratings is None else ratings(r, sum(len(p) for p in per_row)))
        Y = r.normal(0, 0.3, (len(per_row), f)).astype(np.float32)  # not the solution: an unchanged row is observable
        yb = r.normal(0, 0.1, len(per_row)).astype(np.float32)
        return csr, Y, yb, classes

    everything = ["short", "f_plus_5", "long", "same_row", "repeat_40", "down", "up"]
    cases = []
    for name, names, reg, reg_b, kw in (
            ("base", everything[:-1], 0.05, 0.015, {}),
            ("bias0", everything[:-1], 0.05, 0.0, {}),
            ("reg_1e-4", everything[:-1], 1e-4, 0.015, {}),
            ("reg_10", everything, 10.0, 0.6, {}),
            ("cancel", everything[:-1], 0.05, 0.015,
             {"ratings": lambda r, n: (1e4 + r.integers(-4, 5, n) / 2).astype(np.float32), "gb": 1e4 - 3})):
        csr, Y, yb, classes = build(names, 400 + len(cases), **kw)
        cases.append(Case(name, csr, X, xb, Y, yb, reg, reg_b, (0.2, 2.5), classes))
    if f == 100:
        Xs = X.copy()
        Xs[4000:4100] = rng.normal(0, 1.0, f).astype(np.float32)  # entries of O(1)
        groups["same_row"] += [pick(4000, 4100, 100) for _ in range(2)]
        groups["repeat_40"] = [np.full(n, p) for n, p in ((40, 4017), (1, 4018), (2, 4019), (64, 4020), (1100, 4021))]
        csr, Y, yb, classes = build(["same_row", "repeat_40"], 499)
        cases.append(Case("singular", csr, Xs, xb, Y, yb, 1e-7, 0.015, (0.2, 2.5), classes, singular=True))
    _CACHE[("cond", f)] = cases
    return cases
