"""TEST INFRASTRUCTURE shared by tests/test_gpu_als_cg.py and tests/test_als_cg_cpu.py: the rating sets of the explicit
conjugate-gradient half-step's GPU tests (the CPU suite runs the float32 restatement on every judged row of every one of them, to
show that they are fair, and seven deliberate mistakes in float64, to show that they can tell), and the judgement of one GPU
half-step against the float64 iteration of tests/als_cg_reference64.py.  Nothing here needs a GPU to be imported."""
import ctypes as C

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib

import als_checks as achk
import als_cg_reference64 as cgref
import als_reference64 as ref
import ials_checks as ichk
from als_checks import own_major, q_padding, same_bits
from ials_cg_checks import GRID_PASS, SLOTS, many_rows_sample, many_rows_set  # the same launch: 4 rows per workgroup, 2,048 workgroups
from ials_checks import bar_ratio

# 1, 8, 31, 100, 252 and both edges of every per-lane element count of the kernel (als_cg.hip: lane l owns elements l, l + 64, ... of
# the order-(f + 1) vectors: E = ceil((f + 1) / 64) = 1 .. 4).  Together f = 0, 1, 2, 3 mod 4: where the synthesised column f sits in
# its float4, f = 8, 64, 100, 128, 192, 252 being the widths at which it starts one of its own.
WIDTHS = [1, 8, 31, 100, 252, 62, 63, 64, 126, 127, 128, 190, 191, 192]
STEPS = (1, 2, 3)
CHUNK = api.ALS_CHUNK
HYPER = achk.HYPER
MANY_ROWS_F, MANY_ROWS_SEED = 8, 2021
_CACHE = {}


class Case:
    """One half-step: `csr` is what the model is trained on (user-major), `side` the side solved, from `state` (float32 P, Q,
    user_bias, item_bias; default: random factors of O(0.3) and biases of O(0.1) with model rows past the CSR on both sides)."""

    def __init__(self, name, csr, side, f, hyper, seed=None, state=None):
        self.name, self.csr, self.side, self.f, self.hyper, self.seed, self._state = name, csr, side, f, hyper, seed, state

    def state(self):
        if self._state is not None:
            return tuple(a.copy() for a in self._state)
        return achk.random_state(self.csr.rows + 3, self.csr.cols + 5, self.f, self.seed)

    def system_of(self, state):
        """(indptr, indices, data, X, xb, gb, reg, reg_b, x0): the arguments of als_cg_reference64.cg_rows_upto up to x0."""
        P, Q, ub, ib = state
        indptr, indices, data = own_major(self.csr, self.side)
        _, P_reg, Q_reg, ubr, ibr = self.hyper
        if self.side == "users":
            return indptr, indices, data, Q, ib, self.csr.global_bias, P_reg, ubr, cgref.start(P, ub)
        return indptr, indices, data, P, ub, self.csr.global_bias, Q_reg, ibr, cgref.start(Q, ib)


def cases():
    """name -> Case: every width x als_checks.width_length_set() on both sides, and the messy set (repeated pairs, empty rows,
    unsorted items) at f = 8 on both sides."""
    if "cases" not in _CACHE:
        out = {}
        rows_major = achk.width_length_set()
        for f in WIDTHS:
            out["lengths-f%d-users" % f] = Case("lengths-f%d-users" % f, rows_major, "users", f, HYPER, 8000 + f)
            out["lengths-f%d-items" % f] = Case("lengths-f%d-items" % f, rows_major.transpose(), "items", f, HYPER, 8500 + f)
        for side in ("users", "items"):
            out["messy-f8-%s" % side] = Case("messy-f8-%s" % side, ichk.messy_set(), side, 8, HYPER, 8900)
        _CACHE["cases"] = out
    return _CACHE["cases"]


def cg_rows_of(indptr):
    """The rows the CG iteration treats: 1 .. CHUNK ratings."""
    n = np.diff(indptr)
    return np.flatnonzero((n > 0) & (n <= CHUNK))


ONE_RATING_UNFAIR_FROM = 31


def fair_rows(case, steps):
    """The CG rows of `case` that are held to the bar after `steps` steps: all of them, except that from f = 31 on a row of ONE
    rating is not judged at three steps.  Its system z z^T + diag(reg, ..., reg, reg_bias) has exactly three distinct eigenvalues
    -- reg on everything orthogonal to [q; 0] and [0; 1], and the two of that plane, about |q|^2 + 1 and
    (reg + reg_bias |q|^2) / (|q|^2 + 1) -- so the third step is the one that ends the iteration, and it has to tell reg = 0.05 from
    a neighbour between 0.02 and 0.05 in a residual that two steps have already brought down by |q|^2 / reg, |q|^2 = 0.09 f.  Where
    that leaves the set is read off the float32 restatement of tests/als_cg_reference64.py, width by width, and
    tests/test_als_cg_cpu.py asserts it per set: on these rows at three steps it uses 0.14 and 0.44 of the bar at f = 8 (judged),
    0.85 and 1.01 at f = 31, and 2.3 .. 72 bars from f = 62 to 252 (more than the half a set may use: not judged); 9e-3 after two
    steps at every width.  At f = 1 the system has order 2 and is solved after two steps.  The rows left out must still come back
    finite and counted as solved."""
    indptr = own_major(case.csr, case.side)[0]
    rows = cg_rows_of(indptr)
    if steps >= 3 and case.f >= ONE_RATING_UNFAIR_FROM:
        rows = rows[np.diff(indptr)[rows] > 1]
    return rows


def reference(case, steps=max(STEPS)):
    """(rows, [x after 1 step, ..., x after `steps` steps]) of the case's CG rows in float64 from case.state(), computed once."""
    key = ("ref", case.name, steps)
    if key not in _CACHE:
        args = case.system_of(case.state())
        rows = cg_rows_of(args[0])
        _CACHE[key] = (rows, cgref.cg_rows_upto(*args, steps, rows=rows))
    return _CACHE[key]


# ---- conditioning: als_checks.conditioning_cases(8) ------------------------------------------------------------------------------
# The cases the issue names (bias regulariser 0; factor regulariser 1e-4 and 10; partners scaled by 2^-20 and 2^10 are the classes
# `down` and `up` inside them), every row class of theirs that has CG rows, at 1, 2 and 3 steps.  A (case, class, steps) is held to
# the bar on the GPU unless the float32 restatement of tests/als_cg_reference64.py itself uses more than half the bar there:
# tests/test_als_cg_cpu.py asserts at most 0.5 on every judged one AND more than 0.5 on every one listed here, so the list is read
# off the restatement and not argued.  What it shows: at factor regulariser 1e-4 a row with fewer ratings than unknowns, or with a
# rank-1 Gram, has cond(A) ~ |z|^2 / reg ~ 1e4, and the third step cubes it (372 .. 810 bars); partners x 2^10 have |z|^2 ~ 1e6 against
# n reg = 10 n, and already the second step squares 1e5 (6 and 83 bars).  The rows left out must still come back finite and solved.
CONDITIONING_F = 8
CONDITIONING_CASES = ("bias0", "reg_1e-4", "reg_10")
CONDITIONING_UNFAIR = {("reg_1e-4", "short", 3), ("reg_1e-4", "same_row", 3), ("reg_1e-4", "repeat_40", 3), ("reg_10", "up", 2),
                       ("reg_10", "up", 3)}


def conditioning_cases():
    """name -> (Case, {steps: rows judged}, {class: its CG rows}, the als_checks case's name) on both sides."""
    if "cond" not in _CACHE:
        out = {}
        for c in achk.conditioning_cases(CONDITIONING_F):
            if c.name not in CONDITIONING_CASES:
                continue
            for side in ("users", "items"):
                csr, state, hyper = c.for_side(side)
                cg = cg_rows_of(own_major(csr, side)[0])
                classes = {cls: np.intersect1d(rs, cg) for cls, rs in c.classes.items()}
                classes = {cls: rs for cls, rs in classes.items() if len(rs)}
                judged = {s: np.array(sorted(r for cls, rs in classes.items() if (c.name, cls, s) not in CONDITIONING_UNFAIR for r in rs),
                                      np.int64) for s in STEPS}
                name = "%s-%s" % (c.name, side)
                out[name] = (Case(name, csr, side, CONDITIONING_F, hyper, state=state), judged, classes, c.name)
        _CACHE["cond"] = out
    return _CACHE["cond"]


# ---- rows that cannot be solved -----------------------------------------------------------------------------------------------
UNSOLVED_WIDTHS = (8, 100)
OVERFLOW = 3e38  # finite in float32; times a residual of O(1) it is not


def unsolved_cases():
    """name -> (Case, rows of the case's side that cannot be solved, rows whose own start holds a NaN): the messy set with one rating
    NaN (ials_checks.poison_entry_set; its second bad rating is +inf) and one PARTNER row whose first factor is 3e38 -- every row
    that names that partner overflows in its first operator application.  Three other rows of the solved side start from a NaN of
    their own (a factor, the bias, both): they are solved from zero."""
    if "unsolved" not in _CACHE:
        out = {}
        csr, entries = ichk.poison_entry_set()
        for f in UNSOLVED_WIDTHS:
            for side in ("users", "items"):
                indptr, indices, _ = own_major(csr, side)
                bad = set(ichk.rows_of_entries(csr, side, entries).tolist())
                counts = np.bincount(indices, minlength=csr.cols if side == "users" else csr.rows)
                partner = int(np.flatnonzero((counts >= 2) & (counts <= 60))[3])
                owners = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
                bad |= set(owners[indices == partner].tolist())
                P, Q, ub, ib = achk.random_state(csr.rows + 3, csr.cols + 5, f, 8600 + f)
                (Q if side == "users" else P)[partner, 0] = OVERFLOW
                Y, yb = (P, ub) if side == "users" else (Q, ib)
                rated = np.flatnonzero(np.diff(indptr) > 0)
                nan_start = [int(r) for r in rated if r not in bad][5:8]
                Y[nan_start[0], f - 1] = np.nan
                yb[nan_start[1]] = np.nan
                Y[nan_start[2], 0], yb[nan_start[2]] = np.inf, np.nan
                name = "unsolved-f%d-%s" % (f, side)
                out[name] = (Case(name, csr, side, f, HYPER, state=(P, Q, ub, ib)), np.array(sorted(bad), np.int64), nan_start)
        _CACHE["unsolved"] = out
    return _CACHE["unsolved"]


# ---- the GPU call and its judgement ---------------------------------------------------------------------------------------------
def als_cg(model, d_csr, hyper, side, steps):
    n = C.c_int(-1)
    h = cu.Hyper(*[float(x) for x in hyper])
    s = api.SIDES[side] if isinstance(side, str) else side
    rc = lib().cu2rec_model_als_cg(model._h, d_csr._h, C.byref(h), s, int(steps), C.byref(n))
    return rc, n.value


def check_cg_half_step(model, case, d_csr, steps, want=None, judged=None, may_fail=None, report=None, judge_long=True):
    """One GPU CG half-step of `case` against the float64 iteration from the same float32 state; returns the state after it.
    Always: return code 0; the other side, rows without ratings, model rows past the CSR and Q's padding floats keep their bits.
    Every judged row of 1 .. CHUNK ratings is within 1e-3 max(1, |x*|_inf) of x* = [factors; bias], the float64 CG iterate after
    `steps` steps from the row's float32 values; every longer row within the same bar of the exact float64 optimum.
    want: (rows, x*) of the CG rows where the caller has them.  judged: the CG rows held to the bar (default: all; the others must
    still be finite).  may_fail: None -- `unsolved` must be 0; otherwise the rows allowed to be left unsolved: `unsolved` must
    equal the number of rated rows that kept their bits, each of them listed.  report: receives the worst ratios.  judge_long: False
    where the set's long rows are built to be badly conditioned (tests/test_gpu_als_edges.py judges those, by their residual)."""
    csr, side, f, hyper = case.csr, case.side, model.n_factors, case.hyper
    before = model.download()
    pad_before = q_padding(model, f)
    rc, unsolved = als_cg(model, d_csr, hyper, side, steps)
    assert rc == 0, (rc, lib().cu2rec_last_error())
    got = model.download()
    own, other = ((0, 2), (1, 3)) if side == "users" else ((1, 3), (0, 2))
    for k in other:
        assert same_bits(got[k], before[k]), "the other side moved (%s half-step, f=%d)" % (side, f)
    indptr, indices, data, X, xb, gb, reg, reg_b, x0 = case.system_of(before)
    rated = np.flatnonzero(np.diff(indptr) > 0)
    untouched = np.setdiff1d(np.arange(len(before[own[1]])), rated)
    for k in own:  # rows without ratings, and model rows past the CSR, keep their values bit for bit
        assert same_bits(got[k][untouched], before[k][untouched]), (side, f)
    assert same_bits(q_padding(model, f), pad_before) and not pad_before.any()
    x_all = np.concatenate([got[own[0]], got[own[1]][:, None]], axis=1)
    x0_all = np.concatenate([before[own[0]], before[own[1]][:, None]], axis=1)
    kept = rated[(np.ascontiguousarray(x_all[rated]).view(np.uint32) == np.ascontiguousarray(x0_all[rated]).view(np.uint32)).all(axis=1)]
    if may_fail is None:
        assert unsolved == 0, (side, f, steps, unsolved)
        kept = np.zeros(0, np.int64)  # a row that kept its bits without being counted is judged like any other
    else:
        assert unsolved == len(kept), (side, f, unsolved, kept[:8].tolist())
        stray = np.setdiff1d(kept, np.asarray(list(may_fail), np.int64))
        assert len(stray) == 0, ("rows left unsolved that should have been solved", side, f, stray[:8].tolist())
    solved = np.setdiff1d(rated, kept)
    assert np.isfinite(x_all[solved]).all(), (side, f, solved[~np.isfinite(x_all[solved]).all(axis=1)][:8].tolist())
    if want is None:
        rows = cg_rows_of(indptr)
        want = (rows, cgref.cg_rows(indptr, indices, data, X, xb, gb, reg, reg_b, x0, steps, rows=rows))
    rows, xs = want
    on = ~np.isin(rows, kept)
    if judged is not None:
        on &= np.isin(rows, judged)
    worst = bar_ratio(x_all[rows[on]], xs[on])
    long_rows = np.setdiff1d(np.setdiff1d(rated, cg_rows_of(indptr)), kept)
    exact = np.array([np.linalg.solve(*ref.system(indptr, indices, data, np.asarray(X, np.float64), np.asarray(xb, np.float64), gb, reg,
                                                  reg_b, int(r))) for r in long_rows]).reshape(len(long_rows), f + 1)
    worst_long = bar_ratio(x_all[long_rows], exact) if judge_long else 0.0
    if report is not None:
        report[(side, f, steps)] = worst
        report[(side, f, "long")] = worst_long
        report["unsolved"], report["kept"] = unsolved, kept
    assert worst <= 1.0, ("rows off the float64 CG iterate, in units of the bar", case.name, steps, worst)
    assert worst_long <= 1.0, ("long rows off the float64 optimum, in units of the bar", case.name, worst_long)
    return got
