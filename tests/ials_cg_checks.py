"""TEST INFRASTRUCTURE shared by tests/test_gpu_ials_cg.py and tests/test_ials_cg_cpu.py: the entry sets of the conjugate-gradient
half-step's GPU tests (the CPU suite runs the float32 restatement on every judged row of every one of them, to show that they
are fair, and five deliberate mistakes in float64, to show that they can tell), and the judgement of one GPU half-step against
the float64 iteration of tests/ials_cg_reference64.py.  Nothing here needs a GPU to be imported."""
import ctypes as C

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib

import als_checks as achk
import ials_cg_reference64 as cgref
import ials_checks as chk
import ials_reference64 as ref
from als_checks import q_padding, same_bits
from ials_checks import HYPER, Case, bar_ratio

# 1, 8, 31, 100, 252 and both edges of every per-lane element count of the kernel (als_cg.hip: lane l owns elements l, l + 64, ...:
# E = ceil(f / 64) = 1 .. 4); 128 | 129 is also where G0 leaves LDS for L2
WIDTHS = [1, 8, 31, 100, 252, 63, 64, 65, 127, 128, 129, 191, 192, 193]
STEPS = (1, 2, 3)
CHUNK = api.ALS_CHUNK
SLOTS = 4            # rows (wavefronts) per workgroup of the CG kernel
GRID_PASS = 4 * 2048  # rows one trip of its grid-stride loop covers
_CACHE = {}


def cases():
    """name -> ials_checks.Case: every width x als_checks.width_length_set() on both sides at alpha 40, and the messy set (entries of
    0, repeated pairs, rows without entries) at alpha 40 and 0."""
    if "cases" not in _CACHE:
        out = {}
        rows_major = achk.width_length_set()
        for f in WIDTHS:
            out["lengths-f%d-users" % f] = Case("lengths-f%d-users" % f, rows_major, "users", f, 40.0, HYPER, 7000 + f)
            out["lengths-f%d-items" % f] = Case("lengths-f%d-items" % f, rows_major.transpose(), "items", f, 40.0, HYPER, 7500 + f)
        for alpha in (40.0, 0.0):
            for side in ("users", "items"):
                name = "messy-alpha%d-f8-%s" % (alpha, side)
                out[name] = Case(name, chk.messy_set(), side, 8, alpha, HYPER, 7900)
        _CACHE["cases"] = out
    return _CACHE["cases"]


def cg_rows_of(indptr):
    """The rows the CG iteration treats: 1 .. CHUNK entries."""
    n = np.diff(indptr)
    return np.flatnonzero((n > 0) & (n <= CHUNK))


def reference(case, steps=max(STEPS)):
    """(rows, [x after 1 step, ..., x after `steps` steps]) of the case's CG rows in float64 from case.state(), computed once."""
    key = ("ref", case.name, steps)
    if key not in _CACHE:
        state = case.state()
        indptr, indices, data, X, reg = case.system_of(state)
        rows = cg_rows_of(indptr)
        x0 = state[0 if case.side == "users" else 1]
        _CACHE[key] = (rows, cgref.cg_rows_upto(indptr, indices, data, X, reg, case.alpha, x0, steps, rows=rows))
    return _CACHE[key]


def ials_cg(model, d_csr, hyper, alpha, side, steps):
    n = C.c_int(-1)
    h = cu.Hyper(*[float(x) for x in hyper])
    s = api.SIDES[side] if isinstance(side, str) else side
    rc = lib().cu2rec_model_als_implicit_cg(model._h, d_csr._h, C.byref(h), float(alpha), s, int(steps), C.byref(n))
    return rc, n.value


def check_cg_half_step(model, d_csr, csr, side, hyper, alpha, steps, report=None, may_fail=None, want=None):
    """One GPU CG half-step against the float64 iteration from the same float32 state; returns the state after it.
    ials_checks.check_half_step's state checks: the other side, the model rows past the CSR (factors and biases) and Q's padding
    keep their bits; inside the CSR the solved side's biases are +0.0 and rows without entries exactly zero.  Every row of
    1 .. CHUNK entries is within 1e-3 max(1, |x*|_inf) of x*, the float64 CG iterate after `steps` steps from the row's float32
    factors; every longer row within the same bar of the exact float64 optimum (the kernels solve those exactly).
    may_fail / report: as in ials_checks.check_half_step.  want: (rows, x*) of the CG rows where the caller has them."""
    f = model.n_factors
    before = model.download()
    pad_before = q_padding(model, f)
    rc, unsolved = ials_cg(model, d_csr, hyper, alpha, side, steps)
    assert rc == 0, (rc, lib().cu2rec_last_error())
    got = model.download()
    own, other = ((0, 2), (1, 3)) if side == "users" else ((1, 3), (0, 2))
    n_own = csr.rows if side == "users" else csr.cols
    for k in other:
        assert same_bits(got[k], before[k]), "the other side moved (%s half-step, f=%d)" % (side, f)
    for k in own:
        assert same_bits(got[k][n_own:], before[k][n_own:]), "model rows past the CSR moved (%s, f=%d)" % (side, f)
    pad = q_padding(model, f)
    assert not pad[:csr.cols].any() and same_bits(pad[csr.cols:], pad_before[csr.cols:])
    if side == "users":
        assert same_bits(pad, pad_before)
    indptr, indices, data, n_part = ref.own_major(csr, side)
    rated = np.flatnonzero(np.diff(indptr) > 0)
    if may_fail is None:
        assert unsolved == 0, (side, f, unsolved)
        kept = np.zeros(0, np.int64)
    else:
        x_all = np.concatenate([got[own[0]], got[own[1]][:, None]], axis=1)[rated]
        x0_all = np.concatenate([before[own[0]], before[own[1]][:, None]], axis=1)[rated]
        kept = rated[(np.ascontiguousarray(x_all).view(np.uint32) == np.ascontiguousarray(x0_all).view(np.uint32)).all(axis=1)]
        assert unsolved == len(kept), (side, f, unsolved, kept[:8].tolist())
        stray = np.setdiff1d(kept, np.asarray(list(may_fail), np.int64))
        assert len(stray) == 0, ("rows left unsolved that should have been solved", side, f, stray[:8].tolist())
    done = np.setdiff1d(np.arange(n_own), kept)
    assert same_bits(got[own[1]][done], np.zeros(len(done), np.float32)), "a solved bias is not +0.0"
    empty = np.flatnonzero(np.diff(indptr) == 0)
    assert same_bits(got[own[0]][empty], np.zeros((len(empty), f), np.float32)), "a row without entries is not the zero row"
    X, reg = before[other[0]][:n_part], hyper[1 if side == "users" else 2]
    if want is None:
        rows = cg_rows_of(indptr)
        want = (rows, cgref.cg_rows(indptr, indices, data, X, reg, alpha, before[own[0]], steps, rows=rows))
    rows, xs = want
    judged = ~np.isin(rows, kept)
    worst = bar_ratio(got[own[0]][rows[judged]], xs[judged])
    long_rows = np.setdiff1d(np.setdiff1d(rated, rows), kept)
    worst_long = bar_ratio(got[own[0]][long_rows], ref.solve_rows(indptr, indices, data, X, reg, alpha, rows=long_rows))
    if report is not None:
        report[(side, f, steps)] = worst
        report[(side, f, "long")] = worst_long
        if may_fail is not None:
            report["unsolved"], report["kept"] = unsolved, kept
    assert worst <= 1.0, ("rows off the float64 CG iterate, in units of the bar", side, f, steps, worst)
    assert worst_long <= 1.0, ("long rows off the float64 optimum, in units of the bar", side, f, worst_long)
    return got


# ---- rows that cannot be solved: the bad entry makes every sum it enters non-finite -----------------------------------------
def unsolved_cases():
    """name -> (Case, rows of the case's side that hold the bad entry): ials_checks' poison-entry and overflow sets at f = 8 and
    100 on both sides.  The negative-weight set is not used: CG does not promise to detect an indefinite system."""
    return {name: v for name, v in chk.unsolved_cases().items() if not name.startswith("negative")}


# ---- many short rows: more than one trip of the kernel's grid-stride loop ---------------------------------------------------------
def many_rows_set():
    """20,000 rows of 1 .. 4 entries over 50 items (GRID_PASS = 8,192 rows per trip)."""
    if "many" not in _CACHE:
        rng = np.random.default_rng(20000)
        lengths = 1 + (np.arange(20000) % 4)
        per_row = [np.sort(rng.choice(50, n, replace=False)) for n in lengths]
        _CACHE["many"] = achk.csr_from_rows(per_row, 50, rng)
    return _CACHE["many"]


MANY_ROWS_F, MANY_ROWS_SEED = 8, 2020


def many_rows_sample():
    """The rows of many_rows_set() that are judged in float64: every 97th, both sides of every trip's edge, the last row."""
    rows = many_rows_set().rows
    edges = [GRID_PASS - 1, GRID_PASS, 2 * GRID_PASS - 1, 2 * GRID_PASS, rows - 1]
    return edges, np.unique(np.concatenate([np.arange(0, rows, 97), edges]))
