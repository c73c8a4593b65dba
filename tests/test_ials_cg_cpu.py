"""The conjugate-gradient implicit half-step without a GPU: its float64 reference (tests/ials_cg_reference64.py) against
numpy.linalg.solve, the fairness of the GPU test sets (tests/ials_cg_checks.py: a float32 restatement in operator form meets the
bar on every judged row; five deliberate mistakes do not), five sweeps of the restatement on ML_SMALL, and the declarations.

The bar is the project's: max |x - x*| <= 1e-3 max(1, |x*|_inf), x* the float64 CG iterate at the same step count from the same
float32 state."""
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import SIGNATURES
from conftest import ROOT, ml_small

import als_checks as achk
import ials_cg_checks as cgchk
import ials_cg_reference64 as cgref
import ials_checks as chk
import ials_reference64 as ref

def claimed(mutation, case):
    """Whether the GPU set `case` is claimed to see `mutation` at 3 steps.  One step too few and the cold start cannot be seen at
    f = 1, where the first CG step is exact from any start.  The regulariser left out of the matvec is claimed on the messy sets
    only (60 and 150 partners: G0's diagonal is of the regulariser's order; measured 11 .. 226 bars): on the width x length sets
    G0's diagonal is 370 against a regulariser of 0.8 or 1.2, and three steps move no row by more than 0.88 .. 2 bars."""
    if mutation == "no_reg":
        return case.name.startswith("messy")
    if mutation in ("steps_minus_1", "cold_start"):
        return case.f != 1
    return True


@pytest.mark.parametrize("f", [8, 100, 252])
def test_f_steps_of_cg_are_the_exact_solution(f):
    """In exact arithmetic CG ends after f steps; in float64 on these systems (condition numbers <= 34) it is within 1e-6 of the
    bar -- 1e-9 absolute, seven orders above float64 rounding x the condition number -- of numpy.linalg.solve."""
    worst = 0.0
    for side in ("users", "items") if f == 8 else ("users",):
        case = cgchk.cases()["lengths-f%d-%s" % (f, side)]
        state = case.state()
        indptr, indices, data, X, reg = case.system_of(state)
        rows = cgchk.cg_rows_of(indptr)
        G0 = ref.gram64(X)
        got = cgref.cg_rows(indptr, indices, data, X, reg, case.alpha, state[0 if side == "users" else 1], f, rows=rows, G0=G0)
        want = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows, G0=G0)
        worst = max(worst, chk.bar_ratio(got, want))
    print("f=%d: %d steps of float64 CG at %.3g of the bar from numpy.linalg.solve" % (f, f, worst))
    assert worst <= 1e-6, (f, worst)


def test_reference_stops_and_fails_as_written():
    """f = 1: the first step is exact, the later ones stop on rho == 0 or move nothing; a start that is not finite is the zero
    start; an entry that is not finite leaves the row unsolved (NaN); a row without entries is the zero row."""
    X = np.array([[0.5], [0.25], [-1.0]], np.float32)
    indptr, indices = np.array([0, 2, 2, 3]), np.array([0, 2, 1])
    data = np.array([1.0, 2.0, np.inf])
    x0 = np.array([[0.3], [0.7], [0.1]], np.float32)
    A, b = ref.row_system(indptr, indices, data, X, 0.5, 2.0, 0, ref.gram64(X))
    for steps in (1, 5):
        out = cgref.cg_rows(indptr, indices, data, X, 0.5, 2.0, x0, steps)
        assert abs(out[0, 0] - b[0] / A[0, 0]) <= 1e-15 and out[1, 0] == 0.0 and np.isnan(out[2, 0])
    bad = x0.copy()
    bad[0, 0] = np.nan
    assert np.array_equal(cgref.cg_rows(indptr, indices, data, X, 0.5, 2.0, bad, 1)[0], cgref.cg_rows(indptr, indices, data, X, 0.5, 2.0, None, 1)[0])


@pytest.mark.parametrize("name", sorted(cgchk.cases()))
def test_float32_restatement_meets_the_bar_on_every_judged_row(name):
    case = cgchk.cases()[name]
    state = case.state()
    indptr, indices, data, X, reg = case.system_of(state)
    rows, want = cgchk.reference(case)
    assert len(rows) > 0
    got = cgref.cg_rows_f32(indptr, indices, data, X, reg, case.alpha, state[0 if case.side == "users" else 1], max(cgchk.STEPS), rows=rows)
    ratios = [chk.bar_ratio(got[s - 1], want[s - 1]) for s in cgchk.STEPS]
    print("%s: float32 restatement at %s of the bar after 1, 2, 3 steps over %d rows" % (name, ", ".join("%.3g" % r for r in ratios), len(rows)))
    assert max(ratios) <= 0.25, (name, ratios)  # a set above a quarter of the bar would leave the kernel's own order no room


@pytest.mark.parametrize("name", sorted(cgchk.cases()))
def test_five_mistakes_miss_the_bar_on_every_set(name):
    """At 3 steps, per set (at f = 8 a single short row can hide a mistake; the set cannot), on every set claimed() lists.
    Measured: one step too few >= 42 bars, cold start >= 4.2, no G0 >= 142, the right-hand side weighted by w >= 4.8."""
    case = cgchk.cases()[name]
    state = case.state()
    indptr, indices, data, X, reg = case.system_of(state)
    rows, want = cgchk.reference(case)
    x0 = state[0 if case.side == "users" else 1]
    G0 = ref.gram64(X)
    for mutation in cgref.MUTATIONS:
        if not claimed(mutation, case):
            continue
        wrong = cgref.cg_rows(indptr, indices, data, X, reg, case.alpha, x0, 3, mutation=mutation, rows=rows, G0=G0)
        ratio = chk.bar_ratio(wrong, want[2])
        print("%s: %s is %.3g of the bar off" % (name, mutation, ratio))
        assert ratio > 1.0, (name, mutation, ratio)


@pytest.mark.parametrize("name", sorted(cgchk.unsolved_cases()))
def test_restatement_fails_exactly_the_rows_that_hold_the_bad_entry(name):
    case, bad = cgchk.unsolved_cases()[name]
    state = case.state()
    indptr, indices, data, X, reg = case.system_of(state)
    rows = cgchk.cg_rows_of(indptr)
    x0 = state[0 if case.side == "users" else 1]
    got = cgref.cg_rows_f32(indptr, indices, data, X, reg, case.alpha, x0, 3, rows=rows)[-1]
    want = cgref.cg_rows(indptr, indices, data, X, reg, case.alpha, x0, 3, rows=rows)
    failed = rows[np.isnan(got).any(axis=1)]
    assert np.array_equal(failed, np.sort(bad)), (name, failed, bad)
    if name.startswith("poison"):  # (alpha r overflows float32 only: the float64 iterate of an overflow row is finite, and not judged)
        assert np.array_equal(rows[np.isnan(want).any(axis=1)], np.sort(bad)), name
    good = ~np.isin(rows, bad)
    ratio = chk.bar_ratio(got[good], want[good])
    print("%s: float32 restatement at %.3g of the bar on the other %d rows" % (name, ratio, good.sum()))
    assert ratio <= 0.25, (name, ratio)


@pytest.mark.parametrize("f", [8, 100, 252])
def test_forty_steps_of_the_restatement_reach_the_optimum(f):
    case = cgchk.cases()["lengths-f%d-users" % f]
    state = case.state()
    indptr, indices, data, X, reg = case.system_of(state)
    rows = cgchk.cg_rows_of(indptr)
    got = cgref.cg_rows_f32(indptr, indices, data, X, reg, case.alpha, state[0], 40, rows=rows)[-1]
    ratio = chk.bar_ratio(got, ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows))
    print("f=%d: 40 float32 CG steps at %.3g of the bar from the float64 optimum" % (f, ratio))
    assert ratio <= 0.25, (f, ratio)


def test_many_rows_set_takes_more_than_one_grid_pass():
    """And the restatement meets the bar on its judged sample.  Its worst row has ONE entry: the system is G0 + reg I plus a rank-1
    term, two CG steps all but solve it, and the third divides one rounding residue by another -- 0.11 of the bar here against
    3e-3 after two steps; still under the quarter that a set may use."""
    csr = cgchk.many_rows_set()
    assert csr.rows > 2 * cgchk.GRID_PASS and np.diff(csr.indptr).max() <= 4 and np.diff(csr.indptr).min() >= 1
    state = achk.random_state(csr.rows, csr.cols, cgchk.MANY_ROWS_F, cgchk.MANY_ROWS_SEED)
    _, sample = cgchk.many_rows_sample()
    args = (csr.indptr, csr.indices, csr.data, state[1], chk.HYPER[1], 40.0, state[0], 3)
    ratio = chk.bar_ratio(cgref.cg_rows_f32(*args, rows=sample)[-1], cgref.cg_rows(*args, rows=sample))
    print("20,000 rows: float32 restatement at %.3g of the bar over %d sampled rows" % (ratio, len(sample)))
    assert ratio <= 0.25, ratio


def test_five_sweeps_of_the_restatement_on_ml_small():
    """f = 32, 3 steps, from the seed-42-style start: the float64 objective never rises and ends below half its start.  Rows of
    more than 1,024 entries are solved exactly, as the kernels do (ials_reference64.solve_rows_f32)."""
    tr = cu.createSparseMatrix(ml_small())
    f, hyper, alpha = 32, (0.01, 0.1, 0.1, 0.0, 0.0), 40.0
    rng = np.random.default_rng(42)
    P, Q = rng.normal(0, 0.1, (tr.rows, f)).astype(np.float32), rng.normal(0, 0.1, (tr.cols, f)).astype(np.float32)
    L = [ref.objective(tr, P, Q, hyper, alpha)]
    for _ in range(5):
        for side in ("users", "items"):
            indptr, indices, data, n_part = ref.own_major(tr, side)
            own, X, reg = (P, Q[:n_part], hyper[1]) if side == "users" else (Q, P[:n_part], hyper[2])
            G0 = ref.gram_f32(X)
            new = cgref.cg_rows_f32(indptr, indices, data, X, reg, alpha, own, 3, G0=G0)[-1]
            long_rows = np.flatnonzero(np.diff(indptr) > cgref.CHUNK)
            new[long_rows] = ref.solve_rows_f32(indptr, indices, data, X, reg, alpha, rows=long_rows, G0=G0)
            assert np.isfinite(new).all()
            own[:len(new)] = new.astype(np.float32)
            L.append(ref.objective(tr, P, Q, hyper, alpha))
    print("ML_SMALL, f = 32, CG at 3 steps in float32: objective %.6g -> %.6g, last decrease %.3g" % (L[0], L[-1], L[-2] - L[-1]))
    assert all(b <= a for a, b in zip(L, L[1:])), L
    assert L[-1] < 0.5 * L[0], L


def test_declarations():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"enum\s*\{\s*CU2REC_ALS_CG_MAX_STEPS\s*=\s*256\s*\}", header)
    assert re.search(r"int cu2rec_model_als_implicit_cg\(cu2rec_model \*m, const cu2rec_csr \*train, const cu2rec_hyper \*hyper, "
                     r"float alpha, int side,\s*int cg_steps, int \*unsolved\);", header)
    assert re.search(r"int cu2rec_train_implicit_cg\(const cu2rec_csr \*train, cu2rec_config \*cfg, cu2rec_model \*model, float alpha, "
                     r"int cg_steps,\s*int verbose, double \*objectives, cu2rec_train_stats \*stats\);", header)
    assert "does NOT promise to detect an indefinite system" in header and "solved exactly whatever cg_steps is" in header
    assert "cu2rec_model_als_implicit_cg" in SIGNATURES and "cu2rec_train_implicit_cg" in SIGNATURES
    assert api.ALS_CG_MAX_STEPS == 256 and api.IALS_SOLVERS == ("cholesky", "cg")
    L = cu.lib()
    assert L.cu2rec_model_als_implicit_cg(None, None, None, 40.0, 0, 3, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert L.cu2rec_train_implicit_cg(None, None, None, 40.0, 3, 0, None, None) == -1


def test_bad_solver_is_a_value_error_before_anything_is_touched():
    with pytest.raises(ValueError):
        cu.Model.ials(None, None, (0, 1, 1, 0, 0), solver="lu")
    with pytest.raises(ValueError):
        cu.train(None, None, api.default_config(), mode="ials", solver="CG")


def test_mf_usage_lists_C_and_refuses_it_before_the_gpu():
    mf = os.path.join(ROOT, "bin", "mf")

    def run(*args):
        return subprocess.run([mf] + list(args) + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True)
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert "[-C cg_steps]" in res.stderr, res.stderr
    for args in (("-C", "3"), ("-m", "als", "-C", "3"), ("-m", "ials", "-C", "x"), ("-m", "ials", "-C", "3x"), ("-m", "ials", "-C", "0"),
                 ("-m", "ials", "-C", "-1"), ("-m", "ials", "-C", "257")):
        res = run(*args)
        assert res.returncode != 0 and "-C" in res.stderr and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)
