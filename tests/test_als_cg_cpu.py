"""The explicit conjugate-gradient half-step without a GPU: its float64 reference (tests/als_cg_reference64.py) against
numpy.linalg.solve, the fairness of the GPU test sets (tests/als_cg_checks.py: a float32 restatement in operator form is within half
the bar on every judged row; seven deliberate mistakes miss it by more than two bars), and the declarations of the C ABI, the Python
front end and bin/mf.

The bar is the project's: max |x - x*| <= 1e-3 max(1, |x*|_inf) (ials_checks.bar_ratio), x* = [factors; bias] the float64 CG iterate
at the same step count from the same float32 state."""
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import SIGNATURES
from conftest import ROOT

import als_cg_checks as cgchk
import als_cg_reference64 as cgref
import als_checks as achk
import als_reference64 as ref
from ials_checks import bar_ratio

FAIR = 0.5  # of the bar: what a set may use with the restatement alone


def claimed(mutation, case):
    """Whether the GPU set `case` is claimed to see `mutation` at 3 steps: every mutation on every set (measured: 65 bars at the
    least, t_without_partner_bias on messy-f8-items), except one step too few and the cold start at f = 1 -- the system has order
    2, two steps solve it from any start, and both mistakes leave the third iterate where it was (1e-12 of the bar)."""
    if mutation in ("steps_minus_1", "cold_start"):
        return case.f != 1
    return True


@pytest.mark.parametrize("name,extra", [("lengths-f8-users", 3), ("lengths-f8-items", 3), ("messy-f8-users", 3), ("lengths-f31-users", 0),
                                        ("lengths-f31-items", 0)])
def test_D_steps_of_cg_are_the_exact_solution(name, extra):
    """In exact arithmetic CG ends after D = f + 1 steps; in float64 on these systems (cond(A) <= (0.09 f + 1) / 0.02 by the
    regulariser's n-fold weight: 190 at the most, on a one-rating row at f = 31) it agrees with numpy.linalg.solve to 1e-10
    relative.  Wider sets are not used: a row of n ratings is solved after n + 2 steps, and at f = 100 the 98 steps that follow on a
    one-rating row drive rho into the denormals, where the iteration as documented ends not finite.  At f = 8 the rows of about D ratings have D well-separated eigenvalues and really need the last step, which
    float64 takes with conjugacy already lost: 8e-8 after D = 9 steps, 5e-15 after three more -- so those sets are given D + 3."""
    case = cgchk.cases()[name]
    args = case.system_of(case.state())
    indptr, indices, data, X, xb, gb, reg, reg_b, _ = args
    rows = cgchk.cg_rows_of(indptr)
    got = cgref.cg_rows(*args, case.f + 1 + extra, rows=rows)
    want = np.array([np.linalg.solve(*ref.system(indptr, indices, data, np.asarray(X, np.float64), np.asarray(xb, np.float64), gb, reg,
                                                 reg_b, int(r))) for r in rows])
    rel = float((np.abs(got - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1))).max())
    print("%s: %d steps of float64 CG within %.3g (relative) of numpy.linalg.solve over %d rows" % (name, case.f + 1 + extra, rel, len(rows)))
    assert rel <= 1e-10, (name, rel)


def test_reference_starts_stops_and_fails_as_written():
    """A start that is not finite (a factor or the bias) is the zero start; a rating that is not finite leaves the row unsolved
    (NaN); a row without ratings keeps its values; the warm start reads [factors; bias]."""
    X = np.array([[0.5, -0.25], [0.25, 1.0], [-1.0, 0.5]], np.float32)
    xb = np.array([0.1, -0.2, 0.3], np.float32)
    indptr, indices = np.array([0, 2, 2, 3]), np.array([0, 2, 1])
    data = np.array([1.0, 2.0, np.inf])
    x0 = np.array([[0.3, 0.1, 0.7], [0.7, -0.4, 0.2], [0.1, 0.1, 0.1]])
    args = (indptr, indices, data, X, xb, 1.5, 0.5, 0.25)
    out = cgref.cg_rows(*args, x0, 3)
    A, b = ref.system(indptr, indices, data, X.astype(np.float64), xb.astype(np.float64), 1.5, 0.5, 0.25, 0)
    assert np.abs(out[0] - np.linalg.solve(A, b)).max() <= 1e-12  # order 3: three steps are exact
    assert np.array_equal(out[1], x0[1]) and np.isnan(out[2]).all()
    assert not np.allclose(cgref.cg_rows(*args, x0, 1)[0], cgref.cg_rows(*args, None, 1)[0])  # the start is read
    for col in (0, 2):
        bad = x0.copy()
        bad[0, col] = np.nan
        assert np.array_equal(cgref.cg_rows(*args, bad, 1)[0], cgref.cg_rows(*args, None, 1)[0])
    f32 = cgref.cg_rows_f32(*args, x0, 3)[-1]
    assert np.abs(f32[0] - out[0]).max() <= 1e-5 and np.array_equal(f32[1], x0[1]) and np.isnan(f32[2]).all()


@pytest.mark.parametrize("name", sorted(cgchk.cases()))
def test_float32_restatement_is_within_half_the_bar_on_every_judged_row(name):
    case = cgchk.cases()[name]
    args = case.system_of(case.state())
    rows, want = cgchk.reference(case)
    assert len(rows) > 0
    got = cgref.cg_rows_f32(*args, max(cgchk.STEPS), rows=rows)
    ratios = []
    for s in cgchk.STEPS:
        on = np.isin(rows, cgchk.fair_rows(case, s))
        assert on.sum() >= len(rows) - 8  # only the rows of one rating are ever left out
        assert np.isfinite(got[s - 1]).all()
        ratios.append(bar_ratio(got[s - 1][on], want[s - 1][on]))
    print("%s: float32 restatement at %s of the bar after 1, 2, 3 steps over %d rows" % (name, ", ".join("%.3g" % r for r in ratios), len(rows)))
    assert max(ratios) <= FAIR, (name, ratios)


@pytest.mark.parametrize("name", sorted(n for n in cgchk.cases() if n.startswith("lengths")))
def test_one_rating_rows_at_three_steps_are_left_out_only_where_the_restatement_is_unfair(name):
    """als_cg_checks.fair_rows, width by width and side by side: where the one-rating rows are not judged at three steps the
    restatement itself uses more than half the bar on them there, where they are judged it uses at most half; after two steps it is
    fair on them at every width."""
    case = cgchk.cases()[name]
    args = case.system_of(case.state())
    rows, want = cgchk.reference(case)
    one = np.diff(args[0])[rows] == 1
    assert 2 <= one.sum() <= 8 and np.isin(rows[one], cgchk.fair_rows(case, 2)).all()
    got = cgref.cg_rows_f32(*args, 3, rows=rows[one])
    two, three = bar_ratio(got[1], want[1][one]), bar_ratio(got[2], want[2][one])
    judged = np.isin(rows[one], cgchk.fair_rows(case, 3))
    print("%s: one-rating rows: float32 restatement at %.3g of the bar after 2 steps, %.3g after 3 (%s)" % (
        name, two, three, "judged" if judged.all() else "not judged"))
    assert judged.all() or not judged.any()
    assert two <= FAIR, (name, two)
    assert (three <= FAIR) == bool(judged.all()), (name, three)


@pytest.mark.parametrize("name", sorted(cgchk.cases()))
def test_seven_mistakes_miss_the_bar_on_every_set_that_claims_them(name):
    """At 3 steps over the rows judged there, per set, on every set claimed() lists; no set is claimed under two bars."""
    case = cgchk.cases()[name]
    args = case.system_of(case.state())
    rows, want = cgchk.reference(case)
    on = np.isin(rows, cgchk.fair_rows(case, 3))
    for mutation in cgref.MUTATIONS:
        wrong = cgref.cg_rows(*args, 3, mutation=mutation, rows=rows[on])
        ratio = bar_ratio(wrong, want[2][on])
        print("%s: %s is %.3g of the bar off%s" % (name, mutation, ratio, "" if claimed(mutation, case) else " (not claimed)"))
        if claimed(mutation, case):
            assert ratio > 2.0, (name, mutation, ratio)


@pytest.mark.parametrize("name", sorted(cgchk.conditioning_cases()))
def test_conditioning_classes_are_judged_exactly_where_the_restatement_is_fair(name):
    """Every (case, class, steps) of the conditioning sets: judged on the GPU and at most half the bar with the restatement, or
    listed in als_cg_checks.CONDITIONING_UNFAIR and above half the bar with the restatement."""
    case, judged, classes, base = cgchk.conditioning_cases()[name]
    args = case.system_of(case.state())
    rows = cgchk.cg_rows_of(args[0])
    want = cgref.cg_rows_upto(*args, 3, rows=rows)
    got = cgref.cg_rows_f32(*args, 3, rows=rows)
    assert {"short", "f_plus_5", "same_row", "repeat_40", "down"} <= set(classes) and ("up" in classes) == (base == "reg_10")
    for s in cgchk.STEPS:
        assert np.isfinite(got[s - 1]).all()
        for cls, rs in sorted(classes.items()):
            on = np.isin(rows, rs)
            ratio = bar_ratio(got[s - 1][on], want[s - 1][on])
            unfair = (base, cls, s) in cgchk.CONDITIONING_UNFAIR
            assert np.isin(rs, judged[s]).all() != unfair
            print("%s: %s after %d steps: float32 restatement at %.3g of the bar over %d rows%s" % (
                name, cls, s, ratio, on.sum(), " (not judged)" if unfair else ""))
            assert (ratio > FAIR) == unfair, (name, cls, s, ratio)


@pytest.mark.parametrize("name", sorted(cgchk.unsolved_cases()))
def test_restatement_fails_exactly_the_rows_that_hold_the_bad_value(name):
    case, bad, nan_start = cgchk.unsolved_cases()[name]
    args = case.system_of(case.state())
    rows = cgchk.cg_rows_of(args[0])
    assert len(bad) > 2 and not np.isin(nan_start, bad).any() and np.isin(nan_start, rows).all()
    got = cgref.cg_rows_f32(*args, 3, rows=rows)[-1]
    want = cgref.cg_rows(*args, 3, rows=rows)
    assert np.array_equal(rows[np.isnan(got).any(axis=1)], bad), (name, bad)
    good = ~np.isin(rows, bad)
    ratio = bar_ratio(got[good], want[good])
    print("%s: float32 restatement at %.3g of the bar on the other %d rows" % (name, ratio, good.sum()))
    assert ratio <= FAIR, (name, ratio)


def test_many_rows_set_takes_more_than_one_grid_pass():
    """And the restatement is fair on its judged sample at the three steps the GPU test takes (the worst rows have ONE rating, see
    als_cg_checks.fair_rows: 0.42 of the bar at this width against 8e-3 after two steps)."""
    csr = cgchk.many_rows_set()
    assert csr.rows > 2 * cgchk.GRID_PASS and np.diff(csr.indptr).max() <= 4 and np.diff(csr.indptr).min() >= 1
    state = achk.random_state(csr.rows, csr.cols, cgchk.MANY_ROWS_F, cgchk.MANY_ROWS_SEED)
    case = cgchk.Case("many-rows", csr, "users", cgchk.MANY_ROWS_F, cgchk.HYPER, state=state)
    _, sample = cgchk.many_rows_sample()
    args = case.system_of(state)
    ratio = bar_ratio(cgref.cg_rows_f32(*args, 3, rows=sample)[-1], cgref.cg_rows(*args, 3, rows=sample))
    print("20,000 rows: float32 restatement at %.3g of the bar over %d sampled rows" % (ratio, len(sample)))
    assert ratio <= FAIR, ratio


@pytest.mark.parametrize("f", [8, 100])
def test_sixteen_and_boundary_steps_of_the_restatement(f):
    """f = 8: sixteen float32 steps are within half the bar of the exact float64 optimum on every CG row (the GPU test's claim).
    Both widths: the row of exactly 1,024 ratings is fair at one step (the length-boundary test judges it there)."""
    case = cgchk.cases()["lengths-f%d-users" % f]
    args = case.system_of(case.state())
    indptr, indices, data, X, xb, gb, reg, reg_b, _ = args
    rows = cgchk.cg_rows_of(indptr)
    if f == 8:
        got = cgref.cg_rows_f32(*args, 16, rows=rows)[-1]
        want = np.array([np.linalg.solve(*ref.system(indptr, indices, data, np.asarray(X, np.float64), np.asarray(xb, np.float64), gb,
                                                     reg, reg_b, int(r))) for r in rows])
        ratio = bar_ratio(got, want)
        print("f=8: 16 float32 CG steps at %.3g of the bar from the float64 optimum" % ratio)
        assert ratio <= FAIR, ratio
    cut = rows[np.diff(indptr)[rows] == cgchk.CHUNK]
    assert len(cut) == 1
    ratio = bar_ratio(cgref.cg_rows_f32(*args, 1, rows=cut)[-1], cgref.cg_rows(*args, 1, rows=cut))
    assert ratio <= FAIR, (f, ratio)


def test_declarations():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"int cu2rec_model_als_cg\(cu2rec_model \*m, const cu2rec_csr \*train, const cu2rec_hyper \*hyper, int side, "
                     r"int cg_steps,\s*int \*unsolved\);", header)
    assert re.search(r"int cu2rec_train_als_cg\(const cu2rec_csr \*train, const cu2rec_csr \*test, cu2rec_config \*cfg, "
                     r"cu2rec_model \*model, int cg_steps,\s*int verbose, float \*losses, cu2rec_train_stats \*stats\);", header)
    doc = header[header.index("int cu2rec_model_als(cu2rec_model"):header.index("int cu2rec_model_als_cg(")]
    for phrase in ("x0 = [the row's n_factors factors; its bias]", "if rho == 0 stop", "if d == 0 stop", "solved exactly whatever cg_steps is",
                   "CU2REC_ALS_CG_MAX_STEPS"):
        assert phrase in doc, phrase
    assert "cu2rec_model_als_cg" in SIGNATURES and "cu2rec_train_als_cg" in SIGNATURES
    L = cu.lib()
    assert L.cu2rec_model_als_cg(None, None, None, 0, 3, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert L.cu2rec_train_als_cg(None, None, None, None, 3, 0, None, None) == -1


def test_bad_solver_is_a_value_error_before_anything_is_touched():
    with pytest.raises(ValueError):
        cu.Model.als(None, None, (0, 1, 1, 0, 0), solver="lu")
    with pytest.raises(ValueError):
        cu.train(None, None, api.default_config(), mode="als", solver="CG")


def test_mf_alscg_refuses_bad_step_counts_before_the_gpu():
    mf = os.path.join(ROOT, "bin", "mf")

    def run(*args):
        return subprocess.run([mf] + list(args) + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True)
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and "[-C cg_steps]" in usage[0] and re.search(r"-m [a-z|]*\balscg\b", usage[0]), res.stderr
    for args in (("-m", "alscg", "-C", "0"), ("-m", "alscg", "-C", "257"), ("-m", "alscg", "-C", "x"), ("-m", "als", "-C", "3"),
                 ("-m", "blocksolve", "-C", "3"), ("-C", "3")):
        res = run(*args)
        assert res.returncode != 0 and "-C" in res.stderr and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)
    res = run("-m", "alscg", "-g", "2")
    assert res.returncode != 0 and "alscg" in res.stderr and "Free memory" not in res.stdout, res.stderr
