"""CPU checks of alternating least squares: the float64 reference (tests/als_reference64.py) against hand-solved cases and its own
normal equations, and the host side of the new interface -- the C entry point's argument check, the constants the header and the
Python package share, the usage lines of bin/mf and bin/predict.  Also the judge of the GPU edge tests itself: the rounding bound of
als_reference64.row_residual holds for a float32 restatement of the row solve on every conditioning set of tests/als_checks.py,
and three deliberate mistakes in that restatement break it."""
import os
import re
import subprocess

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from conftest import ROOT

import als_checks as chk
import als_reference64 as ref


def _csr(rows, cols, per_row):
    """per_row: list of [(item, rating), ...] per user."""
    indptr = np.zeros(rows + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in per_row])
    items = [i for r in per_row for i, _ in r]
    ratings = [x for r in per_row for _, x in r]
    return api.HostCSR(indptr, np.array(items, np.int32), np.array(ratings, np.float32), rows, cols, 0.0)


def test_reference_f1_closed_form():
    """f = 1, one user with two ratings: the 2 x 2 system solved by hand (Cramer's rule)."""
    gb, q, ib = 0.5, np.array([[2.0], [-1.0]]), np.array([0.25, -0.5])
    csr = _csr(1, 2, [[(0, 4.0), (1, 2.0)]])
    hyper = (0.01, 0.5, 0.5, 0.25, 0.25)
    P, Q, ub, ib2 = ref.half_step(csr, np.zeros((1, 1)), q, np.zeros(1), ib, gb, hyper, "users")
    t = np.array([4.0 - gb - 0.25, 2.0 - gb + 0.5])  # r - gb - ib
    n = 2
    a11 = 4.0 + 1.0 + n * 0.5   # sum q^2 + n P_reg
    a12 = 2.0 - 1.0             # sum q
    a22 = 2.0 + n * 0.25        # sum 1 + n user_bias_reg
    b1, b2 = 2.0 * t[0] - 1.0 * t[1], t[0] + t[1]
    det = a11 * a22 - a12 * a12
    assert np.isclose(P[0, 0], (b1 * a22 - a12 * b2) / det, rtol=1e-14)
    assert np.isclose(ub[0], (a11 * b2 - a12 * b1) / det, rtol=1e-14)
    assert np.array_equal(Q, q) and np.array_equal(ib2, ib)  # the other side is untouched


def test_reference_single_rating_item_side():
    """An item rated once, f = 1: y = [q; ib] solves ((p^2 + Q_reg, p), (p, 1 + item_bias_reg)) y = t (p, 1)."""
    csr = _csr(2, 3, [[(2, 3.0)], []])
    P, ub = np.array([[1.5], [7.0]]), np.array([0.25, 9.0])
    hyper = (0.01, 0.1, 0.2, 0.3, 0.4)
    hP, Q, hub, ib = ref.half_step(csr, P, np.zeros((3, 1)), ub, np.zeros(3), 1.0, hyper, "items")
    t = 3.0 - 1.0 - 0.25
    A = np.array([[1.5 ** 2 + float(np.float32(0.2)), 1.5], [1.5, 1.0 + float(np.float32(0.4))]])
    y = np.linalg.solve(A, t * np.array([1.5, 1.0]))
    assert np.allclose([Q[2, 0], ib[2]], y, rtol=1e-14)
    assert Q[0, 0] == 0 and Q[1, 0] == 0 and ib[0] == 0 and ib[1] == 0  # items without ratings keep their values
    assert np.array_equal(hP, P) and np.array_equal(hub, ub)


def test_reference_solves_normal_equations_and_lowers_objective():
    rng = np.random.default_rng(5)
    tr, _ = synth.make_ratings(60, 25, 700, min_degree=2, seed=11)
    f, gb = 5, tr.global_bias
    P, Q = rng.normal(0, 0.3, (tr.rows, f)), rng.normal(0, 0.3, (tr.cols, f))
    ub, ib = rng.normal(0, 0.1, tr.rows), rng.normal(0, 0.1, tr.cols)
    hyper = (0.01, 0.05, 0.07, 0.02, 0.03)
    L0 = ref.objective(tr, P, Q, ub, ib, gb, hyper)
    P1, Q1, ub1, ib1 = ref.half_step(tr, P, Q, ub, ib, gb, hyper, "users")
    for u in range(tr.rows):
        if tr.indptr[u + 1] == tr.indptr[u]:
            continue
        A, b = ref.system(tr.indptr, tr.indices, tr.data, Q, ib, gb, hyper[1], hyper[3], u)
        x = np.concatenate([P1[u], [ub1[u]]])
        assert np.abs(A @ x - b).max() <= 1e-10 * max(1.0, np.abs(b).max())
    L1 = ref.objective(tr, P1, Q1, ub1, ib1, gb, hyper)
    P2, Q2, ub2, ib2 = ref.half_step(tr, P1, Q1, ub1, ib1, gb, hyper, "items")
    L2 = ref.objective(tr, P2, Q2, ub2, ib2, gb, hyper)
    assert L2 <= L1 <= L0
    # the objective's gradient in one user's factors vanishes at the user half-step's solution
    u, eps = int(np.argmax(np.diff(tr.indptr))), 1e-6
    for k in range(f):
        Pp, Pm = P1.copy(), P1.copy()
        Pp[u, k] += eps
        Pm[u, k] -= eps
        g = ref.objective(tr, Pp, Q1, ub1, ib1, gb, hyper) - ref.objective(tr, Pm, Q1, ub1, ib1, gb, hyper)
        assert abs(g / (2 * eps)) <= 1e-5


def test_model_als_null_is_einval():
    L = cu.lib()
    assert L.cu2rec_model_als(None, None, None, 0, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert "null" in L.cu2rec_last_error().decode()


def test_als_constants_match_header():
    header = open(os.path.join(ROOT, "include", "cu2rec_amd.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"CU2REC_(ALS(?:_[A-Z_]+)?) = (\d+)", header)}
    mantissa, shift = re.search(r"CU2REC_ALS_WORKSPACE_BYTES = (\d+) << (\d+)", header).groups()
    vals["ALS_WORKSPACE_BYTES"] = int(mantissa) << int(shift)
    assert vals["ALS"] == api.ALS == cu.ALS == 5
    assert vals["ALS_MAX_FACTORS"] == api.ALS_MAX_FACTORS == 252
    assert vals["ALS_STEP"] == api.ALS_STEP and vals["ALS_CHUNK"] == api.ALS_CHUNK
    assert vals["ALS_MAX_CHUNKS"] == api.ALS_MAX_CHUNKS and vals["ALS_WORKSPACE_BYTES"] == api.ALS_WORKSPACE_BYTES
    assert api.MODES["als"] == api.ALS


def test_mf_usage_lists_als():
    res = subprocess.run([os.path.join(ROOT, "bin", "mf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bals\b", usage[0]), res.stderr


def test_mf_als_refuses_several_gpus():
    """-m als with -g 2 is refused before any file is read or any GPU is touched."""
    res = subprocess.run([os.path.join(ROOT, "bin", "mf"), "-m", "als", "-g", "2", "missing_train.csv", "missing_test.csv"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "als" in res.stderr, res.stderr


def test_predict_usage_lists_A():
    res = subprocess.run([os.path.join(ROOT, "bin", "predict"), "-c", "x"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert res.returncode != 0 and "[-A]" in res.stderr, res.stderr


def _f32_ratios(case, rows=None, mutation=None, forward=None):
    """{row: max |A x - b| / bound, or None where the float32 restatement meets a bad pivot} over the rows of a Case; with
    `forward` (a dict) also {row: max |x - x*| / (1e-3 max(1, |x*|_inf))} into it."""
    c = case.csr
    out = {}
    with np.errstate(all="ignore"):
        for r in (range(c.rows) if rows is None else rows):
            x = ref.solve_row_f32(c.indptr, c.indices, c.data, case.X, case.xb, c.global_bias, case.reg, case.reg_b, r, mutation)
            if x is None:
                out[r] = None
                continue
            A, b, res, bound = ref.row_residual(c.indptr, c.indices, c.data, case.X, case.xb, c.global_bias, case.reg, case.reg_b, r, x)
            out[r] = ref.residual_ratio(res, bound)
            if forward is not None:
                xs = np.linalg.solve(A, b)
                forward[r] = float(np.abs(x - xs).max() / (1e-3 * max(1.0, np.abs(xs).max())))
    return out


def test_float32_restatement_meets_the_residual_bound_on_every_conditioning_set():
    """The inputs of test_gpu_als_edges.py's conditioning classes are fair: plain float32 arithmetic solves every row outside the
    class `singular` and stays within row_residual's bound everywhere; a singular row either meets a bad pivot or is within it.
    It also meets the forward bar on every row on which Case.well_conditioned() puts that bar in force for the GPU."""
    for f in (8, 100):
        for case in chk.conditioning_cases(f):
            fwd = {}
            ratios = _f32_ratios(case, forward=fwd)
            failed = [r for r, v in ratios.items() if v is None]
            worst = max((v for v in ratios.values() if v is not None), default=0.0)
            barred = np.flatnonzero(case.well_conditioned())
            worst_fwd = max((fwd[r] for r in barred), default=0.0)
            print("f=%d %-9s rows=%d worst residual/bound=%.3g unsolved=%d; forward bar on %d rows, worst error/bar=%.3g"
                  % (f, case.name, case.csr.rows, worst, len(failed), len(barred), worst_fwd))
            if not case.singular:
                assert not failed, (f, case.name, [(r, case.class_of[r]) for r in failed])
                assert len(barred) >= 5
            assert worst <= 1.0, (f, case.name, worst)
            assert worst_fwd <= 1.0, (f, case.name, [(r, case.class_of[r], fwd[r]) for r in barred if fwd[r] > 1.0])


def test_residual_bound_has_teeth():
    """Three mistakes a kernel could make each leave the bound, on both well-conditioned sets (base and bias0): the two
    regularisers swapped and the regulariser scaled by n - 1 (judged on the rows of at most 64 ratings, where an error of
    ~reg |x| stands above n^2 u), and one rating dropped at the chunk boundary of a 1,025-rating row.  A mutated solve that meets
    a bad pivot counts as noticed (the GPU tests require every such row to be solved): swapping in a factor regulariser of 0
    (bias0) leaves rows of fewer ratings than factors singular.  n - 1 is not judged on the one-rating row: there it removes the
    regulariser altogether and leaves z z^T, which has no solution to hold against a bound."""
    for f in (8, 100):
        for base in chk.conditioning_cases(f)[:2]:
            assert base.name in ("base", "bias0")
            short = base.classes["short"]
            assert base.csr.indptr[short[0] + 1] - base.csr.indptr[short[0]] == 1
            clean = _f32_ratios(base, short)
            assert max(clean.values()) <= 1.0
            for mutation in ("swap_reg", "n_minus_1"):
                judged = short[1:] if mutation == "n_minus_1" else short
                got = _f32_ratios(base, judged, mutation)
                missed = [r for r in judged if got[r] is not None and got[r] <= 1.0]
                print("f=%d %s %s: smallest residual/bound %.3g, bad pivot on %d rows"
                      % (f, base.name, mutation, min((v for v in got.values() if v is not None), default=np.inf),
                         sum(v is None for v in got.values())))
                assert not missed, (f, base.name, mutation, [(r, got[r]) for r in missed])
            row = base.classes["long"][0]
            assert base.csr.indptr[row + 1] - base.csr.indptr[row] == 1025
            assert _f32_ratios(base, [row])[row] <= 1.0
            dropped = _f32_ratios(base, [row], "drop_1024")[row]
            print("f=%d %s drop_1024: residual/bound %.3g" % (f, base.name, dropped))
            assert dropped > 1.0, (f, base.name, dropped)
