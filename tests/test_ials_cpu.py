"""CPU checks of implicit-feedback alternating least squares: the float64 reference (tests/ials_reference64.py) against a
hand-solved case, its own objective and gradient; the host side of the interface (argument checks that need no device, the
CLIs' usage lines, the Python front end); and the fairness of the GPU tests' own inputs.

Fairness: on every set tests/test_gpu_ials.py and tests/test_gpu_ials_edges.py judge (tests/ials_checks.cases, unsolved_cases,
big_partner_case), a float32 restatement of the device arithmetic meets the project's forward bar -- every solved row within
1e-3 max(1, |x*|_inf) of the float64 optimum -- on every judged row, none excluded, and fails to factorise exactly the rows the
GPU tests expect to be counted.  Discrimination: on every one of those sets the float64 reference itself misses that bar on some
judged row when it is computed wrongly in each of five ways (n reg for reg, G0 left out, weights 1 + w in the Gram, right-hand
side weighted by w, one tile pair of the row's own sums zeroed)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from conftest import ROOT, ml_small

import ials_checks as chk
import ials_reference64 as ref


def _csr(rows, cols, per_row):
    indptr = np.zeros(rows + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in per_row])
    items = [i for r in per_row for i, _ in r]
    values = [x for r in per_row for _, x in r]
    return api.HostCSR(indptr, np.array(items, np.int32), np.array(values, np.float32), rows, cols, 0.0)


def test_reference_f1_closed_form():
    """f = 1, three items, user 0 with the entries (0, r = 2) and (2, r = 0.5), user 1 with none, alpha = 3:
    p_0 = sum (1 + w) q / (sum_all q^2 + sum w q^2 + P_reg); p_1 = 0; item 1, named by nobody, becomes 0 in the item half-step."""
    q = np.array([[2.0], [-1.0], [0.5]])
    csr = _csr(2, 3, [[(0, 2.0), (2, 0.5)], []])
    hyper = (0.01, 0.5, 0.25, 9.0, 9.0)
    P, Q = ref.half_step(csr, np.array([[7.0], [7.0]]), q, hyper, 3.0, "users")
    w0, w2 = 6.0, 1.5
    want = ((1 + w0) * 2.0 + (1 + w2) * 0.5) / ((4.0 + 1.0 + 0.25) + w0 * 4.0 + w2 * 0.25 + 0.5)
    assert np.isclose(P[0, 0], want, rtol=1e-14) and P[1, 0] == 0.0 and np.array_equal(Q, q)
    P2, Q2 = ref.half_step(csr, P, q, hyper, 3.0, "items")
    g0 = P[0, 0] ** 2
    assert np.isclose(Q2[0, 0], (1 + w0) * P[0, 0] / (g0 + w0 * g0 + 0.25), rtol=1e-14) and Q2[1, 0] == 0.0
    assert np.array_equal(P2, P)


def test_reference_minimises_its_objective():
    """The half-step's rows are stationary points of objective() (central differences), a repeated pair counts twice, and model
    rows past the CSR stay out of both."""
    rng = np.random.default_rng(3)
    per_row = [[(int(i), float(rng.integers(0, 11)) / 2) for i in rng.integers(0, 9, n)] for n in (4, 0, 7, 1, 12)]
    per_row[2][1] = per_row[2][0]  # the same (user, item) pair twice
    csr = _csr(5, 9, per_row)
    f, hyper, alpha = 4, (0.01, 0.3, 0.2, 0.0, 0.0), 2.5
    P, Q = rng.normal(0, 0.3, (7, f)), rng.normal(0, 0.3, (12, f))
    L0 = ref.objective(csr, P, Q, hyper, alpha)
    P1, Q1 = ref.half_step(csr, P, Q, hyper, alpha, "users")
    assert np.array_equal(P1[5:], P[5:]) and np.array_equal(Q1, Q) and not P1[1].any()
    L1 = ref.objective(csr, P1, Q1, hyper, alpha)
    P2, Q2 = ref.half_step(csr, P1, Q1, hyper, alpha, "items")
    L2 = ref.objective(csr, P2, Q2, hyper, alpha)
    assert L2 < L1 < L0
    eps = 1e-6
    for (M, which) in ((P1, 0), (Q2, 1)):
        for r, k in ((0, 1), (2, 3), (4, 0)):
            args = [P1, Q1] if which == 0 else [P2, Q2]
            up, down = M.copy(), M.copy()
            up[r, k] += eps
            down[r, k] -= eps
            hi = ref.objective(csr, *(args[:which] + [up] + args[which + 1:]), hyper, alpha)
            lo = ref.objective(csr, *(args[:which] + [down] + args[which + 1:]), hyper, alpha)
            assert abs(hi - lo) / (2 * eps) <= 1e-6, (which, r, k)
    big = P1.copy()
    big[6] += 100.0  # a model row past the CSR is not part of the objective
    assert ref.objective(csr, big, Q1, hyper, alpha) == L1


def test_reference_objective_never_rises_on_ml_small():
    tr = cu.createSparseMatrix(ml_small())
    rng = np.random.default_rng(9)
    f, hyper = 16, (0.01, 0.1, 0.1, 0.0, 0.0)
    states = ref.run(tr, rng.normal(0, 0.1, (tr.rows, f)), rng.normal(0, 0.1, (tr.cols, f)), hyper, 40.0, 5)
    L = [ref.objective(tr, P, Q, hyper, 40.0) for P, Q in states]
    assert len(L) == 11 and all(b <= a for a, b in zip(L, L[1:])) and L[-1] < 0.5 * L[0], L


def test_restatement_constants_match_the_package():
    assert (ref.STEP, ref.CHUNK, ref.MAX_CHUNKS) == (api.ALS_STEP, api.ALS_CHUNK, api.ALS_MAX_CHUNKS)
    for n in (1025, 2049, 4097, 64 * 1024 + 1):
        assert -(-n // ref.chunk_len(n)) == chk.chk.chunks_of(n)


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_float32_restatement_meets_the_bar_on_every_judged_row(name):
    case = chk.cases()[name]
    indptr, indices, data, X, reg = case.system()
    rows = case.judged()
    assert len(rows) > 0
    want = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows)
    got = ref.solve_rows_f32(indptr, indices, data, X, reg, case.alpha, rows=rows)
    ratio = chk.bar_ratio(got, want)
    print("%s: float32 restatement at %.3g of the bar over %d rows" % (name, ratio, len(rows)))
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_four_mistakes_miss_the_bar_on_every_set(name):
    """(Five since ials_reference64.MUTATIONS holds "tile_pair"; the name is the one the test was added under.)"""
    case = chk.cases()[name]
    indptr, indices, data, X, reg = case.system()
    rows = case.judged()
    want = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows)
    for mutation in ref.MUTATIONS:
        wrong = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows, mutation=mutation)
        ratio = chk.bar_ratio(wrong, want)
        print("%s: %s is %.3g of the bar off" % (name, mutation, ratio))
        assert ratio > 1.0, (name, mutation, ratio)


def test_messy_set_holds_what_it_is_for():
    csr = chk.messy_set()
    assert (csr.data == 0).any() and (np.diff(csr.indptr) == 0).any() and (np.bincount(csr.indices, minlength=csr.cols) == 0).any()
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    assert len(np.unique(users * csr.cols + csr.indices)) < csr.nnz  # repeated pairs
    assert (np.diff(csr.indices) < 0).any() and csr.indices.max() == csr.cols - 4


def test_small_partner_set_has_fewer_partners_than_factors():
    for name in ("small-partners-f100-users", "small-partners-f100-items"):
        case = chk.cases()[name]
        assert case.system()[3].shape[0] < case.f


def _solved_and_failed(case, fail, X=None):
    """The restatement on every row with entries -> (rows it solved, rows it could not factorise), with the solved ones held to
    the bar against float64 and to the five mistakes."""
    indptr, indices, data, X0, reg = case.system()
    X = X0 if X is None else X
    rows = case.judged()
    with np.errstate(all="ignore"):
        got = ref.solve_rows_f32(indptr, indices, data, X, reg, case.alpha, rows=rows)
    failed = rows[np.isnan(got).any(axis=1)]
    solved = np.setdiff1d(rows, failed)
    assert np.array_equal(failed, np.sort(fail)), (case.name, failed, fail)
    if len(solved):
        keep = np.isin(rows, solved)
        want = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=solved)
        ratio = chk.bar_ratio(got[keep], want)
        print("%s: %d rows fail; float32 restatement at %.3g of the bar over the other %d" % (case.name, len(failed), ratio, len(solved)))
        assert ratio <= 1.0, (case.name, ratio)
        for mutation in ref.MUTATIONS:
            wrong = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=solved, mutation=mutation)
            assert chk.bar_ratio(wrong, want) > 1.0, (case.name, mutation)
    return solved, failed


@pytest.mark.parametrize("name", sorted(chk.unsolved_cases()))
def test_restatement_fails_exactly_the_rows_that_cannot_be_solved(name):
    """poison-entry (a NaN and a +inf entry), overflow (alpha r = +inf from finite values) and negative (w = -4,000): the float32
    restatement cannot factorise exactly the rows that hold such an entry, meets the bar on every other row with entries, and the
    five mistakes miss it there.  negative: the float64 system of a failing row has an eigenvalue below -10 reg (it is not
    positive definite: a Cholesky factorisation must meet a non-positive pivot); every other row's is above reg / 2."""
    case, fail = chk.unsolved_cases()[name]
    assert len(fail) >= 1
    solved, failed = _solved_and_failed(case, fail)
    if name.startswith("negative"):
        indptr, indices, data, X, reg = case.system()
        assert (data < 0).sum() > 100
        G0 = ref.gram64(X)
        low = {int(r): np.linalg.eigvalsh(ref.row_system(indptr, indices, data, X, reg, case.alpha, r, G0)[0])[0]
               for r in case.judged()}
        assert all(low[int(r)] < -10 * reg for r in failed), [low[int(r)] for r in failed]
        assert all(low[int(r)] > reg / 2 for r in solved), min(low[int(r)] for r in solved)
        negative_and_solved = [r for r in solved if (data[indptr[r]:indptr[r + 1]] < 0).any()]
        assert len(negative_and_solved) >= 10


@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("f", chk.UNSOLVED_WIDTHS)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_restatement_fails_every_row_on_a_poisoned_partner_nobody_names(bad, f, side):
    """One non-finite factor in a partner row inside the CSR poisons G0, and with it every row that is factorised at all."""
    case = chk.Case("poison-unnamed", chk.messy_set(), side, f, 40.0, chk.HYPER, 6500 + f)
    X = case.system()[3].copy()
    r, c = chk.poisoned_partner(case, "inside")
    assert r not in case.system()[1] and r < len(X)
    X[r, c] = bad
    _solved_and_failed(case, case.judged(), X=X)
    assert chk.poisoned_partner(case, "outside")[0] >= len(X)  # a model row past the CSR is not a partner at all


def test_restatement_meets_the_bar_over_two_g0_batches():
    """The 455 x 1,024 + 1 partner case (the restatement's G0 over all of them is computed once): fair, and the five mistakes
    show.  Takes about half a minute, nearly all of it gram_f32 over 456 tiles at f = 252 (recorded beside the GPU test's own time in
    tests/test_gpu_ials_edges.py::test_g0_over_two_workspace_batches)."""
    case = chk.big_partner_case()
    assert -(-chk.BIG_PARTNERS // ref.CHUNK) == api.ALS_WORKSPACE_BYTES // (36 * 16 * 64 * 4) + 1 == 456
    indptr, indices, data, _, reg = case.system_of(chk.big_partner_state())
    X = chk.big_partner_state()[1][:chk.BIG_PARTNERS]
    rows = case.judged()
    assert len(rows) == 5 and indices.max() == chk.BIG_PARTNERS - 1
    G64 = ref.gram64(X)
    want = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows, G0=G64)
    got = ref.solve_rows_f32(indptr, indices, data, X, reg, case.alpha, rows=rows, G0=ref.gram_f32(X))
    ratio = chk.bar_ratio(got, want)
    print("%s: float32 restatement at %.3g of the bar over %d rows" % (case.name, ratio, len(rows)))
    assert ratio <= 1.0
    for mutation in ref.MUTATIONS:
        wrong = ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows, mutation=mutation, G0=G64)
        ratio = chk.bar_ratio(wrong, want)
        print("%s: %s is %.3g of the bar off" % (case.name, mutation, ratio))
        assert ratio > 1.0, mutation


def test_objective_restatement_is_close_to_float64():
    """The relative error of the float32-Gram objective stays within the figure whose 4-fold is the GPU test's tolerance."""
    worst = 0.0
    everything = dict(chk.cases(), **chk.objective_loop_cases())
    assert all(max(c.csr.nnz, c.csr.rows) > chk.OBJECTIVE_LOOP for c in chk.objective_loop_cases().values())
    for name in chk.OBJECTIVE_SETS + chk.OBJECTIVE_LOOP_SETS:
        case = everything[name]
        P, Q, _, _ = case.state()
        want = ref.objective(case.csr, P, Q, case.hyper, case.alpha)
        got = ref.objective_f32(case.csr, P, Q, case.hyper, case.alpha)
        rel = abs(got - want) / abs(want)
        print("%s: objective %.9g, float32 Grams off by %.3g" % (name, want, rel))
        worst = max(worst, rel)
    assert worst <= chk.OBJECTIVE_RESTATEMENT_ERROR


def test_null_arguments_are_einval_without_a_device():
    L = cu.lib()
    assert L.cu2rec_model_als_implicit(None, None, None, 40.0, 0, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_model_implicit_objective(None, None, None, 40.0, None) == -1
    assert L.cu2rec_train_implicit(None, None, None, 40.0, 0, None, None) == -1


def test_python_front_end():
    assert "ials" not in api.MODES  # the SGD mode table is unchanged: train() handles the string itself
    assert callable(cu.Model.ials) and callable(cu.Model.implicit_objective)


def test_mf_usage_lists_ials_and_refuses_several_gpus():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bials\b", usage[0]) and "[-a alpha]" in usage[0], res.stderr
    res = subprocess.run([mf, "-m", "ials", "-g", "2", "missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "ials" in res.stderr, res.stderr
    res = subprocess.run([mf, "-m", "ials", "-a", "-1", "missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "-a" in res.stderr, res.stderr


def test_predict_usage_lists_I_and_refuses_it_with_A():
    predict = os.path.join(ROOT, "bin", "predict")
    res = subprocess.run([predict, "-c", "x"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "[-I alpha]" in res.stderr, res.stderr
    res = subprocess.run([predict, "-c", "x", "-i", "x", "-g", "x", "-q", "x", "-A", "-I", "40", "x.csv"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "-A" in res.stderr and "-I" in res.stderr, res.stderr
    for bad in ("-1", "nan", "x"):
        res = subprocess.run([predict, "-c", "x", "-i", "x", "-g", "x", "-q", "x", "-I", bad, "x.csv"], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "-I must be a finite number >= 0" in res.stderr, (bad, res.stderr)
