"""The conjugate-gradient implicit half-step on the GPU (cu2rec_model_als_implicit_cg, cu2rec_train_implicit_cg, bin/mf -m ials -C,
Model.ials(solver="cg"), train(mode="ials", solver="cg")) against the float64 iteration of tests/ials_cg_reference64.py.

The bar for a row x of 1 .. 1,024 entries is the project's, max |x - x*| <= 1e-3 max(1, |x*|_inf), with x* the float64 CG iterate
after the same number of steps from the same float32 state; tests/test_ials_cg_cpu.py shows on the CPU that a float32 restatement
in operator form meets it on every row judged here (at no more than 2.1e-3 of the bar) and that five deliberate mistakes do not.
Longer rows are solved exactly: bit for bit what cu2rec_model_als_implicit writes.  The judge lives in tests/ials_cg_checks.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib
from conftest import ROOT, ml_small

import als_checks as achk
import ials_cg_checks as cgchk
import ials_cg_reference64 as cgref
import ials_reference64 as ref
from als_checks import interplay, model_from, random_state, same_bits, same_state
from ials_cg_checks import check_cg_half_step, ials_cg
from ials_checks import HYPER, bar_ratio, ials

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6


@pytest.mark.parametrize("name", sorted(cgchk.cases()))
def test_half_step_matches_float64_cg(name):
    """Widths 1, 8, 31, 100, 252 and both edges of every per-lane element count (63 | 64 | 65, 127 | 128 | 129 -- also G0 in LDS |
    in L2 --, 191 | 192 | 193) x rows of 1 .. 4,097 entries on both sides, and the messy set at alpha 40 and 0; 1, 2 and 3 steps."""
    case = cgchk.cases()[name]
    d = cu.DeviceCSR(case.csr)
    rows, want = cgchk.reference(case)
    report = {}
    for steps in cgchk.STEPS:
        model = model_from(case.state(), case.csr.global_bias)
        check_cg_half_step(model, d, case.csr, case.side, case.hyper, case.alpha, steps, report=report, want=(rows, want[steps - 1]))
    print("%s: worst row at %s of the bar after 1, 2, 3 steps; long rows at %.3g" % (
        name, ", ".join("%.3g" % report[(case.side, case.f, s)] for s in cgchk.STEPS), report[(case.side, case.f, "long")]))


@pytest.mark.parametrize("f", [8, 100, 252])
def test_the_cut_between_cg_and_the_exact_rows(f):
    """Rows of 1,025 .. 4,097 entries come out bit for bit as cu2rec_model_als_implicit writes them from the same state, whatever
    cg_steps is; the row of 1,024 entries is CG's (judged by the CG reference at one step, and not the exact solution's bits)."""
    case = cgchk.cases()["lengths-f%d-users" % f]
    csr, d = case.csr, cu.DeviceCSR(case.csr)
    n = np.diff(csr.indptr)
    long_rows, at_cut = np.flatnonzero(n > cgchk.CHUNK), int(np.flatnonzero(n == cgchk.CHUNK)[0])
    assert sorted(n[long_rows]) == [1025, 2047, 2048, 2049, 4097]
    exact = model_from(case.state(), csr.global_bias)
    assert ials(exact, d, case.hyper, case.alpha, "users") == (0, 0)
    Pe = exact.download()[0]
    rows, want = cgchk.reference(case)
    for steps in (1, 7):
        m = model_from(case.state(), csr.global_bias)
        assert ials_cg(m, d, case.hyper, case.alpha, "users", steps) == (0, 0)
        Pc = m.download()[0]
        assert same_bits(Pc[long_rows], Pe[long_rows]), (f, steps)
        assert not same_bits(Pc[at_cut], Pe[at_cut])
        if steps == 1:
            k = int(np.flatnonzero(rows == at_cut)[0])
            assert bar_ratio(Pc[at_cut:at_cut + 1], want[0][k:k + 1]) <= 1.0


@pytest.mark.parametrize("f", [8, 100, 252])
def test_forty_steps_reach_the_exact_optimum(f):
    case = cgchk.cases()["lengths-f%d-users" % f]
    state = case.state()
    m = model_from(state, case.csr.global_bias)
    assert ials_cg(m, cu.DeviceCSR(case.csr), case.hyper, case.alpha, "users", 40) == (0, 0)
    indptr, indices, data, X, reg = case.system_of(state)
    rows = cgchk.cg_rows_of(indptr)
    ratio = bar_ratio(m.download()[0][rows], ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rows))
    print("f=%d: 40 CG steps at %.3g of the bar from the float64 optimum" % (f, ratio))
    assert ratio <= 1.0, (f, ratio)


def test_stopping_rules():
    """Steps past convergence: f = 1 at 5 steps (the first is exact), and 3 steps on a model the exact solver has just solved
    (rho is rounding noise or 0): finite, nothing unsolved, within the bar of the exact optimum."""
    case = cgchk.cases()["lengths-f1-users"]
    state = case.state()
    m = model_from(state, case.csr.global_bias)
    assert ials_cg(m, cu.DeviceCSR(case.csr), case.hyper, case.alpha, "users", 5) == (0, 0)
    indptr, indices, data, X, reg = case.system_of(state)
    rated = np.flatnonzero(np.diff(indptr) > 0)
    got = m.download()[0]
    assert np.isfinite(got).all()
    assert bar_ratio(got[rated], ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rated)) <= 1.0
    for side in ("users", "items"):
        case = cgchk.cases()["lengths-f100-%s" % side]
        state = case.state()
        d = cu.DeviceCSR(case.csr)
        m = model_from(state, case.csr.global_bias)
        assert ials(m, d, case.hyper, case.alpha, side) == (0, 0)
        assert ials_cg(m, d, case.hyper, case.alpha, side, 3) == (0, 0)
        indptr, indices, data, X, reg = case.system_of(state)
        rated = np.flatnonzero(np.diff(indptr) > 0)
        got = m.download()[0 if side == "users" else 1]
        assert np.isfinite(got).all()
        ratio = bar_ratio(got[rated], ref.solve_rows(indptr, indices, data, X, reg, case.alpha, rows=rated))
        print("CG at 3 steps after the exact solver, %s: %.3g of the bar from the optimum" % (side, ratio))
        assert ratio <= 1.0, (side, ratio)


@pytest.mark.parametrize("f", [8, 100, 129])
def test_a_start_that_is_not_finite_is_the_zero_start(f):
    case = cgchk.cases()["lengths-f%d-users" % f]
    csr, d = case.csr, cu.DeviceCSR(case.csr)
    P, Q, ub, ib = case.state()
    poisoned, zeroed = P.copy(), P.copy()
    rows = {5: np.nan, 6: np.inf, 40: -np.inf, 211: np.nan}  # rows of 1,023 and 1,024 entries, a short one, the last row of the CSR
    for u, v in rows.items():
        poisoned[u, (3 * u) % f] = v
        zeroed[u] = 0.0
    poisoned[211, f - 1] = np.inf
    out = []
    for start in (poisoned, zeroed):
        m = model_from((start, Q, ub, ib), csr.global_bias)
        assert ials_cg(m, d, case.hyper, case.alpha, "users", 2) == (0, 0)
        out.append(m.download())
    assert same_state(*out) and np.isfinite(out[0][0]).all()


def _one_user(csr, u, state, f, steps, hyper=HYPER, alpha=40.0):
    """User u solved from a one-user CSR of the same cols, from its row of `state`."""
    P, Q, ub, ib = state
    lo, hi = csr.indptr[u], csr.indptr[u + 1]
    one = api.HostCSR([0, hi - lo], csr.indices[lo:hi], csr.data[lo:hi], 1, csr.cols, 0.0)
    m = cu.Model(1, Q.shape[0], f, 0.0, P=P[u:u + 1], Q=Q, user_bias=ub[u:u + 1], item_bias=ib)
    assert ials_cg(m, cu.DeviceCSR(one), hyper, alpha, "users", steps) == (0, 0)
    return m.download()[0][0]


@pytest.mark.parametrize("f", [100, 252])
def test_deterministic_and_independent_of_the_other_rows(f):
    csr = achk.width_length_set()
    d = cu.DeviceCSR(csr)
    state = random_state(csr.rows, csr.cols, f, 77)
    runs = []
    for _ in range(2):
        m = model_from(state, 0.0)
        assert m.ials(d, HYPER, 40.0, "both", sweeps=2, solver="cg", cg_steps=3) == 0
        runs.append(m.download())
    assert same_state(*runs), "two runs differ"
    batch = model_from(runs[0], 0.0)
    assert batch.ials(d, HYPER, 40.0, "users", solver="cg", cg_steps=3) == 0
    Pb = batch.download()[0]
    # the first and the last wavefront of a workgroup (rows 4 k and 4 k + 3), long rows, the last row
    for u in [0, 3, 4, 7, 8, 9, 10, 11, 50, 208, 211]:
        assert same_bits(_one_user(csr, u, runs[0], f, 3), Pb[u]), u


@pytest.mark.parametrize("rows", [cgchk.SLOTS - 1, cgchk.SLOTS, cgchk.SLOTS + 1, 2 * cgchk.SLOTS + 1])
def test_row_counts_around_one_workgroup(rows):
    """3, 4, 5 and 9 rows (four wavefronts = four rows per workgroup): every row judged, every row equal to its one-row solve."""
    full = achk.width_length_set()
    keep = [12 + 7 * i for i in range(rows)]
    per_row = [full.indices[full.indptr[u]:full.indptr[u + 1]] for u in keep]
    data = np.concatenate([full.data[full.indptr[u]:full.indptr[u + 1]] for u in keep])
    csr = achk.csr_from_rows(per_row, full.cols, None, gb=0.0, ratings=data)
    f = 31
    state = random_state(rows, csr.cols, f, 900 + rows)
    m = model_from(state, 0.0)
    got = check_cg_half_step(m, cu.DeviceCSR(csr), csr, "users", HYPER, 40.0, 2)
    for u in range(rows):
        assert same_bits(_one_user(csr, u, state, f, 2), got[0][u]), (rows, u)


def test_more_rows_than_one_grid_pass():
    """20,000 rows of 1 .. 4 entries at f = 8: the kernel's grid-stride loop takes three trips.  A sample is judged in float64, rows
    on both sides of every trip's edge and the last row are pinned by their one-row CSRs."""
    csr = cgchk.many_rows_set()
    f = cgchk.MANY_ROWS_F
    state = random_state(csr.rows, csr.cols, f, cgchk.MANY_ROWS_SEED)
    m = model_from(state, 0.0)
    assert ials_cg(m, cu.DeviceCSR(csr), HYPER, 40.0, "users", 3) == (0, 0)
    got = m.download()
    assert same_bits(got[1], state[1]) and not got[2].any()
    edges, sample = cgchk.many_rows_sample()
    want = cgref.cg_rows(csr.indptr, csr.indices, csr.data, state[1], HYPER[1], 40.0, state[0], 3, rows=sample)
    ratio = bar_ratio(got[0][sample], want)
    print("20,000 rows: %d sampled rows at %.3g of the bar" % (len(sample), ratio))
    assert ratio <= 1.0
    moved = (got[0].view(np.uint32) != state[0].view(np.uint32)).any(axis=1)
    assert moved.all(), "rows the kernel never reached: %s" % np.flatnonzero(~moved)[:8]
    for u in edges:
        assert same_bits(_one_user(csr, u, state, f, 3), got[0][u]), u


def test_cg_and_the_exact_solvers_share_one_csr():
    """CG, Cholesky, CG (and the explicit half-step) on one Model and one DeviceCSR equal the same steps on fresh objects bit for
    bit; one DeviceCSR serves CG at f = 8, Cholesky at f = 252 and CG at f = 8 again (g0, its dense copy and the workspace regrown
    and reused)."""
    tr, _ = synth.make_ratings(300, 80, 5000, min_degree=2, seed=85)
    start = random_state(tr.rows, tr.cols, 16, 3000)
    last = interplay([lambda m, d: m.ials(d, HYPER, 40.0, "users", solver="cg", cg_steps=3),
                      lambda m, d: m.ials(d, HYPER, 40.0, "items"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "items", solver="cg", cg_steps=2),
                      lambda m, d: m.als(d, achk.HYPER, "users"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "both", solver="cg", cg_steps=1),
                      lambda m, d: m.implicit_objective(d, HYPER, 40.0)], tr, 16, state=start)
    assert all(np.isfinite(a).all() for a in last)
    csr = achk.batch_set(40, 17).transpose()
    shared = cu.DeviceCSR(csr)
    for step, (f, solver) in enumerate(((8, "cg"), (252, "cholesky"), (8, "cg"), (252, "cg"), (100, "cg"))):
        state = random_state(csr.rows, csr.cols, f, 3200 + step)
        results = []
        for d in (shared, cu.DeviceCSR(csr)):
            m = model_from(state, 0.0)
            assert m.ials(d, HYPER, 40.0, "both", solver=solver, cg_steps=3) == 0
            results.append(m.download())
        assert same_state(*results), (step, f, solver)


@pytest.mark.parametrize("name", sorted(cgchk.unsolved_cases()))
def test_rows_that_hold_a_bad_entry_keep_their_bits_and_are_counted(name):
    """One entry NaN and one +inf (poison-entry), one weight alpha r = +inf (overflow): exactly the rows that hold it are left as
    they were and counted; every other row is judged."""
    case, bad = cgchk.unsolved_cases()[name]
    model = model_from(case.state(), case.csr.global_bias)
    report = {}
    check_cg_half_step(model, cu.DeviceCSR(case.csr), case.csr, case.side, case.hyper, case.alpha, 3, report=report, may_fail=bad)
    assert report["unsolved"] == len(bad) and np.array_equal(report["kept"], np.sort(bad)), (name, report["unsolved"], report["kept"], bad)


def test_objective_never_rises_on_ml_small():
    hyper, alpha, f = (0.01, 0.1, 0.1, 0.0, 0.0), 40.0, 32
    tr = cu.createSparseMatrix(ml_small())
    d = cu.DeviceCSR(tr)
    final = {}
    for solver in ("cg", "cholesky"):
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        states = [model.download()]
        for _ in range(5):
            for side in ("users", "items"):
                assert model.ials(d, hyper, alpha, side, solver=solver, cg_steps=3) == 0
                states.append(model.download())
        L = [ref.objective(tr, s[0], s[1], hyper, alpha) for s in states]
        final[solver] = L[-1]
        for k in range(1, len(L)):
            assert L[k] <= L[k - 1], (solver, k, L[k - 1], L[k])
        assert L[-1] < 0.5 * L[0]
    print("ML_SMALL, f = 32, 5 sweeps: objective %.6g (CG, 3 steps) against %.6g (Cholesky)" % (final["cg"], final["cholesky"]))


def test_train_ials_cg_equals_the_sweeps(capfd):
    tr, te = synth.make_ratings(300, 80, 5000, min_degree=2, seed=51)
    f, alpha = 12, 10.0
    cfg = api.default_config(total_iterations=5, n_factors=f, check_error=2, patience=0.0, learning_rate=0.125, P_reg=HYPER[1],
                             Q_reg=HYPER[2])
    capfd.readouterr()
    P, Q, objectives, ub, ib, stats = cu.train(tr, None, cfg, mode="ials", alpha=alpha, verbose=True, return_stats=True, solver="cg",
                                               cg_steps=2)
    out = capfd.readouterr().out
    assert cfg.learning_rate == np.float32(0.125) and cfg.cur_iterations == 5 and "New Learning Rate" not in out
    lines = [l for l in out.splitlines() if l.startswith("TRAIN:")]
    assert [l.split()[2] for l in lines] == ["1", "2", "4", "5"] and all("implicit objective" in l for l in lines), lines
    assert not [l for l in out.splitlines() if l.startswith("TEST:")]
    checked = [0, 1, 3, 4]
    assert objectives.dtype == np.float64 and np.isfinite(objectives[checked]).all() and np.isnan(np.delete(objectives, checked)).all()
    d = cu.DeviceCSR(tr)
    m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    hyper = (0.0, HYPER[1], HYPER[2], 0.0, 0.0)
    assert m.ials(d, hyper, alpha, "both", sweeps=5, solver="cg", cg_steps=2) == 0
    assert same_state((P, Q, ub, ib), m.download())
    exact = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    assert exact.ials(d, hyper, alpha, "both", sweeps=5) == 0
    assert not same_bits(exact.download()[0], P)  # CG really ran
    assert objectives[4] == m.implicit_objective(d, hyper, alpha)
    assert all(b <= a for a, b in zip(objectives[checked], objectives[checked][1:]))
    rows = int((np.diff(tr.indptr) > 0).sum()) + int((np.bincount(tr.indices, minlength=tr.cols) > 0).sum())
    assert stats.updates == 5 * rows
    # is_train = 0: the item side is frozen bit for bit
    cfg2 = api.default_config(total_iterations=2, n_factors=f, check_error=10, is_train=0, P_reg=HYPER[1], Q_reg=HYPER[2])
    P2, Q2, _, _, ib2 = cu.train(tr, None, cfg2, mode="ials", alpha=alpha, verbose=False, solver="cg", cg_steps=2)
    init = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    _, Q0, _, ib0 = init.download()
    assert same_bits(Q2, Q0) and same_bits(ib2, ib0)
    assert init.ials(d, hyper, alpha, "users", sweeps=2, solver="cg", cg_steps=2) == 0
    assert same_bits(P2, init.download()[0])


def test_bin_mf_ials_C(tmp_path):
    mf = os.path.join(ROOT, "bin", "mf")
    tr0, te0 = synth.make_ratings(200, 50, 3000, min_degree=3, seed=61)
    synth.write_csv(str(tmp_path / "train.csv"), tr0)
    synth.write_csv(str(tmp_path / "test.csv"), te0)
    f = 8
    hyper = (0.01, 0.3, 0.2, 0.02, 0.03)
    (tmp_path / "c.cfg").write_text("0 4 %d 0.01 42 %g %g %g %g\n" % ((f,) + hyper[1:]))
    files = [str(tmp_path / "train.csv"), str(tmp_path / "test.csv")]
    res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "ials", "-a", "10", "-C", "3"] + files, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    assert "implicit objective" in res.stdout and "TEST: Iteration" not in res.stdout
    tr = cu.createSparseMatrix(str(tmp_path / "train.csv"))
    cfg = api.default_config(total_iterations=4, n_factors=f, P_reg=hyper[1], Q_reg=hyper[2], user_bias_reg=hyper[3], item_bias_reg=hyper[4])
    want = cu.train(tr, None, cfg, mode="ials", alpha=10.0, verbose=False, solver="cg", cg_steps=3)
    exact = cu.train(tr, None, api.default_config(total_iterations=4, n_factors=f, P_reg=hyper[1], Q_reg=hyper[2]), mode="ials",
                     alpha=10.0, verbose=False)
    assert not np.allclose(want[0], exact[0], rtol=1e-5, atol=1e-6)  # the files below are CG's, not the exact solver's
    pre = str(tmp_path / ("train_f%d_" % f))
    for name, w in zip(("p", "q", "user_bias", "item_bias"), (want[0], want[1], want[3], want[4])):
        got = cu.read_array(pre + name + ".csv").reshape(w.shape)
        assert np.allclose(got, w, rtol=1e-5, atol=1e-6), name
    for args in (["-C", "3"], ["-m", "als", "-C", "3"], ["-m", "ials", "-C", "three"], ["-m", "ials", "-C", "0"], ["-m", "ials", "-C", "257"]):
        res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg")] + args + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)


def test_errors_leave_the_model_alone():
    tr, _ = synth.make_ratings(100, 40, 1500, min_degree=2, seed=41)
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, 8, tr.global_bias)
    before = model.download()
    for steps in (0, -1, 257):
        assert ials_cg(model, d, HYPER, 40.0, "users", steps)[0] == EINVAL, steps
        with pytest.raises(cu.Cu2recError):
            model.ials(d, HYPER, 40.0, "users", solver="cg", cg_steps=steps)
        with pytest.raises(cu.Cu2recError):
            cu.train(tr, None, api.default_config(total_iterations=1, n_factors=8, P_reg=0.5, Q_reg=0.5), mode="ials", verbose=False,
                     solver="cg", cg_steps=steps)
    lr, P_reg, Q_reg, ubr, ibr = HYPER
    for hyper, alpha, side in (((lr, 0.0, Q_reg, ubr, ibr), 40.0, "users"), ((lr, P_reg, np.nan, ubr, ibr), 40.0, "items"),
                               (HYPER, -1.0, "users"), (HYPER, np.inf, "items"), (HYPER, 40.0, 2)):
        assert ials_cg(model, d, hyper, alpha, side, 3)[0] == EINVAL, (hyper, alpha, side)
    h = cu.Hyper(*HYPER)
    L = lib()
    assert L.cu2rec_model_als_implicit_cg(None, d._h, C.byref(h), 40.0, 0, 3, None) == EINVAL
    assert L.cu2rec_model_als_implicit_cg(model._h, None, C.byref(h), 40.0, 0, 3, None) == EINVAL
    assert L.cu2rec_model_als_implicit_cg(model._h, d._h, None, 40.0, 0, 3, None) == EINVAL
    small = cu.Model(tr.rows, tr.cols - 1, 8, 0.0)
    kept = small.download()
    assert ials_cg(small, d, HYPER, 40.0, "users", 3)[0] == EINVAL and same_state(small.download(), kept)
    with pytest.raises(ValueError):
        model.ials(d, HYPER, 40.0, "users", solver="qr")
    with pytest.raises(ValueError):
        cu.train(tr, None, api.default_config(total_iterations=1, n_factors=8), mode="ials", verbose=False, solver="")
    assert same_state(model.download(), before)
    wide = cu.Model(tr.rows, tr.cols, 253, tr.global_bias)
    wide_before = wide.download()
    assert ials_cg(wide, d, HYPER, 40.0, "users", 3)[0] == EUNSUPPORTED
    assert same_state(wide.download(), wide_before)
    assert ials_cg(model, d, HYPER, 40.0, "users", 256) == (0, 0)  # CU2REC_ALS_CG_MAX_STEPS itself, and the same objects still work
    assert L.cu2rec_model_als_implicit_cg(model._h, d._h, C.byref(h), 40.0, 1, 1, None) == 0  # unsolved may be NULL


def test_the_default_is_the_exact_solver():
    case = cgchk.cases()["lengths-f31-users"]
    d = cu.DeviceCSR(case.csr)
    out = []
    for kw in ({}, {"solver": "cholesky"}, {"solver": "cholesky", "cg_steps": 0}):
        m = model_from(case.state(), 0.0)
        assert m.ials(d, HYPER, 40.0, "both", **kw) == 0
        out.append(m.download())
    m = model_from(case.state(), 0.0)
    for side in ("users", "items"):
        assert ials(m, d, HYPER, 40.0, side) == (0, 0)
    out.append(m.download())
    m = model_from(case.state(), 0.0)
    assert m.ials(d, HYPER, 40.0, "both", solver="cg") == 0  # cg_steps defaults to 3
    cg = m.download()
    assert all(same_state(out[0], o) for o in out[1:]) and not same_bits(cg[0], out[0][0])
    m = model_from(case.state(), 0.0)
    assert m.ials(d, HYPER, 40.0, "both", solver="cg", cg_steps=3) == 0
    assert same_state(cg, m.download())
