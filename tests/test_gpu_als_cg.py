"""The explicit conjugate-gradient half-step on the GPU (cu2rec_model_als_cg, cu2rec_train_als_cg, bin/mf -m alscg, Model.als(solver="cg"),
train(mode="als", solver="cg")) against the float64 iteration of tests/als_cg_reference64.py.

The bar for a row x = [factors; bias] of 1 .. 1,024 ratings is the project's, max |x - x*| <= 1e-3 max(1, |x*|_inf), with x* the
float64 CG iterate after the same number of steps from the same float32 state; tests/test_als_cg_cpu.py shows on the CPU that a
float32 restatement in operator form is within half of it on every row judged here (at no more than 0.018 of it on the width x
length grid from f = 31 on, 0.44 at f = 8) and that seven deliberate mistakes miss it by more than two bars.  Longer rows are solved exactly: bit for bit what
cu2rec_model_als writes.  The sets and the judge live in tests/als_cg_checks.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib
from conftest import ROOT, ml_small

import als_cg_checks as cgchk
import als_cg_reference64 as cgref
import als_checks as achk
import als_reference64 as ref
from als_cg_checks import als_cg, check_cg_half_step
from als_checks import HYPER, als, model_from, own_major, random_state, same_bits, same_state
from ials_checks import bar_ratio

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6


@pytest.mark.parametrize("name", sorted(cgchk.cases()))
def test_half_step_matches_float64_cg(name):
    """Widths 1, 8, 31, 100, 252 and both edges of every per-lane element count of the order-(f + 1) vectors (62 | 63 | 64,
    126 | 127 | 128, 190 | 191 | 192) x rows of 1 .. 4,097 ratings on both sides, and the messy set; 1, 2 and 3 steps."""
    case = cgchk.cases()[name]
    d = cu.DeviceCSR(case.csr)
    rows, want = cgchk.reference(case)
    report = {}
    for steps in cgchk.STEPS:
        model = model_from(case.state(), case.csr.global_bias)
        check_cg_half_step(model, case, d, steps, want=(rows, want[steps - 1]), judged=cgchk.fair_rows(case, steps), report=report)
    print("%s: worst row at %s of the bar after 1, 2, 3 steps; long rows at %.3g" % (
        name, ", ".join("%.3g" % report[(case.side, case.f, s)] for s in cgchk.STEPS), report[(case.side, case.f, "long")]))


@pytest.mark.parametrize("f", [8, 100])
def test_the_cut_between_cg_and_the_exact_rows(f):
    """Rows of 1,025 .. 4,097 ratings come out bit for bit as cu2rec_model_als writes them from the same state, whatever cg_steps
    is; the row of 1,024 ratings is CG's (judged by the CG reference at one step, and not the exact solution's bits)."""
    case = cgchk.cases()["lengths-f%d-users" % f]
    csr, d = case.csr, cu.DeviceCSR(case.csr)
    n = np.diff(csr.indptr)
    long_rows, at_cut = np.flatnonzero(n > cgchk.CHUNK), int(np.flatnonzero(n == cgchk.CHUNK)[0])
    assert sorted(n[long_rows]) == [1025, 2047, 2048, 2049, 4097]
    exact = model_from(case.state(), csr.global_bias)
    assert als(exact, d, case.hyper, "users") == (0, 0)
    Pe, _, ube, _ = exact.download()
    rows, want = cgchk.reference(case)
    for steps in (1, 2, 3, 7):
        m = model_from(case.state(), csr.global_bias)
        assert als_cg(m, d, case.hyper, "users", steps) == (0, 0)
        Pc, _, ubc, _ = m.download()
        assert same_bits(Pc[long_rows], Pe[long_rows]) and same_bits(ubc[long_rows], ube[long_rows]), (f, steps)
        assert not same_bits(Pc[at_cut], Pe[at_cut])
        if steps == 1:
            k = int(np.flatnonzero(rows == at_cut)[0])
            x = np.concatenate([Pc[at_cut], ubc[at_cut:at_cut + 1]])[None, :]
            assert bar_ratio(x, want[0][k:k + 1]) <= 1.0


@pytest.mark.parametrize("name", sorted(cgchk.conditioning_cases()))
def test_conditioning(name):
    """Bias regulariser 0, factor regulariser 1e-4 and 10, partners scaled by 2^-20 and 2^10 at f = 8: every class at every step count
    is held to the bar, except those of als_cg_checks.CONDITIONING_UNFAIR (the float32 restatement itself is off there); their rows
    must come back finite and solved."""
    case, judged = cgchk.conditioning_cases()[name][:2]
    d = cu.DeviceCSR(case.csr)
    report = {}
    for steps in cgchk.STEPS:
        model = model_from(case.state(), case.csr.global_bias)
        check_cg_half_step(model, case, d, steps, judged=judged[steps], report=report, judge_long=False)
    print("%s: worst judged row at %s of the bar after 1, 2, 3 steps" % (name, ", ".join("%.3g" % report[(case.side, 8, s)] for s in cgchk.STEPS)))


@pytest.mark.parametrize("name", sorted(cgchk.unsolved_cases()))
def test_rows_that_hold_a_bad_value_keep_their_bits_and_are_counted(name):
    """A NaN and a +inf rating, and a partner row that overflows: exactly the rows that read them are left as they were and counted;
    every other row is judged.  Three rows whose own factors or bias hold a NaN or an inf are solved from zero."""
    case, bad, nan_start = cgchk.unsolved_cases()[name]
    d = cu.DeviceCSR(case.csr)
    model = model_from(case.state(), case.csr.global_bias)
    report = {}
    got = check_cg_half_step(model, case, d, 3, may_fail=bad, report=report)
    assert report["unsolved"] == len(bad) and np.array_equal(report["kept"], bad), (name, report["unsolved"], report["kept"], bad)
    zeroed = case.state()
    Y, yb = (zeroed[0], zeroed[2]) if case.side == "users" else (zeroed[1], zeroed[3])
    Y[nan_start], yb[nan_start] = 0.0, 0.0
    m = model_from(zeroed, case.csr.global_bias)
    assert als_cg(m, d, case.hyper, case.side, 3) == (0, len(bad))
    from_zero = m.download()
    own = (0, 2) if case.side == "users" else (1, 3)
    for k in own:
        assert same_bits(got[k][nan_start], from_zero[k][nan_start]) and np.isfinite(got[k][nan_start]).all(), name


def _one_user(csr, u, state, f, steps, hyper=HYPER):
    """User u solved from a one-user CSR of the same cols and global bias, from its row of `state`."""
    P, Q, ub, ib = state
    lo, hi = csr.indptr[u], csr.indptr[u + 1]
    one = api.HostCSR([0, hi - lo], csr.indices[lo:hi], csr.data[lo:hi], 1, csr.cols, csr.global_bias)
    m = cu.Model(1, Q.shape[0], f, csr.global_bias, P=P[u:u + 1], Q=Q, user_bias=ub[u:u + 1], item_bias=ib)
    assert als_cg(m, cu.DeviceCSR(one), hyper, "users", steps) == (0, 0)
    got = m.download()
    return got[0][0], got[2][0]


@pytest.mark.parametrize("f", [100, 252])
def test_deterministic_and_independent_of_the_other_rows(f):
    csr = achk.width_length_set()
    d = cu.DeviceCSR(csr)
    state = random_state(csr.rows, csr.cols, f, 78)
    runs = []
    for _ in range(2):
        m = model_from(state, csr.global_bias)
        assert m.als(d, HYPER, "both", sweeps=2, solver="cg", cg_steps=3) == 0
        runs.append(m.download())
    assert same_state(*runs), "two runs differ"
    batch = model_from(runs[0], csr.global_bias)
    assert batch.als(d, HYPER, "users", solver="cg", cg_steps=3) == 0
    Pb, _, ubb, _ = batch.download()
    # the first and the last wavefront of a workgroup (rows 4 k and 4 k + 3), long rows, the last row
    for u in [0, 3, 4, 7, 8, 9, 10, 11, 50, 208, 211]:
        p, b = _one_user(csr, u, runs[0], f, 3)
        assert same_bits(p, Pb[u]) and same_bits(b, ubb[u]), u


@pytest.mark.parametrize("f", [8, 100, 191])
def test_item_half_step_is_the_user_half_step_of_the_transposed_problem(f):
    csr = achk.width_length_set()
    P, Q, ub, ib = random_state(csr.rows + 2, csr.cols + 3, f, 79)
    lr, P_reg, Q_reg, ubr, ibr = HYPER
    for steps in (1, 3):
        m = model_from((P, Q, ub, ib), csr.global_bias)
        assert als_cg(m, cu.DeviceCSR(csr), HYPER, "items", steps) == (0, 0)
        t = model_from((Q, P, ib, ub), csr.global_bias)
        assert als_cg(t, cu.DeviceCSR(csr.transpose()), (lr, Q_reg, P_reg, ibr, ubr), "users", steps) == (0, 0)
        Pm, Qm, ubm, ibm = m.download()
        assert same_state((Pm, Qm, ubm, ibm), tuple(t.download()[k] for k in (1, 0, 3, 2))), (f, steps)
        assert not same_bits(Qm, Q)


@pytest.mark.parametrize("rows", [cgchk.SLOTS - 1, cgchk.SLOTS, cgchk.SLOTS + 1, 2 * cgchk.SLOTS + 1])
def test_row_counts_around_one_workgroup(rows):
    """3, 4, 5 and 9 rows (four wavefronts = four rows per workgroup): every row judged, every row equal to its one-row solve."""
    full = achk.width_length_set()
    keep = [12 + 7 * i for i in range(rows)]
    per_row = [full.indices[full.indptr[u]:full.indptr[u + 1]] for u in keep]
    data = np.concatenate([full.data[full.indptr[u]:full.indptr[u + 1]] for u in keep])
    csr = achk.csr_from_rows(per_row, full.cols, None, gb=full.global_bias, ratings=data)
    f = 31
    state = random_state(rows, csr.cols, f, 910 + rows)
    case = cgchk.Case("rows-%d" % rows, csr, "users", f, HYPER, state=state)
    got = check_cg_half_step(model_from(state, csr.global_bias), case, cu.DeviceCSR(csr), 2)
    for u in range(rows):
        p, b = _one_user(csr, u, state, f, 2)
        assert same_bits(p, got[0][u]) and same_bits(b, got[2][u]), (rows, u)


def test_more_rows_than_one_grid_pass():
    """20,000 rows of 1 .. 4 ratings at f = 8, three steps: the kernel's grid-stride loop takes three trips.  A sample is judged in
    float64, rows on both sides of every trip's edge and the last row are pinned by their one-row CSRs."""
    csr = cgchk.many_rows_set()
    f = cgchk.MANY_ROWS_F
    state = random_state(csr.rows, csr.cols, f, cgchk.MANY_ROWS_SEED)
    case = cgchk.Case("many-rows", csr, "users", f, HYPER, state=state)
    m = model_from(state, csr.global_bias)
    assert als_cg(m, cu.DeviceCSR(csr), HYPER, "users", 3) == (0, 0)
    got = m.download()
    assert same_bits(got[1], state[1]) and same_bits(got[3], state[3])
    edges, sample = cgchk.many_rows_sample()
    want = cgref.cg_rows(*case.system_of(state), 3, rows=sample)
    x = np.concatenate([got[0], got[2][:, None]], axis=1)
    ratio = bar_ratio(x[sample], want)
    print("20,000 rows: %d sampled rows at %.3g of the bar" % (len(sample), ratio))
    assert ratio <= 1.0
    moved = (got[0].view(np.uint32) != state[0].view(np.uint32)).any(axis=1) & (got[2].view(np.uint32) != state[2].view(np.uint32))
    assert moved.all(), "rows the kernel never reached: %s" % np.flatnonzero(~moved)[:8]
    for u in edges:
        p, b = _one_user(csr, u, state, f, 3)
        assert same_bits(p, got[0][u]) and same_bits(b, got[2][u]), u


def test_sixteen_steps_reach_the_exact_optimum():
    case = cgchk.cases()["lengths-f8-users"]
    state = case.state()
    m = model_from(state, case.csr.global_bias)
    assert als_cg(m, cu.DeviceCSR(case.csr), case.hyper, "users", 16) == (0, 0)
    indptr, indices, data, X, xb, gb, reg, reg_b, _ = case.system_of(state)
    rows = cgchk.cg_rows_of(indptr)
    want = np.array([np.linalg.solve(*ref.system(indptr, indices, data, np.asarray(X, np.float64), np.asarray(xb, np.float64), gb, reg,
                                                 reg_b, int(r))) for r in rows])
    got = m.download()
    ratio = bar_ratio(np.concatenate([got[0], got[2][:, None]], axis=1)[rows], want)
    print("f=8: 16 CG steps at %.3g of the bar from the float64 optimum" % ratio)
    assert ratio <= 1.0, ratio


def _ml_small_split():
    full = cu.createSparseMatrix(ml_small())
    pos = np.arange(full.nnz) - np.repeat(full.indptr[:-1], np.diff(full.indptr))
    test = pos % 5 == 4  # every fifth rating of each user
    users = np.repeat(np.arange(full.rows), np.diff(full.indptr))

    def part(mask):
        indptr = np.zeros(full.rows + 1, np.int64)
        indptr[1:] = np.cumsum(np.bincount(users[mask], minlength=full.rows))
        return api.HostCSR(indptr, full.indices[mask], full.data[mask], full.rows, full.cols, full.global_bias)
    return part(~test), part(test)


def _half_step_slack(tr, before, after, side):
    """als_reference64.objective_slack summed over the rows the half-step moved: how far rounding may lift the objective."""
    indptr, indices, data = own_major(tr, side)
    own, other = ((0, 2), (1, 3)) if side == "users" else ((1, 3), (0, 2))
    reg, reg_b = (HYPER[1], HYPER[3]) if side == "users" else (HYPER[2], HYPER[4])
    slack = 0.0
    for r in np.flatnonzero(np.diff(indptr) > 0):
        x_new = np.append(after[own[0]][r], after[own[1]][r])
        x_old = np.append(before[own[0]][r], before[own[1]][r])
        bound = ref.row_residual(indptr, indices, data, before[other[0]], before[other[1]], tr.global_bias, reg, reg_b, int(r), x_new)[3]
        slack += ref.objective_slack(bound, x_new, x_old)
    return slack


def test_objective_never_rises_on_ml_small():
    """Five sweeps at three steps, f = 32, from the seed-42 initial model: the float64 objective after a half-step is never above
    the one before it by more than als_reference64.objective_slack summed over the half-step's rows (evaluated only where the
    objective did not fall), and it ends below its start.  The test RMSE next to exact ALS's is printed, not asserted."""
    tr, te = _ml_small_split()
    d = cu.DeviceCSR(tr)
    rmse = {}
    for solver in ("cg", "cholesky"):
        model = cu.Model(tr.rows, tr.cols, 32, tr.global_bias)
        states = [model.download()]
        for _ in range(5):
            for side in ("users", "items"):
                assert model.als(d, HYPER, side, solver=solver, cg_steps=3) == 0
                states.append(model.download())
        rmse[solver] = ref.rmse(te, *states[-1], tr.global_bias)
        if solver == "cg":
            L = [ref.objective(tr, *s, tr.global_bias, HYPER) for s in states]
            for k in range(1, len(L)):
                if L[k] > L[k - 1]:
                    slack = _half_step_slack(tr, states[k - 1], states[k], "users" if k % 2 else "items")
                    assert L[k] <= L[k - 1] + slack, (k, L[k - 1], L[k], slack)
            assert L[-1] < L[0], L
    print("ML_SMALL, f = 32, 5 sweeps: objective %.6g -> %.6g; test RMSE %.4f (CG, 3 steps) against %.4f (Cholesky)"
          % (L[0], L[-1], rmse["cg"], rmse["cholesky"]))


def test_train_als_cg_equals_the_sweeps(capfd):
    tr, te = synth.make_ratings(300, 80, 5000, min_degree=2, seed=51)
    f = 12
    cfg = api.default_config(total_iterations=5, n_factors=f, check_error=2, patience=0.0, learning_rate=0.125,
                             P_reg=HYPER[1], Q_reg=HYPER[2], user_bias_reg=HYPER[3], item_bias_reg=HYPER[4])
    capfd.readouterr()
    P, Q, losses, ub, ib, stats = cu.train(tr, te, cfg, mode="als", verbose=True, return_stats=True, solver="cg", cg_steps=2)
    out = capfd.readouterr().out
    assert cfg.learning_rate == np.float32(0.125) and cfg.cur_iterations == 5 and "New Learning Rate" not in out
    lines = [l for l in out.splitlines() if l.startswith(("TRAIN:", "TEST:"))]
    assert [l.split()[2] for l in lines] == ["1", "1", "2", "2", "4", "4", "5", "5"], lines
    checked = [0, 1, 3, 4]
    assert np.isfinite(losses[checked]).all() and np.isnan(np.delete(losses, checked)).all()
    d = cu.DeviceCSR(tr)
    m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    assert m.als(d, HYPER, "both", sweeps=5, solver="cg", cg_steps=2) == 0
    assert same_state((P, Q, ub, ib), m.download())
    assert losses[4] == np.float32(m.loss(cu.DeviceCSR(te))["rmse"])
    exact = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    assert exact.als(d, HYPER, "both", sweeps=5) == 0
    assert not same_bits(exact.download()[0], P)  # CG really ran
    rows = len(achk.rows_with_ratings(tr, "users")) + len(achk.rows_with_ratings(tr, "items"))
    assert stats.updates == 5 * rows
    # is_train = 0: the item side is frozen bit for bit; the users are their CG half-steps against it
    cfg2 = api.default_config(total_iterations=2, n_factors=f, check_error=10, is_train=0, P_reg=HYPER[1], Q_reg=HYPER[2],
                              user_bias_reg=HYPER[3], item_bias_reg=HYPER[4])
    P2, Q2, _, ub2, ib2 = cu.train(tr, te, cfg2, mode="als", verbose=False, solver="cg", cg_steps=2)
    init = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    _, Q0, _, ib0 = init.download()
    assert same_bits(Q2, Q0) and same_bits(ib2, ib0)
    assert init.als(d, HYPER, "users", sweeps=2, solver="cg", cg_steps=2) == 0
    Pw, _, ubw, _ = init.download()
    assert same_bits(P2, Pw) and same_bits(ub2, ubw)


def test_bin_mf_alscg(tmp_path):
    mf = os.path.join(ROOT, "bin", "mf")
    tr0, te0 = synth.make_ratings(200, 50, 3000, min_degree=3, seed=61)
    synth.write_csv(str(tmp_path / "train.csv"), tr0)
    synth.write_csv(str(tmp_path / "test.csv"), te0)
    f = 8
    (tmp_path / "c.cfg").write_text("0 4 %d 0.01 42 %g %g %g %g\n" % ((f,) + HYPER[1:]))
    files = [str(tmp_path / "train.csv"), str(tmp_path / "test.csv")]
    tr, te = cu.createSparseMatrix(files[0]), cu.createSparseMatrix(files[1])
    pre = str(tmp_path / ("train_f%d_" % f))

    def config():
        return api.default_config(total_iterations=4, n_factors=f, P_reg=HYPER[1], Q_reg=HYPER[2], user_bias_reg=HYPER[3],
                                  item_bias_reg=HYPER[4])
    exact = cu.train(tr, te, config(), mode="als", verbose=False)
    for args, steps in ((["-C", "3"], 3), ([], 3), (["-C", "1"], 1)):  # -C defaults to 3
        res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "alscg"] + args + files, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert res.returncode == 0, res.stderr
        assert "TEST: Iteration" in res.stdout and "New Learning Rate" not in res.stdout
        want = cu.train(tr, te, config(), mode="als", verbose=False, solver="cg", cg_steps=steps)
        assert not np.allclose(want[0], exact[0], rtol=1e-5, atol=1e-6)  # the files below are CG's, not the exact solver's
        for name, w in zip(("p", "q", "user_bias", "item_bias"), (want[0], want[1], want[3], want[4])):
            got = cu.read_array(pre + name + ".csv").reshape(w.shape)
            assert np.allclose(got, w, rtol=1e-5, atol=1e-6), (name, args)
        assert np.isclose(cu.read_array(pre + "global_bias.csv")[0, 0], tr.global_bias)
    for args in (["-m", "alscg", "-C", "0"], ["-m", "alscg", "-C", "257"], ["-m", "alscg", "-C", "x"], ["-m", "als", "-C", "3"]):
        res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg")] + args + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)


def test_errors_leave_the_model_alone():
    tr, te = synth.make_ratings(100, 40, 1500, min_degree=2, seed=41)
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, 8, tr.global_bias)
    before = model.download()
    for steps in (0, -1, 257):
        assert als_cg(model, d, HYPER, "users", steps)[0] == EINVAL, steps
        with pytest.raises(cu.Cu2recError):
            model.als(d, HYPER, "users", solver="cg", cg_steps=steps)
        with pytest.raises(cu.Cu2recError):
            cu.train(tr, te, api.default_config(total_iterations=1, n_factors=8), mode="als", verbose=False, solver="cg", cg_steps=steps)
    lr, P_reg, Q_reg, ubr, ibr = HYPER
    for hyper, side in (((lr, 0.0, Q_reg, ubr, ibr), "users"), ((lr, np.nan, Q_reg, ubr, ibr), "users"), ((lr, P_reg, 0.0, ubr, ibr), "items"),
                        ((lr, P_reg, np.inf, ubr, ibr), "items"), ((lr, P_reg, Q_reg, -0.5, ibr), "users"),
                        ((lr, P_reg, Q_reg, ubr, np.nan), "items")):
        assert als_cg(model, d, hyper, side, 3)[0] == als(model, d, hyper, side)[0] == EINVAL, (hyper, side)
    for side in (2, -1):
        assert als_cg(model, d, HYPER, side, 3)[0] == EINVAL, side
    h = cu.Hyper(*HYPER)
    L = lib()
    assert L.cu2rec_model_als_cg(None, d._h, C.byref(h), 0, 3, None) == EINVAL
    assert L.cu2rec_model_als_cg(model._h, None, C.byref(h), 0, 3, None) == EINVAL
    assert L.cu2rec_model_als_cg(model._h, d._h, None, 0, 3, None) == EINVAL
    small = cu.Model(tr.rows - 1, tr.cols, 8, tr.global_bias)  # ratings past the model's users
    kept = small.download()
    assert als_cg(small, d, HYPER, "users", 3)[0] == als(small, d, HYPER, "users")[0] == EINVAL and same_state(small.download(), kept)
    with pytest.raises(ValueError):
        model.als(d, HYPER, "users", solver="qr")
    with pytest.raises(ValueError):
        cu.train(tr, te, api.default_config(total_iterations=1, n_factors=8), mode="als", verbose=False, solver="")
    assert same_state(model.download(), before)
    wide = cu.Model(tr.rows, tr.cols, 253, tr.global_bias)
    wide_before = wide.download()
    assert als_cg(wide, d, HYPER, "users", 3)[0] == EUNSUPPORTED and same_state(wide.download(), wide_before)
    assert L.cu2rec_model_als_cg(model._h, d._h, C.byref(h), 1, 1, None) == 0  # unsolved may be NULL, and the same objects still work


def test_the_default_is_the_exact_solver():
    case = cgchk.cases()["lengths-f31-users"]
    d = cu.DeviceCSR(case.csr)
    gb = case.csr.global_bias
    out = []
    for kw in ({}, {"solver": "cholesky"}, {"solver": "cholesky", "cg_steps": 0}):
        m = model_from(case.state(), gb)
        assert m.als(d, HYPER, "both", **kw) == 0
        out.append(m.download())
    m = model_from(case.state(), gb)
    for side in ("users", "items"):
        assert als(m, d, HYPER, side) == (0, 0)
    out.append(m.download())
    m = model_from(case.state(), gb)
    assert m.als(d, HYPER, "both", solver="cg") == 0  # cg_steps defaults to 3
    cg = m.download()
    assert all(same_state(out[0], o) for o in out[1:]) and not same_bits(cg[0], out[0][0])
    m = model_from(case.state(), gb)
    assert m.als(d, HYPER, "both", solver="cg", cg_steps=3) == 0
    assert same_state(cg, m.download())
