"""Softmax matrix factorization on the GPU (cu2rec_model_softmax, _gradient, _objective, _lse, _mass, cu2rec_train_softmax,
bin/mf -m softmax) against the float64 reference of tests/softmax_reference64.py.

The log-sum-exp, sum_i pi and every gradient value are judged entrywise by the bounds derived in that module: tests/test_softmax_cpu.py
shows on the CPU that a float32 restatement of the kernels' arithmetic stays below 0.18 of them on every set judged here and that ten
deliberate mistakes in the model exceed them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib
from conftest import ROOT, ml_small

import softmax_checks as chk
import softmax_reference64 as ref
from als_checks import model_from, same_bits, same_state

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_lse_mass_and_gradient_match_float64(name):
    """Every width of lmf_checks.WIDTHS, own-row count of OWN_ROWS and partner count of PARTNERS, rows of 0, 1, 2 and 300 unsorted
    entries with repeated pairs, cols past every stored item, on both sides, and the large-score, dominated and empty-user sets:
    lse_u, sum_i pi_ui (the dense pass's column f) and every gradient value within the derived bounds, the users' bias gradient
    exact zeros.  The model (its rows past the CSR too) and the accumulators keep their bits, and a second call returns the same
    bits."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, case.gb)
    d = cu.DeviceCSR(case.csr)
    lse, mass = model.softmax_lse(d), model.softmax_mass(d)
    got = model.softmax_gradient(d, case.hyper, case.side)
    r = {"lse": chk.judge_lse(case, state, lse), "mass": chk.judge_mass(case, state, mass), "gradient": chk.judge(case, state, got)}
    print("%s: worst values at %s of the bounds" % (name, {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) <= 1.0, (name, r)
    assert np.isfinite(lse).all() and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    if case.side == "users":
        assert not got[1].any()
    assert same_state(model.download(), state)
    assert all(not a.any() for a in model.lmf_state())
    again = model.softmax_gradient(d, case.hyper, case.side)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1])
    assert same_bits(lse, model.softmax_lse(d)) and same_bits(mass, model.softmax_mass(d))


@pytest.mark.parametrize("name", ["f100-65x1000", "f31-33x129", "f224-33x1000", "large-score-users"])
def test_a_user_alone_has_the_lse_and_gradient_it_has_among_the_others(name):
    case = chk.cases()[name]
    P, Q, ub, ib = case.state()
    d = cu.DeviceCSR(case.csr)
    model = model_from((P, Q, ub, ib), case.gb)
    lse, full = model.softmax_lse(d), model.softmax_gradient(d, case.hyper, "users")
    for u in (0, 1, case.csr.rows - 1):
        one = cu.DeviceCSR(case.csr.slice_users(u, u + 1))
        alone = model_from((P[u:u + 1], Q, ub[u:u + 1], ib), case.gb)
        assert same_bits(alone.softmax_lse(one), lse[u:u + 1]), u
        assert same_bits(alone.softmax_gradient(one, case.hyper, "users")[0][0], full[0][u]), u


def _own(state, side):
    P, Q, ub, ib = state
    return (P, ub) if side == "users" else (Q, ib)


@pytest.mark.parametrize("name", ["f100-65x1000", "f63-1x31-items", "f252-65x31-items", "empty-user", "empty-user-items"])
def test_one_side_moves_per_half_step_by_the_adagrad_step_of_its_gradient(name):
    """x' and a' of the side's rows inside the CSR against the float64 step from the device's own gradient (four correctly rounded
    float32 operations, tests/test_lmf_cpu.py); the other side, the rows past the CSR, the user biases and their accumulators keep
    their bits."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, case.gb)
    d = cu.DeviceCSR(case.csr)
    side, lr = case.side, float(np.float32(case.hyper[0]))
    n = case.csr.rows if side == "users" else case.csr.cols
    other = "items" if side == "users" else "users"
    before, acc0 = state, model.lmf_state()
    for _ in range(2):  # the second call accumulates
        grad = model.softmax_gradient(d, case.hyper, side)
        assert model.softmax(d, case.hyper, side) == 0
        after, acc1 = model.download(), model.lmf_state()
        pairs = [(_own(before, side)[0], _own(acc0, side)[0], grad[0], _own(after, side)[0], _own(acc1, side)[0])]
        if side == "items":
            pairs.append((before[3], acc0[3], grad[1], after[3], acc1[3]))
        for x0, a0, g, x1, a1 in pairs:
            x64, a64 = ref.step(x0[:n], a0[:n], g, lr)
            assert (np.abs(x1[:n] - x64) <= 2.0 ** -22 * np.maximum(np.abs(x64), lr)).all()
            assert (np.abs(a1[:n] - a64) <= 2.0 ** -23 * a64).all()
            assert same_bits(x1[n:], x0[n:]) and same_bits(a1[n:], a0[n:])
        assert same_state(_own(after, other), _own(before, other)) and same_state(_own(acc1, other), _own(acc0, other))
        assert same_bits(after[2], state[2]) and not acc1[2].any()  # user biases never move
        before, acc0 = after, acc1
    assert (acc1[0 if side == "users" else 1][:n] > 0).any()
    model.lmf_reset()
    assert all(not a.any() for a in model.lmf_state())


def test_a_nan_in_one_users_factors_leaves_that_user_and_then_every_item_alone():
    case = chk.cases()["f100-65x1000"]
    P, Q, ub, ib = case.state()
    d = cu.DeviceCSR(case.csr)
    n = case.csr.rows
    rest = np.arange(n) != 37
    bad = P.copy()
    bad[37, 5] = np.nan
    clean, model = model_from((P, Q, ub, ib), case.gb), model_from((bad, Q, ub, ib), case.gb)
    lse = model.softmax_lse(d)
    assert np.isnan(lse[37]) and same_bits(lse[rest], clean.softmax_lse(d)[rest])
    assert clean.softmax(d, case.hyper, "users") == 0
    assert model.softmax(d, case.hyper, "users") == 1
    got, want = model.download(), clean.download()
    assert same_bits(got[0][37], bad[37]) and same_bits(got[0][:n][rest], want[0][:n][rest])
    acc, acc_clean = model.lmf_state(), clean.lmf_state()
    assert not acc[0][37].any() and same_bits(acc[0][:n][rest], acc_clean[0][:n][rest])
    # the item half-step: that user's coefficients are NaN for every item
    assert model.softmax(d, case.hyper, "items") == case.csr.cols
    assert same_state(model.download(), got) and same_state(model.lmf_state(), acc)
    assert clean.softmax(d, case.hyper, "items") == 0


def test_two_sweeps_twice_are_four_sweeps_once():
    case = chk.cases()["f31-33x129"]
    d = cu.DeviceCSR(case.csr)
    a, b = model_from(case.state(), case.gb), model_from(case.state(), case.gb)
    a.lmf_reset()
    assert a.softmax(d, case.hyper, "both", sweeps=2) == 0 and a.softmax(d, case.hyper, "both", sweeps=2) == 0
    b.lmf_reset()
    assert b.softmax(d, case.hyper, "both", sweeps=4) == 0
    assert same_state(a.download(), b.download()) and same_state(a.lmf_state(), b.lmf_state())
    assert not same_bits(a.download()[0], case.state()[0])


@pytest.mark.parametrize("name", chk.OBJECTIVE_SETS)
def test_objective_matches_float64(name):
    """Within svd_checks.MARGIN times what the float32 restatement is off by (softmax_checks.OBJECTIVE_RESTATEMENT_ERROR, measured by
    tests/test_softmax_cpu.py): the device's expf / logf are not numpy's."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, case.gb)
    got = model.softmax_objective(cu.DeviceCSR(case.csr), case.hyper)
    want = ref.objective(case.csr, state, case.gb, case.hyper)
    print("%s: objective %.12g, off by %.3g" % (name, got, abs(got - want) / abs(want)))
    assert abs(got - want) <= chk.MARGIN * chk.OBJECTIVE_RESTATEMENT_ERROR * abs(want), (got, want)
    assert same_state(model.download(), state)


def test_argument_checks_leave_everything_alone():
    case = chk.cases()["f8-33x129"]
    model = model_from(case.state(), case.gb)
    d = cu.DeviceCSR(case.csr)
    L = lib()
    assert model.softmax(d, case.hyper, "users") == 0
    before, acc = model.download(), model.lmf_state()
    lr, P_reg, Q_reg, ubr, ibr = case.hyper
    n = C.c_int(-7)

    def all_calls(hyper, side, want, m=model, dd=d):
        h = cu.Hyper(*[float(x) for x in hyper])
        out = C.c_double()
        assert L.cu2rec_model_softmax(m._h, dd._h, C.byref(h), side, C.byref(n)) == want
        assert L.cu2rec_model_softmax_gradient(m._h, dd._h, C.byref(h), side, None, None) == want
        if side in (0, 1):
            assert L.cu2rec_model_softmax_objective(m._h, dd._h, C.byref(h), C.byref(out)) == want
            cfg = api.default_config(total_iterations=1, n_factors=m.n_factors, learning_rate=hyper[0], P_reg=hyper[1], Q_reg=hyper[2],
                                     user_bias_reg=hyper[3], item_bias_reg=hyper[4])
            assert L.cu2rec_train_softmax(dd._h, C.byref(cfg), m._h, 0, None, None) == want

    all_calls(case.hyper, 2, EINVAL)
    all_calls(case.hyper, -1, EINVAL)
    for k in (1, 2, 4):  # P_reg, Q_reg, item_bias_reg
        for v in (-0.5, np.nan, np.inf):
            hyper = list(case.hyper)
            hyper[k] = v
            all_calls(hyper, 1, EINVAL)
    for v in (0.0, -0.1, np.nan, np.inf):
        all_calls((v, P_reg, Q_reg, ubr, ibr), 0, EINVAL)
    wide = cu.DeviceCSR(api.HostCSR(case.csr.indptr, case.csr.indices, case.csr.data, case.csr.rows, model.cols + 1, case.gb))
    all_calls(case.hyper, 0, EINVAL, dd=wide)
    out = np.zeros(case.csr.rows, np.float32)
    assert L.cu2rec_model_softmax_lse(model._h, wide._h, out.ctypes.data_as(C.c_void_p)) == EINVAL
    h = cu.Hyper(*case.hyper)
    assert L.cu2rec_model_softmax(None, d._h, C.byref(h), 0, None) == EINVAL
    assert L.cu2rec_model_softmax(model._h, None, C.byref(h), 0, None) == EINVAL
    assert L.cu2rec_model_softmax(model._h, d._h, None, 0, None) == EINVAL
    assert L.cu2rec_model_softmax_objective(model._h, d._h, C.byref(h), None) == EINVAL
    assert L.cu2rec_model_softmax_lse(model._h, d._h, None) == EINVAL
    assert n.value == -7
    assert same_state(model.download(), before) and same_state(model.lmf_state(), acc)
    big = cu.Model(4, 6, 253, 0.0)
    tiny = cu.DeviceCSR(api.HostCSR(np.array([0, 1, 1, 1, 1]), np.array([2], np.int32), np.array([1.0], np.float32), 4, 6, 0.0))
    all_calls(case.hyper, 0, EUNSUPPORTED, m=big, dd=tiny)
    assert L.cu2rec_model_softmax(model._h, d._h, C.byref(h), 1, None) == 0  # n_unchanged may be NULL
    with pytest.raises(ValueError):
        model.softmax(d, case.hyper, side="rows")


def test_no_items_and_no_entries_are_valid_problems():
    P, Q, ub, ib = chk.cases()["f8-33x129"].state()
    model = model_from((P, Q, ub, ib), 0.5)
    hyper = chk.HYPER
    no_entries = cu.DeviceCSR(api.HostCSR(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 9, 0.5))
    g, gb = model.softmax_gradient(no_entries, hyper, "users")
    assert same_bits(g, (-(np.float32(hyper[1]) * P[:5])).astype(np.float32)) and not gb.any()
    g, gb = model.softmax_gradient(no_entries, hyper, "items")
    assert same_bits(g, (-(np.float32(hyper[2]) * Q[:9])).astype(np.float32))
    assert same_bits(gb, (-(np.float32(hyper[4]) * ib[:9])).astype(np.float32))
    no_items = cu.DeviceCSR(api.HostCSR(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 0, 0.5))
    assert np.isneginf(model.softmax_lse(no_items)).all()
    assert model.softmax(no_items, hyper, "both") == 0
    assert model.softmax_gradient(no_items, hyper, "items")[0].shape == (0, 8)
    assert np.isfinite(model.softmax_objective(no_entries, hyper))


def test_the_other_trainers_are_unchanged_on_a_model_and_csr_softmax_has_used():
    """lmf, bpr and als on the objects softmax has used -- its views, the shared gradient workspace and partial sums, the reset
    accumulators -- against the same calls on a model created from the downloaded state and a CSR uploaded afresh: bit for bit."""
    case = chk.cases()["f31-33x129"]
    used, d_used = model_from(case.state(), case.gb), cu.DeviceCSR(case.csr)
    assert used.softmax(d_used, case.hyper, "both", sweeps=2) == 0
    used.softmax_objective(d_used, case.hyper)
    used.softmax_mass(d_used)
    used.lmf_reset()
    fresh, d_fresh = model_from(used.download(), case.gb), cu.DeviceCSR(case.csr)
    for step in (lambda m, d: m.lmf(d, case.hyper, 2.0, "both"), lambda m, d: m.lmf_objective(d, case.hyper, 2.0),
                 lambda m, d: m.bpr(d, case.hyper, 42, 0, "both"), lambda m, d: m.als(d, case.hyper, "both"),
                 lambda m, d: m.softmax(d, case.hyper, "both")):
        assert step(used, d_used) == step(fresh, d_fresh)
        assert same_state(used.download(), fresh.download()) and same_state(used.lmf_state(), fresh.lmf_state())


# ---------------------------------------------------------------------------------------------------- the ML_SMALL experiment

_RUN = {}


def _ml_small_run():
    """The Model.softmax loop on the experiment from the library's initial model, once: the objective after every half-step, the end."""
    if not _RUN:
        tr, _ = chk.ml_small()
        d = cu.DeviceCSR(tr)
        model = cu.Model(tr.rows, tr.cols, chk.ML_SMALL_F, tr.global_bias)
        assert same_state(model.download(), chk.ml_small_start())  # the reference starts where the device does
        objectives = []
        for _ in range(chk.ML_SMALL_SWEEPS):
            for side in ("users", "items"):
                assert model.softmax(d, chk.ML_SMALL_HYPER, side) == 0
                objectives.append(model.softmax_objective(d, chk.ML_SMALL_HYPER))
        _RUN.update(state=model.download(), objectives=objectives, tr=tr)
    return _RUN


def test_sweeps_on_ml_small_follow_the_float64_run():
    """softmax_checks.ML_SMALL_*: the objective after every half-step, the final factors and biases and the final scores within
    svd_checks.MARGIN x the float32 restatement's recorded distances of the FLOAT64 run's, and the held-out hits equal to float64's
    up to the recorded users within reach."""
    run = _ml_small_run()
    s64, o64 = chk.ml_small_run64()
    worst = max(abs(a - b) / abs(b) for a, b in zip(run["objectives"], o64))
    factors = max(np.abs(np.asarray(a, np.float64) - b).max() for a, b in zip(run["state"], s64))
    S64 = chk.scores_of(s64, run["tr"].global_bias)
    scores = np.abs(chk.scores_of(run["state"], run["tr"].global_bias) - S64).max() / np.abs(S64).max()
    hits = chk.hits_of(run["state"])
    print("objective distance %.3g (the restatement's: %.3g), factor distance %.3g (%.3g), score distance %.3g (%.3g), hits %d (%d)"
          % (worst, chk.ML_SMALL_OBJECTIVE_DISTANCE, factors, chk.ML_SMALL_FACTOR_DISTANCE, scores, chk.ML_SMALL_SCORE_DISTANCE, hits,
             chk.ML_SMALL_HITS))
    assert len(o64) == 2 * chk.ML_SMALL_SWEEPS and worst <= chk.MARGIN * chk.ML_SMALL_OBJECTIVE_DISTANCE
    assert factors <= chk.MARGIN * chk.ML_SMALL_FACTOR_DISTANCE
    assert scores <= chk.MARGIN * chk.ML_SMALL_SCORE_DISTANCE
    assert abs(hits - chk.ML_SMALL_HITS) <= chk.ML_SMALL_WITHIN_REACH
    assert same_bits(run["state"][2], chk.ml_small_start()[2])  # user biases keep their bits


def test_train_and_bin_mf_give_the_loops_factors(tmp_path, capfd):
    """train(mode="softmax") ends on the Model.softmax loop's state bit for bit, with the objective at the loss cadence;
    bin/mf -m softmax writes the five files the loop's state gives through the same writer, byte for byte, and -k's ranking line."""
    run = _ml_small_run()
    tr, f = run["tr"], chk.ML_SMALL_F
    lr, P_reg, Q_reg, ubr, ibr = chk.ML_SMALL_HYPER
    cfg = api.default_config(total_iterations=chk.ML_SMALL_SWEEPS, n_factors=f, check_error=4, learning_rate=lr, P_reg=P_reg, Q_reg=Q_reg,
                             user_bias_reg=ubr, item_bias_reg=ibr)
    capfd.readouterr()
    P, Q, objectives, ub, ib, stats = cu.train(tr, None, cfg, mode="softmax", verbose=True, return_stats=True)
    out = capfd.readouterr().out
    assert same_state((P, Q, ub, ib), run["state"])
    lines = [l for l in out.splitlines() if l.startswith("TRAIN:")]
    assert [l.split()[2] for l in lines] == ["1", "4", "6"] and all("GPU softmax objective" in l for l in lines), lines
    checked = [0, 3, 5]
    assert objectives.dtype == np.float64 and np.isnan(np.delete(objectives, checked)).all()
    assert [objectives[k] for k in checked] == [run["objectives"][2 * k + 1] for k in checked]
    assert cfg.learning_rate == np.float32(lr) and "New Learning Rate" not in out
    assert stats.updates == chk.ML_SMALL_SWEEPS * (tr.rows + tr.cols)

    mf = os.path.join(ROOT, "bin", "mf")
    csv = tmp_path / "ratings.csv"
    with open(ml_small(), "rb") as src:  # the whole file: its values are stars, not ones, so the loop is run again on them
        csv.write_bytes(src.read())
    full = cu.createSparseMatrix(str(csv))
    model = cu.Model(full.rows, full.cols, f, full.global_bias)
    assert model.softmax(cu.DeviceCSR(full), chk.ML_SMALL_HYPER, "both", sweeps=2) == 0
    (tmp_path / "c.cfg").write_text("0 2 %d %g 42 %g %g %g %g\n" % (f, lr, P_reg, Q_reg, ubr, ibr))
    res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "softmax", "-k", "10", str(csv), str(csv)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    assert "GPU softmax objective" in res.stdout and "Precision@10" in res.stdout and "TEST: Iteration" not in res.stdout
    want = tmp_path / "want"
    want.mkdir()
    shapes = ((full.rows, f), (full.cols, f), (full.rows, 1), (full.cols, 1))
    for name, data, (rows, cols) in zip(("p", "q", "user_bias", "item_bias"), model.download(), shapes):
        api.writeToFile(str(want), "ratings", name, data, rows, cols, f)
        assert (tmp_path / ("ratings_f%d_%s.csv" % (f, name))).read_bytes() == (want / ("ratings_f%d_%s.csv" % (f, name))).read_bytes(), name
    assert (tmp_path / ("ratings_f%d_global_bias.csv" % f)).exists()
    for flag in (["-a", "2"], ["-C", "3"], ["-g", "2"], ["-s", "4"], ["-w", "mean"], ["-W", "cosine"], ["-N", "5"], ["-L", "10"],
                 ["-l", "1"], ["-n", "3"]):
        res = subprocess.run([mf, "-m", "softmax"] + flag + [str(csv), str(csv)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "Free memory" not in res.stdout, (flag, res.stderr)
