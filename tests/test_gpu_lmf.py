"""Logistic matrix factorization on the GPU (cu2rec_model_lmf, cu2rec_model_lmf_gradient, cu2rec_model_lmf_objective,
cu2rec_train_lmf, bin/mf -m lmf) against the float64 reference of tests/lmf_reference64.py.

A gradient is judged entrywise by lmf_reference64.bound(): tests/test_lmf_cpu.py shows on the CPU that a float32 restatement of the
kernels' arithmetic stays below 0.18 of it on every set judged here and that eight deliberate mistakes in the model exceed it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib
from conftest import ROOT, ml_small

import lmf_checks as chk
import lmf_reference64 as ref
from als_checks import model_from, same_bits
from ials_checks import bar_ratio

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6


def _same_state(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def _judge(case, state, got):
    g, gb = ref.gradient(case.csr, state, case.gb, case.hyper, case.alpha, case.side)
    b, bb = ref.bound(case.csr, state, case.gb, case.hyper, case.alpha, case.side)
    assert got[0].shape == g.shape and got[1].shape == gb.shape
    return max(ref.ratio(got[0], g, b), ref.ratio(got[1], gb, bb))


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_gradient_matches_float64(name):
    """Every width of lmf_checks.WIDTHS, own-row count of OWN_ROWS and partner count of PARTNERS, rows of 0, 1, 2 and 300 unsorted
    entries with repeated pairs, cols past every stored item, non-zero biases and global bias, on both sides: every gradient value
    within the rounding bound.  The model and the accumulators keep their bits, and a second call returns the same bits."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, case.gb)
    d = cu.DeviceCSR(case.csr)
    got = model.lmf_gradient(d, case.hyper, case.alpha, case.side)
    r = _judge(case, state, got)
    print("%s: worst value at %.3g of the bound" % (name, r))
    assert r <= 1.0, (name, r)
    assert _same_state(model.download(), state)
    assert all(not a.any() for a in model.lmf_state())
    again = model.lmf_gradient(d, case.hyper, case.alpha, case.side)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1])


@pytest.mark.parametrize("name", ["f100-65x1000", "f8-33x129", "f252-65x31", "f32-65x1000"])
def test_item_half_step_is_the_user_half_step_of_the_transposed_problem(name):
    case = chk.cases()[name]
    P, Q, ub, ib = case.state()
    lr, P_reg, Q_reg, ubr, ibr = case.hyper
    items = model_from((P, Q, ub, ib), case.gb).lmf_gradient(cu.DeviceCSR(case.csr), case.hyper, case.alpha, "items")
    users = model_from((Q, P, ib, ub), case.gb).lmf_gradient(cu.DeviceCSR(case.csr.transpose()), (lr, Q_reg, P_reg, ibr, ubr),
                                                              case.alpha, "users")
    assert same_bits(items[0], users[0]) and same_bits(items[1], users[1])


@pytest.mark.parametrize("name", ["f100-65x1000", "f31-33x129", "f224-33x1000"])
def test_a_row_alone_has_the_gradient_it_has_among_the_others(name):
    case = chk.cases()[name]
    P, Q, ub, ib = case.state()
    full = model_from((P, Q, ub, ib), case.gb).lmf_gradient(cu.DeviceCSR(case.csr), case.hyper, case.alpha, "users")
    for u in (0, 1, case.csr.rows - 1):
        one = case.csr.slice_users(u, u + 1)
        got = model_from((P[u:u + 1], Q, ub[u:u + 1], ib), case.gb).lmf_gradient(cu.DeviceCSR(one), case.hyper, case.alpha, "users")
        assert same_bits(got[0][0], full[0][u]) and same_bits(got[1][:1], full[1][u:u + 1]), u


@pytest.mark.parametrize("side", ["users", "items"])
def test_saturated_scores_give_a_finite_gradient_within_the_bound(side):
    """Scores of about +-200 in both signs: sigma never becomes inf / inf."""
    case = chk.saturated_case(side)
    state = case.state()
    got = model_from(state, case.gb).lmf_gradient(cu.DeviceCSR(case.csr), case.hyper, case.alpha, side)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    r = _judge(case, state, got)
    print("%s: worst value at %.3g of the bound" % (case.name, r))
    assert r <= 1.0


def _own(state, side):
    P, Q, ub, ib = state
    return (P, ub) if side == "users" else (Q, ib)


def _check_step(before, acc_before, grad, after, acc_after, n, lr):
    """x' and a' of rows [0, n) against the float64 step from the device's own gradient and prior state: four correctly rounded
    float32 operations (tests/test_lmf_cpu.py: test_step_restatement_against_float64); the rows past n keep their bits."""
    lr = float(np.float32(lr))  # the learning rate the device holds
    for x0, a0, g, x1, a1 in ((before[0], acc_before[0], grad[0], after[0], acc_after[0]),
                              (before[1], acc_before[1], grad[1], after[1], acc_after[1])):
        x64, a64 = ref.step(x0[:n], a0[:n], g, lr)
        assert (np.abs(x1[:n] - x64) <= 2.0 ** -22 * np.maximum(np.abs(x64), lr)).all()
        assert (np.abs(a1[:n] - a64) <= 2.0 ** -23 * a64).all()
        assert same_bits(x1[n:], x0[n:]) and same_bits(a1[n:], a0[n:])


@pytest.mark.parametrize("name", ["f100-65x1000", "f63-1x31-items", "f252-65x31-items", "f8-33x1"])
def test_step_accumulates_resets_and_is_left_alone_by_the_other_trainers(name):
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, case.gb)
    d = cu.DeviceCSR(case.csr)
    side, lr = case.side, case.hyper[0]
    n = case.csr.rows if side == "users" else case.csr.cols
    acc = lambda: _own(model.lmf_state(), side)
    zeros = acc()
    assert not zeros[0].any() and not zeros[1].any()
    g1 = model.lmf_gradient(d, case.hyper, case.alpha, side)
    assert model.lmf(d, case.hyper, case.alpha, side) == 0
    s1, a1 = model.download(), acc()
    _check_step(_own(state, side), zeros, g1, _own(s1, side), a1, n, lr)
    other = "items" if side == "users" else "users"
    assert _same_state(_own(s1, other), _own(state, other))
    assert all(not a.any() for a in _own(model.lmf_state(), other))
    # a second call accumulates
    g2 = model.lmf_gradient(d, case.hyper, case.alpha, side)
    assert model.lmf(d, case.hyper, case.alpha, side) == 0
    s2, a2 = model.download(), acc()
    _check_step(_own(s1, side), a1, g2, _own(s2, side), a2, n, lr)
    assert (a2[0][:n] >= a1[0][:n]).all() and (a2[0][:n] > a1[0][:n]).any()
    # the other trainers leave the accumulators' bits alone
    kept = model.lmf_state()
    model.sgd(d, case.hyper, 42, 0, 2, mode=api.SGD_ORDERED)
    model.als(d, case.hyper, "both")
    model.ials(d, case.hyper, 1.0, "both")
    assert _same_state(model.lmf_state(), kept)
    model.lmf_reset()
    assert all(not a.any() for a in model.lmf_state())


def test_a_nan_in_an_own_row_leaves_that_row_alone_and_an_inf_in_a_partner_every_row():
    case = chk.cases()["f100-65x1000"]
    P, Q, ub, ib = case.state()
    d = cu.DeviceCSR(case.csr)
    n = case.csr.rows
    rest = np.arange(n) != 37
    bad = P.copy()
    bad[37, 5] = np.nan
    clean, model = model_from((P, Q, ub, ib), case.gb), model_from((bad, Q, ub, ib), case.gb)
    assert clean.lmf(d, case.hyper, case.alpha, "users") == 0
    assert model.lmf(d, case.hyper, case.alpha, "users") == 1
    got, want = model.download(), clean.download()
    assert same_bits(got[0][37], bad[37]) and same_bits(got[2][37:38], ub[37:38])
    assert same_bits(got[0][:n][rest], want[0][:n][rest]) and same_bits(got[2][:n][rest], want[2][:n][rest])
    acc, acc_clean = model.lmf_state(), clean.lmf_state()
    assert not acc[0][37].any() and acc[2][37] == 0
    assert same_bits(acc[0][:n][rest], acc_clean[0][:n][rest]) and same_bits(acc[2][:n][rest], acc_clean[2][:n][rest])
    # accumulators that are not zero are kept too: g = -reg x = 1.5e19 squares to 2.25e38, and twice that is not a float
    big = P.copy()
    big[37, 5] = -2.5e19
    model = model_from((big, Q, ub, ib), case.gb)
    assert model.lmf(d, case.hyper, case.alpha, "users") == 0
    s1, a1 = model.download(), model.lmf_state()
    assert a1[0][37, 5] > 2e38 and a1[0][37].all()
    assert model.lmf(d, case.hyper, case.alpha, "users") == 1
    s2, a2 = model.download(), model.lmf_state()
    assert same_bits(s2[0][37], s1[0][37]) and same_bits(s2[2][37:38], s1[2][37:38])
    assert same_bits(a2[0][37], a1[0][37]) and same_bits(a2[2][37:38], a1[2][37:38])
    assert not same_bits(s2[0][36], s1[0][36]) and not same_bits(a2[0][36], a1[0][36])
    # one inf in a partner row: every own row is counted and unchanged
    Qinf = Q.copy()
    Qinf[900, 3] = np.inf
    model = model_from((P, Qinf, ub, ib), case.gb)
    assert model.lmf(d, case.hyper, case.alpha, "users") == n
    assert _same_state(model.download(), (P, Qinf, ub, ib))
    assert all(not a.any() for a in model.lmf_state())


@pytest.mark.parametrize("name", chk.OBJECTIVE_SETS)
def test_objective_matches_float64(name):
    """Within four times what the float32 restatement is off by (lmf_checks.OBJECTIVE_RESTATEMENT_ERROR, measured by
    tests/test_lmf_cpu.py): the device's accumulation order is not the restatement's."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, case.gb)
    got = model.lmf_objective(cu.DeviceCSR(case.csr), case.hyper, case.alpha)
    want = ref.objective(case.csr, state, case.gb, case.hyper, case.alpha)
    print("%s: objective %.12g, off by %.3g" % (name, got, abs(got - want) / abs(want)))
    assert abs(got - want) <= 4 * chk.OBJECTIVE_RESTATEMENT_ERROR * abs(want), (got, want)
    assert _same_state(model.download(), state)


def test_argument_checks_leave_everything_alone():
    case = chk.cases()["f8-33x129"]
    state = case.state()
    model = model_from(state, case.gb)
    d = cu.DeviceCSR(case.csr)
    L = lib()
    assert model.lmf(d, case.hyper, case.alpha, "users") == 0
    before, acc = model.download(), model.lmf_state()
    lr, P_reg, Q_reg, ubr, ibr = case.hyper
    n = C.c_int(-7)

    def all_calls(hyper, alpha, side, want, m=model, dd=d):
        h = cu.Hyper(*[float(x) for x in hyper])
        out = C.c_double()
        assert L.cu2rec_model_lmf(m._h, dd._h, C.byref(h), alpha, side, C.byref(n)) == want
        assert L.cu2rec_model_lmf_gradient(m._h, dd._h, C.byref(h), alpha, side, None, None) == want
        if side in (0, 1):
            assert L.cu2rec_model_lmf_objective(m._h, dd._h, C.byref(h), alpha, C.byref(out)) == want
            cfg = api.default_config(total_iterations=1, n_factors=m.n_factors, learning_rate=hyper[0], P_reg=hyper[1], Q_reg=hyper[2],
                                     user_bias_reg=hyper[3], item_bias_reg=hyper[4])
            assert L.cu2rec_train_lmf(dd._h, C.byref(cfg), m._h, alpha, 0, None, None) == want

    all_calls(case.hyper, 1.0, 2, EINVAL)
    all_calls(case.hyper, 1.0, -1, EINVAL)
    for alpha in (-1.0, np.nan, np.inf):
        all_calls(case.hyper, alpha, 0, EINVAL)
    for k in (1, 2, 3, 4):
        for v in (-0.5, np.nan, np.inf):
            hyper = list(case.hyper)
            hyper[k] = v
            all_calls(hyper, 1.0, 1, EINVAL)
    for v in (0.0, -0.1, np.nan, np.inf):
        all_calls((v, P_reg, Q_reg, ubr, ibr), 1.0, 0, EINVAL)
    wide = api.HostCSR(case.csr.indptr, case.csr.indices, case.csr.data, case.csr.rows, model.cols + 1, case.gb)
    all_calls(case.hyper, 1.0, 0, EINVAL, dd=cu.DeviceCSR(wide))
    h = cu.Hyper(*case.hyper)
    assert L.cu2rec_model_lmf(None, d._h, C.byref(h), 1.0, 0, None) == EINVAL
    assert L.cu2rec_model_lmf(model._h, None, C.byref(h), 1.0, 0, None) == EINVAL
    assert L.cu2rec_model_lmf(model._h, d._h, None, 1.0, 0, None) == EINVAL
    assert L.cu2rec_model_lmf_objective(model._h, d._h, C.byref(h), 1.0, None) == EINVAL
    assert n.value == -7
    assert _same_state(model.download(), before) and _same_state(model.lmf_state(), acc)
    big = cu.Model(4, 6, 253, 0.0)
    tiny = cu.DeviceCSR(api.HostCSR(np.array([0, 1, 1, 1, 1]), np.array([2], np.int32), np.array([1.0], np.float32), 4, 6, 0.0))
    all_calls(case.hyper, 1.0, 0, EUNSUPPORTED, m=big, dd=tiny)
    assert L.cu2rec_model_lmf(model._h, d._h, C.byref(h), 1.0, 1, None) == 0  # n_unchanged may be NULL
    with pytest.raises(ValueError):
        model.lmf(d, case.hyper, side="rows")


def test_of_two_failed_argument_checks_the_earlier_one_is_reported():
    """The logistic calls check side, the regularisers, alpha, the learning rate, the shape and n_factors, in this order.  For every
    two neighbours a call that fails both: the earlier one's status and text under the entry point's own name (the texts as the
    library had them before the BPR calls shared the check), the model and the accumulators bit-unchanged.  A 3 x 4 CSR at f = 4;
    the shape fails on a model of two users, n_factors on one of 253 factors."""
    SIDE, REG, ALPHA, LR, SHAPE = (": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS", ": every regulariser must be finite and >= 0",
                                   ": alpha must be finite and >= 0", ": learning_rate must be finite and > 0",
                                   ": entries exceed the model's shape")
    d = cu.DeviceCSR(api.HostCSR(np.array([0, 2, 2, 3]), np.array([0, 3, 1], np.int32), np.array([1.0, 2.0, 1.0], np.float32), 3, 4, 0.0))
    L = lib()
    good = (0.05, 0.1, 0.2, 0.3, 0.4)
    model, two_users, two_users_253 = cu.Model(3, 4, 4, 0.0), cu.Model(2, 4, 4, 0.0), cu.Model(2, 4, 253, 0.0)
    assert model.lmf(d, good, 1.0, "both") == 0  # accumulators that are not zeros
    before = {m: (m.download(), m.lmf_state()) for m in (model, two_users, two_users_253)}

    def refused(m, hyper, alpha, side, text):
        h, out = cu.Hyper(*hyper), C.c_double()
        cfg = api.default_config(total_iterations=1, n_factors=m.n_factors, learning_rate=hyper[0], P_reg=hyper[1], Q_reg=hyper[2],
                                 user_bias_reg=hyper[3], item_bias_reg=hyper[4])
        calls = [("cu2rec_model_lmf", lambda: L.cu2rec_model_lmf(m._h, d._h, C.byref(h), alpha, side, None)),
                 ("cu2rec_model_lmf_gradient", lambda: L.cu2rec_model_lmf_gradient(m._h, d._h, C.byref(h), alpha, side, None, None))]
        if side in (0, 1):  # the calls without a side
            calls += [("cu2rec_model_lmf_objective", lambda: L.cu2rec_model_lmf_objective(m._h, d._h, C.byref(h), alpha, C.byref(out))),
                      ("cu2rec_train_lmf", lambda: L.cu2rec_train_lmf(d._h, C.byref(cfg), m._h, alpha, 0, None, None))]
        for fn, call in calls:
            assert call() == EINVAL, fn
            assert L.cu2rec_last_error().decode() == fn + text
            assert _same_state(m.download(), before[m][0]) and _same_state(m.lmf_state(), before[m][1]), fn

    refused(model, (0.05, 0.1, -0.2, 0.3, 0.4), 1.0, 2, SIDE)       # side, regularisers
    refused(model, (0.05, 0.1, 0.2, np.nan, 0.4), -1.0, 0, REG)     # regularisers, alpha
    refused(model, (0.0, 0.1, 0.2, 0.3, 0.4), np.inf, 1, ALPHA)     # alpha, learning rate
    refused(two_users, (-0.05, 0.1, 0.2, 0.3, 0.4), 1.0, 0, LR)     # learning rate, shape
    refused(two_users_253, good, 1.0, 1, SHAPE)                     # shape, n_factors


# ---------------------------------------------------------------------------------------------------- sweeps on the fixture

_RUN = {}


def _fixture_run():
    """The Model.lmf loop on the fixture from the library's initial model, once: the objective after every half-step and the end."""
    if not _RUN:
        tr, start = chk.fixture()
        d = cu.DeviceCSR(tr)
        model = cu.Model(tr.rows, tr.cols, chk.FIXTURE_F, tr.global_bias)
        assert _same_state(model.download(), start)  # the reference starts where the device does
        objectives = []
        for _ in range(chk.FIXTURE_SWEEPS):
            for side in ("users", "items"):
                assert model.lmf(d, chk.FIXTURE_HYPER, chk.FIXTURE_ALPHA, side) == 0
                objectives.append(model.lmf_objective(d, chk.FIXTURE_HYPER, chk.FIXTURE_ALPHA))
        _RUN.update(state=model.download(), objectives=objectives, tr=tr)
    return _RUN


def test_sweeps_on_ml_small_follow_the_float64_run():
    """f = 32, alpha = 2, lr = 0.2, P_reg = Q_reg = 0.6, 8 sweeps: the objective after every half-step within 8 x the float32
    restatement's distance (lmf_checks.FIXTURE_OBJECTIVE_DISTANCE, measured on the CPU) of the FLOAT64 run's, and the factors and
    biases within the project's forward bar of the float64 run's."""
    run = _fixture_run()
    s64, o64 = chk.fixture_run64()
    worst = max(abs(a - b) / abs(b) for a, b in zip(run["objectives"], o64))
    print("objective distance %.3g (the restatement's: %.3g)" % (worst, chk.FIXTURE_OBJECTIVE_DISTANCE))
    assert len(o64) == 2 * chk.FIXTURE_SWEEPS and worst <= 8 * chk.FIXTURE_OBJECTIVE_DISTANCE
    bars = [bar_ratio(np.reshape(x, (len(x), -1)), np.reshape(y, (len(y), -1))) for x, y in zip(run["state"], s64)]
    print("forward bar ratios: %s" % bars)
    assert max(bars) <= 1.0


def test_train_and_bin_mf_give_the_loops_factors(tmp_path, capfd):
    """train(mode="lmf") ends on the Model.lmf loop's state bit for bit, with the objective at the loss cadence; bin/mf -m lmf
    writes the five files the loop's state gives through the same writer, byte for byte (the files hold six digits)."""
    run = _fixture_run()
    tr, f = run["tr"], chk.FIXTURE_F
    lr, P_reg, Q_reg, ubr, ibr = chk.FIXTURE_HYPER
    cfg = api.default_config(total_iterations=chk.FIXTURE_SWEEPS, n_factors=f, check_error=3, learning_rate=lr, P_reg=P_reg, Q_reg=Q_reg,
                             user_bias_reg=ubr, item_bias_reg=ibr)
    capfd.readouterr()
    P, Q, objectives, ub, ib, stats = cu.train(tr, None, cfg, mode="lmf", alpha=chk.FIXTURE_ALPHA, verbose=True, return_stats=True)
    out = capfd.readouterr().out
    assert _same_state((P, Q, ub, ib), run["state"])
    lines = [l for l in out.splitlines() if l.startswith("TRAIN:")]
    assert [l.split()[2] for l in lines] == ["1", "3", "6", "8"] and all("GPU logistic objective" in l for l in lines), lines
    checked = [0, 2, 5, 7]
    assert objectives.dtype == np.float64 and np.isnan(np.delete(objectives, checked)).all()
    assert [objectives[k] for k in checked] == [run["objectives"][2 * k + 1] for k in checked]
    assert cfg.learning_rate == np.float32(lr) and "New Learning Rate" not in out
    assert stats.updates == chk.FIXTURE_SWEEPS * (tr.rows + tr.cols)

    mf = os.path.join(ROOT, "bin", "mf")
    csv = tmp_path / "ratings.csv"
    with open(ml_small(), "rb") as src:
        csv.write_bytes(src.read())
    (tmp_path / "c.cfg").write_text("0 %d %d %g 42 %g %g %g %g\n" % (chk.FIXTURE_SWEEPS, f, lr, P_reg, Q_reg, ubr, ibr))
    res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "lmf", "-a", "%g" % chk.FIXTURE_ALPHA, "-k", "10", str(csv), str(csv)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    assert "GPU logistic objective" in res.stdout and "Precision@10" in res.stdout and "TEST: Iteration" not in res.stdout
    want = tmp_path / "want"
    want.mkdir()
    shapes = ((tr.rows, f), (tr.cols, f), (tr.rows, 1), (tr.cols, 1))
    for name, data, (rows, cols) in zip(("p", "q", "user_bias", "item_bias"), run["state"], shapes):
        api.writeToFile(str(want), "ratings", name, data, rows, cols, f)
        assert (tmp_path / ("ratings_f%d_%s.csv" % (f, name))).read_bytes() == (want / ("ratings_f%d_%s.csv" % (f, name))).read_bytes(), name


def test_training_beats_the_untrained_model_at_hit_rate_at_10():
    """Every user's last entry held out: a sanity condition, not a quality claim."""
    tr, _ = chk.fixture()
    last = tr.indptr[1:] - 1
    keep = np.ones(tr.nnz, bool)
    keep[last] = False
    counts = np.diff(tr.indptr) - 1
    indptr = np.concatenate([[0], np.cumsum(counts)])
    train = api.HostCSR(indptr, tr.indices[keep], tr.data[keep], tr.rows, tr.cols, tr.global_bias)
    held = api.HostCSR(np.arange(tr.rows + 1), tr.indices[last], tr.data[last], tr.rows, tr.cols, tr.global_bias)
    d_train, d_held = cu.DeviceCSR(train), cu.DeviceCSR(held)
    model = cu.Model(tr.rows, tr.cols, chk.FIXTURE_F, tr.global_bias)
    untrained = model.rank_metrics(d_held, 10, exclude=d_train)["hit_rate"]
    assert model.lmf(d_train, chk.FIXTURE_HYPER, chk.FIXTURE_ALPHA, "both", sweeps=chk.FIXTURE_SWEEPS) == 0
    trained = model.rank_metrics(d_held, 10, exclude=d_train)["hit_rate"]
    print("hit rate @10: untrained %.4f, trained %.4f" % (untrained, trained))
    assert trained > untrained
