"""Bayesian Personalized Ranking on the GPU (cu2rec_model_bpr, cu2rec_model_bpr_gradient, cu2rec_model_bpr_objective,
cu2rec_csr_bpr_negatives, cu2rec_train_bpr, bin/mf -m bpr) against the float64 reference of tests/bpr_reference64.py.

The negatives are compared as integers.  A gradient is judged entrywise by bpr_reference64.bound(): tests/test_bpr_cpu.py shows on
the CPU that a float32 restatement of the kernels' arithmetic stays below 0.25 of it on every set judged here and that ten
deliberate mistakes in the model exceed it thirtyfold."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib
from conftest import ROOT

import bpr_checks as chk
import bpr_reference64 as ref
from als_checks import model_from, same_bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6
SEED, SWEEP = chk.GRADIENT_SEED, chk.GRADIENT_SWEEP


def _same_state(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def _judge(case, state, got):
    neg = case.negatives()
    g, gb = ref.gradient(case.csr, state, case.hyper, neg, case.side)
    b, bb = ref.bound(case.csr, state, case.hyper, neg, case.side)
    assert got[0].shape == g.shape and got[1].shape == gb.shape
    return max(ref.ratio(got[0], g, b), ref.ratio(got[1], gb, bb))


@pytest.mark.parametrize("name", sorted(chk.negative_sets()))
def test_negatives_equal_the_cpu_draws(name):
    """Rows of 0, 1, 2, 3, 4, 5, 7, 40 and 300 unsorted entries with repeats, a row that stores every column, one that stores all but
    one, cols == 1 and cols past every stored item; two seeds and sweeps 0, 1 and 2^29 - 1: every negative equals the CPU's."""
    csr = chk.negative_sets()[name]
    d = cu.DeviceCSR(csr)
    for seed in chk.SEEDS:
        for sweep in chk.SWEEPS:
            got = d.bpr_negatives(seed, sweep)
            assert got.dtype == np.int32 and np.array_equal(got, ref.negatives(csr, seed, sweep)), (name, seed, sweep)
    assert np.array_equal(d.bpr_negatives(chk.SEEDS[0], 0), ref.negatives(csr, chk.SEEDS[0], 0))  # after other sweeps, the same again


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_gradient_matches_float64(name):
    """Every width of bpr_checks.WIDTHS on sets with every row length, entries without a triple, items that are only positives, only
    negatives, both and neither, non-zero item biases and model rows past the CSR, on both sides: every gradient value within the
    rounding bound, the users' bias gradient a zero.  The model and the accumulators keep their bits, and a second call returns the
    same bits."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, 0.25)
    d = cu.DeviceCSR(case.csr)
    got = model.bpr_gradient(d, case.hyper, SEED, SWEEP, case.side)
    r = _judge(case, state, got)
    print("%s: worst value at %.3g of the bound" % (name, r))
    assert r <= 1.0, (name, r)
    if case.side == "users":
        assert not got[1].any()
    assert _same_state(model.download(), state)
    assert all(not a.any() for a in model.lmf_state())
    again = model.bpr_gradient(d, case.hyper, SEED, SWEEP, case.side)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1])


@pytest.mark.parametrize("side", ["users", "items"])
def test_saturated_scores_give_a_finite_gradient_within_the_bound(side):
    """x_e of about +-200 in both signs: sigma never becomes inf / inf."""
    case = chk.saturated_case(side)
    state = case.state()
    got = model_from(state, 0.0).bpr_gradient(cu.DeviceCSR(case.csr), case.hyper, SEED, SWEEP, side)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    r = _judge(case, state, got)
    print("%s: worst value at %.3g of the bound" % (case.name, r))
    assert r <= 1.0


@pytest.mark.parametrize("name", ["f100-65x1000", "f3-33x40", "f191-17x257"])
def test_a_user_alone_has_the_gradient_and_negatives_it_has_among_the_others(name):
    """In a CSR of the same shape where every other row is empty."""
    case = chk.cases()[name]
    csr, state = case.csr, case.state()
    full = model_from(state, 0.0).bpr_gradient(cu.DeviceCSR(csr), case.hyper, SEED, SWEEP, "users")
    neg = cu.DeviceCSR(csr).bpr_negatives(SEED, SWEEP)
    for u in (0, 1, 9, csr.rows - 1):
        lo, hi = csr.indptr[u], csr.indptr[u + 1]
        indptr = np.concatenate([np.zeros(u + 1, np.int64), np.full(csr.rows - u, hi - lo)])
        alone = cu.DeviceCSR(api.HostCSR(indptr, csr.indices[lo:hi], csr.data[lo:hi], csr.rows, csr.cols, 0.0))
        assert np.array_equal(alone.bpr_negatives(SEED, SWEEP), neg[lo:hi]), u
        got = model_from(state, 0.0).bpr_gradient(alone, case.hyper, SEED, SWEEP, "users")
        assert same_bits(got[0][u], full[0][u]), u


def _own(state, side):
    P, Q, ub, ib = state
    return (P, ub) if side == "users" else (Q, ib)


def _check_step(before, acc_before, grad, after, acc_after, n, lr):
    """tests/test_gpu_lmf.py's: x' and a' of rows [0, n) against the float64 step from the device's own gradient and prior state,
    within four correctly rounded float32 operations; the rows past n keep their bits."""
    lr = float(np.float32(lr))
    for x0, a0, g, x1, a1 in ((before[0], acc_before[0], grad[0], after[0], acc_after[0]),
                              (before[1], acc_before[1], grad[1], after[1], acc_after[1])):
        x64, a64 = ref.step(x0[:n], a0[:n], g, lr)
        assert (np.abs(x1[:n] - x64) <= 2.0 ** -22 * np.maximum(np.abs(x64), lr)).all()
        assert (np.abs(a1[:n] - a64) <= 2.0 ** -23 * a64).all()
        assert same_bits(x1[n:], x0[n:]) and same_bits(a1[n:], a0[n:])


@pytest.mark.parametrize("name", ["f100-65x1000", "f63-33x40-items", "f252-33x40", "f4-17x257-items"])
def test_step_accumulates_and_keeps_every_other_bit(name):
    """Two half-steps of one side: the step against float64 from the device's own gradient; the other side, the model rows past the
    CSR, user_bias (a -0.0 among it) and its accumulator keep their bits."""
    case = chk.cases()[name]
    P, Q, ub, ib = case.state()
    ub[3] = -0.0
    state = (P, Q, ub, ib)
    model = model_from(state, 0.0)
    d = cu.DeviceCSR(case.csr)
    side, lr = case.side, case.hyper[0]
    n = case.csr.rows if side == "users" else case.csr.cols
    acc = lambda: _own(model.lmf_state(), side)
    zeros = acc()
    assert not zeros[0].any() and not zeros[1].any()
    before, acc_before = state, zeros
    for sweep in (SWEEP, SWEEP + 1):
        g = model.bpr_gradient(d, case.hyper, SEED, sweep, side)
        assert model.bpr(d, case.hyper, SEED, sweep, side, 1) == 0
        after, acc_after = model.download(), acc()
        _check_step(_own(before, side), acc_before, g, _own(after, side), acc_after, n, lr)
        other = "items" if side == "users" else "users"
        assert _same_state(_own(after, other), _own(state, other))
        assert all(not a.any() for a in _own(model.lmf_state(), other))
        assert same_bits(after[2], ub) and not model.lmf_state()[2].any()
        before, acc_before = after, acc_after
    assert (acc_after[0][:n] > 0).any()


def test_user_bias_and_its_accumulator_keep_their_bits_after_a_logistic_step():
    """The accumulators are shared with lmf(): after a logistic half-step has made a_ub non-zero, BPR's user half-step returns
    user_bias and a_ub bit for bit, moves P and adds to aP; lmf_reset zeroes what both have accumulated."""
    case = chk.cases()["f100-65x1000"]
    model = model_from(case.state(), 0.0)
    d = cu.DeviceCSR(case.csr)
    assert model.lmf(d, case.hyper, 1.0, "users") == 0
    s1, a1 = model.download(), model.lmf_state()
    assert a1[2][:case.csr.rows].all()
    assert model.bpr(d, case.hyper, SEED, SWEEP, "users") == 0
    s2, a2 = model.download(), model.lmf_state()
    assert same_bits(s2[2], s1[2]) and same_bits(a2[2], a1[2])
    assert not same_bits(s2[0], s1[0]) and (a2[0] >= a1[0]).all() and (a2[0] > a1[0]).any()
    assert _same_state((s2[1], s2[3], a2[1], a2[3]), (s1[1], s1[3], a1[1], a1[3]))
    model.lmf_reset()
    assert all(not a.any() for a in model.lmf_state())


def test_a_nan_own_row_and_an_inf_partner_row_are_left_unchanged_and_counted():
    case = chk.cases()["f100-65x1000"]
    P, Q, ub, ib = case.state()
    csr = case.csr
    d = cu.DeviceCSR(csr)
    n = csr.rows
    neg = case.negatives()
    rest = np.arange(n) != 36
    bad = P.copy()
    bad[36, 5] = np.nan  # row 36 has 300 entries (36 % 9 == 0)
    clean, model = model_from((P, Q, ub, ib), 0.0), model_from((bad, Q, ub, ib), 0.0)
    assert clean.bpr(d, case.hyper, SEED, SWEEP, "users") == 0
    assert model.bpr(d, case.hyper, SEED, SWEEP, "users") == 1
    got, want = model.download(), clean.download()
    assert same_bits(got[0][36], bad[36])
    assert same_bits(got[0][:n][rest], want[0][:n][rest])
    acc, acc_clean = model.lmf_state(), clean.lmf_state()
    assert not acc[0][36].any() and same_bits(acc[0][:n][rest], acc_clean[0][:n][rest])
    # one inf in an item row: exactly the users with a triple that names it, as positive or as negative, are counted and unchanged
    lo = csr.indptr[36]
    item = int(csr.indices[lo])
    Qinf = Q.copy()
    Qinf[item, 3] = np.inf
    rows = np.repeat(np.arange(n), np.diff(csr.indptr))
    hit = np.unique(rows[(neg >= 0) & ((csr.indices == item) | (neg == item))])
    assert 0 < len(hit) < n
    model = model_from((P, Qinf, ub, ib), 0.0)
    assert model.bpr(d, case.hyper, SEED, SWEEP, "users") == len(hit)
    got = model.download()
    assert same_bits(got[0][hit], P[hit]) and same_bits(np.delete(got[0][:n], hit, 0), np.delete(want[0][:n], hit, 0))
    # the item side: an inf user row leaves every item it touches unchanged
    Pinf = P.copy()
    Pinf[36, 0] = np.inf
    touched = np.unique(np.concatenate([csr.indices[rows == 36][neg[rows == 36] >= 0], neg[(rows == 36) & (neg >= 0)]]))
    model = model_from((Pinf, Q, ub, ib), 0.0)
    assert model.bpr(d, case.hyper, SEED, SWEEP, "items") == len(touched)
    got = model.download()
    assert same_bits(got[1][touched], Q[touched]) and same_bits(got[3][touched], ib[touched])
    assert not model.lmf_state()[1][touched].any()


@pytest.mark.parametrize("name", chk.OBJECTIVE_SETS)
def test_objective_and_counts_match_float64(name):
    """The counts exactly; L within four times bpr_checks.OBJECTIVE_RESTATEMENT_ERROR (the multiple of tests/test_gpu_lmf.py)."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, 0.0)
    L, n, m = model.bpr_objective(cu.DeviceCSR(case.csr), case.hyper, SEED, SWEEP)
    want, wn, wm = ref.objective(case.csr, state, case.hyper, case.negatives())
    print("%s: objective %.15g, off by %.3g" % (name, L, abs(L - want) / abs(want)))
    assert (n, m) == (wn, wm)
    assert abs(L - want) <= 4 * chk.OBJECTIVE_RESTATEMENT_ERROR * abs(want), (L, want)
    assert _same_state(model.download(), state)


def test_problems_without_triples():
    """cols == 1 (every draw is the stored item), nnz == 0 and cols == 0: valid, no triple, the gradient is -reg x."""
    hyper = chk.HYPER
    for csr in (chk.negative_sets()["5x1"], api.HostCSR(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 7, 0.0),
                api.HostCSR(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 0, 0.0)):
        rng = np.random.default_rng(1)
        state = (rng.normal(0, 1, (6, 5)).astype(np.float32), rng.normal(0, 1, (8, 5)).astype(np.float32),
                 rng.normal(0, 1, 6).astype(np.float32), rng.normal(0, 1, 8).astype(np.float32))
        model = model_from(state, 0.0)
        d = cu.DeviceCSR(csr)
        L, n, m = model.bpr_objective(d, hyper, SEED, 0)
        assert (n, m) == (0, 0) and abs(L - ref.objective(csr, state, hyper, ref.negatives(csr, SEED, 0))[0]) <= 1e-12 * abs(L)
        g, gb = model.bpr_gradient(d, hyper, SEED, 0, "users")
        assert same_bits(g, -(np.float32(hyper[1]) * state[0][:5])) and not gb.any()
        g, gb = model.bpr_gradient(d, hyper, SEED, 0, "items")
        assert same_bits(g, -(np.float32(hyper[2]) * state[1][:csr.cols])) and same_bits(gb, -(np.float32(hyper[4]) * state[3][:csr.cols]))
        assert model.bpr(d, hyper, SEED, 0, "both") == 0


def test_other_trainers_are_unchanged_by_the_cache_on_the_csr():
    """sgd, als, ials and lmf give the same bits on a CSR that the BPR calls have used (row-sorted view, negatives, regrouping, the
    kept sort values of the item-major view) as on a fresh one, in either order of first use."""
    case = chk.cases()["f62-65x1000"]
    state = case.state()
    hyper = (0.01, 0.6, 0.9, 0.25, 0.4)

    def results(d):
        out = []
        for call in (lambda m: m.sgd(d, hyper, 42, 0, 2, mode=api.SGD_ORDERED), lambda m: m.als(d, hyper, "both"),
                     lambda m: m.ials(d, hyper, 1.0, "both"), lambda m: m.lmf(d, hyper, 1.0, "both")):
            m = model_from(state, 0.0)
            call(m)
            out.extend(m.download())
            m.close()
        return out

    fresh = results(cu.DeviceCSR(case.csr))
    used = cu.DeviceCSR(case.csr)
    model_from(state, 0.0).bpr(used, hyper, SEED, 0, "both")  # builds the item-major view itself
    assert _same_state(results(used), fresh)
    after = cu.DeviceCSR(case.csr)
    results(after)  # the ALS calls build the view first
    a, b = model_from(state, 0.0), model_from(state, 0.0)
    a.bpr(after, hyper, SEED, 0, "both")
    b.bpr(used, hyper, SEED, 0, "both")
    assert _same_state(a.download(), b.download())


def test_argument_checks_leave_everything_alone():
    case = chk.cases()["f4-17x257"]
    state = case.state()
    model = model_from(state, 0.0)
    d = cu.DeviceCSR(case.csr)
    L = lib()
    assert model.bpr(d, case.hyper, SEED, 0, "users") == 0
    before, acc = model.download(), model.lmf_state()
    lr, P_reg, Q_reg, ubr, ibr = case.hyper
    n = C.c_int(-7)

    def all_calls(hyper, sweep, side, want, m=model, dd=d):
        h = cu.Hyper(*[float(x) for x in hyper])
        out = C.c_double()
        assert L.cu2rec_model_bpr(m._h, dd._h, C.byref(h), SEED, sweep, side, C.byref(n)) == want
        assert L.cu2rec_model_bpr_gradient(m._h, dd._h, C.byref(h), SEED, sweep, side, None, None) == want
        if side in (0, 1):
            assert L.cu2rec_model_bpr_objective(m._h, dd._h, C.byref(h), SEED, sweep, C.byref(out), None, None) == want
            cfg = api.default_config(total_iterations=1, n_factors=m.n_factors, learning_rate=hyper[0], P_reg=hyper[1], Q_reg=hyper[2],
                                     user_bias_reg=hyper[3], item_bias_reg=hyper[4])
            cfg.cur_iterations = max(sweep, 0)
            if sweep >= 0:
                assert L.cu2rec_train_bpr(dd._h, C.byref(cfg), m._h, 0, None, None) == want

    all_calls(case.hyper, 0, 2, EINVAL)
    all_calls(case.hyper, 0, -1, EINVAL)
    for sweep in (-1, 1 << 29, 2 ** 31 - 1):
        all_calls(case.hyper, sweep, 0, EINVAL)
        assert L.cu2rec_csr_bpr_negatives(d._h, SEED, sweep, np.zeros(case.csr.nnz, np.int32).ctypes.data_as(C.c_void_p)) == EINVAL
    for k in (1, 2, 3, 4):
        for v in (-0.5, np.nan, np.inf):
            hyper = list(case.hyper)
            hyper[k] = v
            all_calls(hyper, 0, 1, EINVAL)
    for v in (0.0, -0.1, np.nan, np.inf):
        all_calls((v, P_reg, Q_reg, ubr, ibr), 0, 0, EINVAL)
    wide = api.HostCSR(case.csr.indptr, case.csr.indices, case.csr.data, case.csr.rows, model.cols + 1, 0.0)
    all_calls(case.hyper, 0, 0, EINVAL, dd=cu.DeviceCSR(wide))
    h = cu.Hyper(*case.hyper)
    assert L.cu2rec_model_bpr(None, d._h, C.byref(h), SEED, 0, 0, None) == EINVAL
    assert L.cu2rec_model_bpr(model._h, None, C.byref(h), SEED, 0, 0, None) == EINVAL
    assert L.cu2rec_model_bpr(model._h, d._h, None, SEED, 0, 0, None) == EINVAL
    assert L.cu2rec_model_bpr_objective(model._h, d._h, C.byref(h), SEED, 0, None, None, None) == EINVAL
    assert L.cu2rec_csr_bpr_negatives(d._h, SEED, 0, None) == EINVAL
    assert n.value == -7
    assert _same_state(model.download(), before) and _same_state(model.lmf_state(), acc)
    big = cu.Model(4, 6, 253, 0.0)
    tiny = cu.DeviceCSR(api.HostCSR(np.array([0, 1, 1, 1, 1]), np.array([2], np.int32), np.array([1.0], np.float32), 4, 6, 0.0))
    all_calls(case.hyper, 0, 0, EUNSUPPORTED, m=big, dd=tiny)
    assert L.cu2rec_model_bpr(model._h, d._h, C.byref(h), SEED, (1 << 29) - 1, 1, None) == 0  # the last sweep; n_unchanged may be NULL
    with pytest.raises(ValueError):
        model.bpr(d, case.hyper, side="rows")


def test_of_two_failed_argument_checks_the_earlier_one_is_reported():
    """The BPR calls check side, the regularisers, the learning rate, the shape, the sweep and n_factors, in this order.  For every
    two neighbours a call that fails both: the earlier one's status and text under the entry point's own name (the texts as the
    library had them before the logistic calls shared the check), the model and the accumulators bit-unchanged.  A 3 x 4 CSR at
    f = 4; the shape fails on a model of two users, n_factors on one of 253 factors."""
    SIDE, REG, LR, SHAPE, SWEEP_TEXT = (": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS", ": every regulariser must be finite and >= 0",
                                        ": learning_rate must be finite and > 0", ": entries exceed the model's shape",
                                        ": sweep must be in [0, 2^29)")
    d = cu.DeviceCSR(api.HostCSR(np.array([0, 2, 2, 3]), np.array([0, 3, 1], np.int32), np.array([1.0, 2.0, 1.0], np.float32), 3, 4, 0.0))
    L = lib()
    good = (0.05, 0.1, 0.2, 0.3, 0.4)
    model, two_users, f253 = cu.Model(3, 4, 4, 0.0), cu.Model(2, 4, 4, 0.0), cu.Model(3, 4, 253, 0.0)
    assert model.bpr(d, good, SEED, 0, "both") == 0  # accumulators that are not zeros
    before = {m: (m.download(), m.lmf_state()) for m in (model, two_users, f253)}

    def refused(m, hyper, sweep, side, text):
        h, out = cu.Hyper(*hyper), C.c_double()
        cfg = api.default_config(total_iterations=1, n_factors=m.n_factors, learning_rate=hyper[0], P_reg=hyper[1], Q_reg=hyper[2],
                                 user_bias_reg=hyper[3], item_bias_reg=hyper[4])
        cfg.cur_iterations = sweep  # the one sweep's number
        calls = [("cu2rec_model_bpr", lambda: L.cu2rec_model_bpr(m._h, d._h, C.byref(h), SEED, sweep, side, None)),
                 ("cu2rec_model_bpr_gradient", lambda: L.cu2rec_model_bpr_gradient(m._h, d._h, C.byref(h), SEED, sweep, side, None, None))]
        if side in (0, 1):  # the calls without a side
            calls += [("cu2rec_model_bpr_objective",
                       lambda: L.cu2rec_model_bpr_objective(m._h, d._h, C.byref(h), SEED, sweep, C.byref(out), None, None)),
                      ("cu2rec_train_bpr", lambda: L.cu2rec_train_bpr(d._h, C.byref(cfg), m._h, 0, None, None))]
        for fn, call in calls:
            assert call() == EINVAL, fn
            assert L.cu2rec_last_error().decode() == fn + text
            assert _same_state(m.download(), before[m][0]) and _same_state(m.lmf_state(), before[m][1]), fn

    refused(model, (0.05, 0.1, -0.2, 0.3, 0.4), 0, 2, SIDE)             # side, regularisers
    refused(model, (0.0, 0.1, 0.2, np.nan, 0.4), 0, 0, REG)             # regularisers, learning rate
    refused(two_users, (-0.05, 0.1, 0.2, 0.3, 0.4), 0, 1, LR)           # learning rate, shape
    refused(two_users, good, 1 << 29, 0, SHAPE)                         # shape, sweep
    refused(f253, good, 1 << 29, 1, SWEEP_TEXT)                         # sweep, n_factors


# ---------------------------------------------------------------------------------------------------- sweeps on the fixture

_RUN = {}


def _fixture_run():
    """The Model.bpr loop on the fixture from the library's initial model, once: the objective after every half-step and the end."""
    if not _RUN:
        train, held, start = chk.fixture()
        d = cu.DeviceCSR(train)
        model = cu.Model(train.rows, train.cols, chk.FIXTURE_F, train.global_bias)
        assert _same_state(model.download(), start)  # the reference starts where the device does
        objectives = []
        for t in range(chk.FIXTURE_SWEEPS):
            for side in ("users", "items"):
                assert model.bpr(d, chk.FIXTURE_HYPER, chk.FIXTURE_SEED, t, side) == 0
                objectives.append(model.bpr_objective(d, chk.FIXTURE_HYPER, chk.FIXTURE_SEED, t))
        hit = model.rank_metrics(cu.DeviceCSR(held), 10, exclude=d)["hit_rate"]
        untrained = cu.Model(train.rows, train.cols, chk.FIXTURE_F, train.global_bias).rank_metrics(cu.DeviceCSR(held), 10, exclude=d)["hit_rate"]
        _RUN.update(state=model.download(), objectives=objectives, train=train, hit=hit, untrained=untrained,
                    no_triple=int((d.bpr_negatives(chk.FIXTURE_SEED, chk.FIXTURE_SWEEPS - 1) < 0).sum()))
    return _RUN


def test_sweeps_on_ml_small_follow_the_float64_run():
    """f = 32, the settings of bpr_checks, six sweeps with every user's last entry held out: the objective after every half-step
    within 8 x the float32 restatement's measured distance of the recorded FLOAT64 run's (the multiple of tests/test_gpu_lmf.py), the
    triples exactly its, the ordered triples and the held-out hits @10 within the margins measured on the CPU
    (bpr_checks.FIXTURE_REFERENCE: both are 0), the entries without a triple as many as the reference's."""
    run, R = _fixture_run(), chk.FIXTURE_REFERENCE
    got = run["objectives"]
    worst = max(abs(a[0] - b) / abs(b) for a, b in zip(got, R["objectives"]))
    print("objective distance %.3g (the restatement's: %.3g); ordered %s; hit rate %.6f (untrained %.6f)"
          % (worst, R["objective_distance"], [o[2] for o in got], run["hit"], run["untrained"]))
    assert len(got) == 2 * chk.FIXTURE_SWEEPS == len(R["objectives"])
    # the recorded objectives hold six decimals: 5e-7 absolute, far below the distance allowed
    assert worst <= 8 * R["objective_distance"] + 5e-7 / min(abs(b) for b in R["objectives"])
    assert [o[1] for o in got] == R["triples"]
    assert all(abs(o[2] - b) <= R["auc_flips"] for o, b in zip(got[-1:], R["ordered"][-1:]))
    assert abs(run["hit"] - R["hit_rate"]) * run["train"].rows <= R["hit_flips"] + 1e-9
    assert run["no_triple"] == run["train"].nnz - R["triples"][-1]
    assert run["hit"] > run["untrained"] and got[-1][2] / got[-1][1] > 0.85


def test_train_and_bin_mf_give_the_loops_factors(tmp_path, capfd):
    """train(mode="bpr") ends on the Model.bpr loop's state bit for bit, with the objective at the loss cadence; bin/mf -m bpr writes
    the five files the loop's state gives through the same writer, byte for byte (the files hold six digits)."""
    run = _fixture_run()
    train, f = run["train"], chk.FIXTURE_F
    lr, P_reg, Q_reg, ubr, ibr = chk.FIXTURE_HYPER
    cfg = api.default_config(total_iterations=chk.FIXTURE_SWEEPS, n_factors=f, check_error=4, learning_rate=lr, P_reg=P_reg, Q_reg=Q_reg,
                             user_bias_reg=ubr, item_bias_reg=ibr, seed=chk.FIXTURE_SEED)
    capfd.readouterr()
    P, Q, objectives, ub, ib, stats = cu.train(train, None, cfg, mode="bpr", verbose=True, return_stats=True)
    out = capfd.readouterr().out
    assert _same_state((P, Q, ub, ib), run["state"])
    lines = [l for l in out.splitlines() if l.startswith("TRAIN:")]
    assert [l.split()[2] for l in lines] == ["1", "4", "6"] and all("GPU BPR objective" in l for l in lines), lines
    checked = [0, 3, 5]
    assert objectives.dtype == np.float64 and np.isnan(np.delete(objectives, checked)).all()
    assert [objectives[k] for k in checked] == [run["objectives"][2 * k + 1][0] for k in checked]
    assert cfg.learning_rate == np.float32(lr) and "New Learning Rate" not in out
    assert stats.updates == chk.FIXTURE_SWEEPS * (train.rows + train.cols)

    # bin/mf reads a file: the training entries written out, read back (its shape is the file's), and the same loop run on that
    mf = os.path.join(ROOT, "bin", "mf")
    csv = tmp_path / "ratings.csv"
    rows = np.repeat(np.arange(train.rows), np.diff(train.indptr))
    with open(csv, "w") as fh:
        fh.write("userId,movieId,rating\n")
        for u, i, r in zip(rows.tolist(), train.indices.tolist(), train.data.tolist()):
            fh.write("%d,%d,%g\n" % (u + 1, i + 1, r))
    read = cu.createSparseMatrix(str(csv))
    assert read.rows == train.rows and np.array_equal(read.indices, train.indices)
    model = cu.Model(read.rows, read.cols, f, read.global_bias)
    assert model.bpr(cu.DeviceCSR(read), chk.FIXTURE_HYPER, chk.FIXTURE_SEED, 0, "both", chk.FIXTURE_SWEEPS) == 0
    state = model.download()
    (tmp_path / "c.cfg").write_text("0 %d %d %g %d %g %g %g %g\n" % (chk.FIXTURE_SWEEPS, f, lr, chk.FIXTURE_SEED, P_reg, Q_reg, ubr, ibr))
    res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "bpr", "-k", "10", str(csv), str(csv)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    assert "GPU BPR objective" in res.stdout and "Precision@10" in res.stdout and "TEST: Iteration" not in res.stdout
    want = tmp_path / "want"
    want.mkdir()
    shapes = ((read.rows, f), (read.cols, f), (read.rows, 1), (read.cols, 1))
    for name, data, (nr, nc) in zip(("p", "q", "user_bias", "item_bias"), state, shapes):
        api.writeToFile(str(want), "ratings", name, data, nr, nc, f)
        assert (tmp_path / ("ratings_f%d_%s.csv" % (f, name))).read_bytes() == (want / ("ratings_f%d_%s.csv" % (f, name))).read_bytes(), name
