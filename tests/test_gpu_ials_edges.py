"""Implicit-feedback alternating least squares on the GPU at its edges: rows that cannot be solved (the counted-and-unchanged
path), G0 over two workspace batches, the objective kernel's grid-stride loops, the explicit half-step, the implicit half-step,
the objective and the SGD modes interleaved on shared objects, the item side's partner range and the device transposition.

Every tile count NT = ials_tiles(f) = 1 .. 8 at both of its edges (f = 32 NT - 1 and 32 NT) runs through
tests/test_gpu_ials.py::test_half_step_matches_float64 and ::test_objective_matches_float64, which take their sets from
tests/ials_checks.cases() and OBJECTIVE_SETS.  What they print on an MI355X is recorded below.

Every judgement is against the float64 reference (tests/ials_reference64.py) built from the same float32 state;
tests/test_ials_cpu.py shows on the CPU that the float32 restatement of the kernels' arithmetic meets the bar on every set used
here, fails exactly the rows expected to be counted here, and that five deliberate mistakes miss the bar.

Recorded, not asserted -- the worst row of test_half_step_matches_float64 in units of the bar (users / items) on an MI355X:
    NT = 1   f = 31: 3.1e-4 / 2.6e-4      NT = 2   f = 32: 2.7e-4 / 2.4e-4    f = 63: 6.5e-4 / 7.3e-4
    NT = 3   f = 64: 1.9e-4 / 2.2e-4    f = 95: 2.5e-4 / 3.2e-4 (with the row of 64 x 1,024 + 1 entries)
    NT = 4   f = 96: 2.6e-4 / 1.7e-4    f = 127: 8.8e-4 / 1.15e-3
    NT = 5   f = 128: 2.5e-4 / 4.8e-4   f = 159: 1.08e-3 / 1.05e-3
    NT = 6   f = 160: 3.9e-4 / 2.5e-4   f = 191: 1.04e-3 / 1.01e-3
    NT = 7   f = 192: 3.1e-4 / 2.6e-4   f = 223: 1.53e-3 / 1.26e-3
    NT = 8   f = 224: 3.9e-4 / 3.0e-4   f = 252: 3.6e-4 / 3.8e-4
and the objective's relative error against float64 at f = 32, 63, 96, 160, 191, 224: 3.98e-8, 3.6e-9, 2.25e-8, 6.5e-9, 1.11e-8,
4.68e-8 (tolerance 1.88e-7); on the two loop sets of this file 3.1e-11 and 2.1e-9.  In the tests of this file the worst solved
row is at 0.157 of the bar (poison-entry and negative at f = 100, users: 60 partners, fewer than factors).  No test here or
there found the kernels or the host code wrong.
"""
import os
import subprocess
import time

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from conftest import ROOT

import als_checks
import als_reference64
import ials_checks as chk
import ials_reference64 as ref
from als_checks import interplay, model_from, random_state, same_bits, same_state
from ials_checks import HYPER, check_half_step, ials

pytestmark = pytest.mark.gpu

SGD_HYPER = (0.01, 0.05, 0.04, 0.02, 0.03)


def _moved(a, b):
    """Per row: do the two float32 matrices differ in any bit?"""
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1)


# ---- B: rows that cannot be solved ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("f", chk.UNSOLVED_WIDTHS)
def test_a_poisoned_partner_nobody_names_fails_every_row(f, side):
    """A NaN, then a +inf, in one factor of a partner row inside the CSR that no entry names: it enters G0, so every row with
    entries is counted and keeps its bits, and every row without entries is still written as zeros.  The same value in a model
    row past the CSR's range is not read: the result is the clean run's bit for bit."""
    case = chk.Case("poison-unnamed", chk.messy_set(), side, f, 40.0, HYPER, 6500 + f)
    csr, state = case.csr, case.state()
    d = cu.DeviceCSR(csr)
    clean = check_half_step(model_from(state, 0.0), d, csr, side, HYPER, case.alpha)
    rated = case.judged()
    partner, own = (1, 0) if side == "users" else (0, 1)
    for bad in (np.nan, np.inf):
        for where in ("inside", "outside"):
            poisoned = [a.copy() for a in state]
            poisoned[partner][chk.poisoned_partner(case, where)] = bad
            model = model_from(poisoned, 0.0)
            if where == "inside":
                report = {}
                check_half_step(model, d, csr, side, HYPER, case.alpha, report=report, may_fail=rated)
                assert report["unsolved"] == len(rated) > 0 and np.array_equal(report["kept"], rated), (bad, report["unsolved"])
            else:
                assert ials(model, d, HYPER, case.alpha, side) == (0, 0)
                got = model.download()
                assert same_bits(got[own], clean[own]) and same_bits(got[own + 2], clean[own + 2]), (bad, where)
                assert same_bits(got[partner], poisoned[partner]) and same_bits(got[partner + 2], poisoned[partner + 2])


@pytest.mark.parametrize("name", sorted(chk.unsolved_cases()))
def test_rows_that_cannot_be_solved_are_counted_and_kept(name):
    """poison-entry: one entry value NaN and one +inf (alpha 40).  overflow: finite values and the finite alpha 3e38, whose
    product with the one entry of 2.0 is +inf in float32; every other value is 0, so every other weight is exactly 0 and those
    rows are solved and held to the bar like any other (the sub-case is precise: no row has a huge finite weight).  negative:
    mildly negative entries (w = -0.08) on rows whose system stays above reg I -- solved and judged -- and three entries of
    w = -4,000, whose rows' float64 systems have an eigenvalue below -10 reg.  In each, exactly the rows that hold such an entry
    are counted and keep their bits; every other row with entries meets the bar; rows without entries are zero."""
    case, fail = chk.unsolved_cases()[name]
    model = model_from(case.state(), 0.0)
    report = {}
    check_half_step(model, cu.DeviceCSR(case.csr), case.csr, case.side, case.hyper, case.alpha, report=report, may_fail=fail)
    print("%s: %d rows counted, worst solved row at %.3g of the bar" % (name, report["unsolved"], report[(case.side, case.f)]))
    assert report["unsolved"] == len(fail) >= 1 and np.array_equal(report["kept"], np.sort(fail)), (report["kept"], fail)


def test_train_implicit_counts_only_the_rows_it_solved():
    """cu2rec_train_implicit on the poison-entry data: stats.updates = sweeps x (rows with entries - counted rows) per side."""
    csr, entries = chk.poison_entry_set()
    cfg = api.default_config(total_iterations=3, n_factors=8, check_error=10, P_reg=HYPER[1], Q_reg=HYPER[2])
    P, Q, _, _, _, stats = cu.train(csr, None, cfg, mode="ials", alpha=40.0, verbose=False, return_stats=True)
    want = 0
    for side in ("users", "items"):
        rated = int((np.diff(ref.own_major(csr, side)[0]) > 0).sum())
        want += rated - len(chk.rows_of_entries(csr, side, entries))
    assert stats.updates == 3 * want, (stats.updates, want)
    assert np.isfinite(P).all() and np.isfinite(Q).all()  # the counted rows keep their finite initial values


def test_predict_I_reports_a_user_it_could_not_fit(tmp_path):
    """bin/predict -I -u on a users file in which one user has a NaN rating: exit status 0, the line on stderr that names one
    user, and every other user's output equal to that of the file without that user."""
    predict = os.path.join(ROOT, "bin", "predict")
    f, items = 8, 50
    rng = np.random.default_rng(5)
    api.writeCSV(str(tmp_path / "q.csv"), rng.normal(0, 0.3, (items, f)).astype(np.float32))
    api.writeCSV(str(tmp_path / "item_bias.csv"), np.zeros((items, 1), np.float32))
    api.writeCSV(str(tmp_path / "global_bias.csv"), np.zeros((1, 1), np.float32))
    (tmp_path / "c.cfg").write_text("0 4 %d 0.01 42 %g %g %g %g\n" % ((f,) + HYPER[1:]))
    good = ["%d,%d,%.1f" % (uid, i + 1, rng.integers(1, 11) / 2) for uid, n in ((3, 6), (7, 1), (12, 9))
            for i in sorted(rng.choice(items, n, replace=False).tolist())]
    bad = ["9,4,2.5", "9,17,nan", "9,30,1.0"]
    (tmp_path / "clean.csv").write_text("\n".join(["userId,itemId,rating"] + good) + "\n")
    (tmp_path / "nan.csv").write_text("\n".join(["userId,itemId,rating"] + good[:7] + bad + good[7:]) + "\n")
    assert np.isnan(cu.createSparseMatrix(str(tmp_path / "nan.csv")).data).sum() == 1
    args = [predict, "-c", str(tmp_path / "c.cfg"), "-i", str(tmp_path / "item_bias.csv"), "-g", str(tmp_path / "global_bias.csv"),
            "-q", str(tmp_path / "q.csv"), "-I", "10", "-u", "-k", "10"]
    runs = {}
    for name in ("clean", "nan"):
        res = subprocess.run(args + [str(tmp_path / (name + ".csv"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode == 0, res.stderr
        runs[name] = res
    assert "could not be fitted" not in runs["clean"].stderr
    assert "predict: 1 user(s) could not be fitted" in runs["nan"].stderr, runs["nan"].stderr
    blocks = {name: {int(b.split("\n")[0]): b for b in res.stdout.split("User: ")[1:]} for name, res in runs.items()}
    assert sorted(blocks["clean"]) == [3, 7, 12] and sorted(blocks["nan"]) == [3, 7, 9, 12]
    for uid in (3, 7, 12):
        assert "Rank: 10\t" in blocks["clean"][uid] and blocks["nan"][uid] == blocks["clean"][uid], uid


@pytest.mark.parametrize("side", ["users", "items"])
def test_explicit_als_counts_only_the_row_of_a_nan_rating(side):
    """Explicit ALS, a NaN rating VALUE (tests/test_gpu_als.py has the NaN partner row): only the row that holds it is counted."""
    csr, entries = chk.poison_entry_set()
    csr = api.HostCSR(csr.indptr, csr.indices, np.where(np.isinf(csr.data), np.float32(2.5), csr.data), csr.rows, csr.cols, 0.0)
    fail = chk.rows_of_entries(csr, side, entries[:1])
    model = model_from(random_state(csr.rows + 3, csr.cols + 5, 16, 31), 0.0)
    report = {}
    als_checks.check_half_step(model, cu.DeviceCSR(csr), csr, side, singular=fail, report=report)
    assert report["unsolved"] == 1


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_explicit_als_non_finite_user_row_leaves_its_items_unchanged(bad):
    """tests/test_gpu_als.py::test_non_finite_item_row_leaves_its_users_unchanged on the item side: the items the poisoned user
    rated are counted and kept, every other item is solved and meets the bar."""
    tr, _ = synth.make_ratings(200, 60, 3000, min_degree=2, seed=31)
    state = [a.copy() for a in random_state(tr.rows, tr.cols, 16, 32)]
    u = int(np.diff(tr.indptr).argmax())
    state[0][u, 3] = bad
    rated_by_u = np.unique(tr.indices[tr.indptr[u]:tr.indptr[u + 1]])
    assert 0 < len(rated_by_u) < len(np.unique(tr.indices))
    model = model_from(state, tr.global_bias)
    report = {}
    als_checks.check_half_step(model, cu.DeviceCSR(tr), tr, "items", singular=rated_by_u, report=report)
    assert report["unsolved"] == len(rated_by_u)


# ---- C: G0 over two workspace batches -------------------------------------------------------------------------------------------
def test_g0_over_two_workspace_batches():
    """f = 252 over 455 x 1,024 + 1 partner rows: the Gram kernel's second batch (chunk0 = 455) is one tile of one row, and
    als_gram_sum_kernel adds it onto the first batch's sum.  Five rows of 1 .. 2,049 entries are judged against float64 (G0 in
    row blocks); +1.0 on the last partner row -- the whole second batch -- changes every one of them, +1.0 on the model row
    behind it none.
    Measured wall time: on an MI355X 2.2 s (1.2 s to make the state and upload the CSR, 0.9 s for the judged half-step with its
    downloads and the float64 G0, 0.1 s for the two further half-steps); the CPU fairness test of the same case
    (tests/test_ials_cpu.py::test_restatement_meets_the_bar_over_two_g0_batches) takes 27 .. 31 s, nearly all of it the float32
    restatement's G0 over 456 tiles."""
    t0 = time.time()
    case, state = chk.big_partner_case(), chk.big_partner_state()
    csr, rows = case.csr, case.csr.rows
    d = cu.DeviceCSR(csr)
    t1 = time.time()
    report = {}
    base = check_half_step(model_from(state, 0.0), d, csr, "users", case.hyper, case.alpha, report=report)[0]
    t2 = time.time()
    Q = state[1]
    for row, moves in ((chk.BIG_PARTNERS - 1, True), (chk.BIG_PARTNERS, False)):
        saved = Q[row].copy()
        Q[row] += 1.0
        try:
            model = model_from(state, 0.0)
        finally:
            Q[row] = saved
        assert ials(model, d, case.hyper, case.alpha, "users") == (0, 0)
        moved = _moved(model.download()[0][:rows], base[:rows])
        assert moved.all() if moves else not moved.any(), (row, moved)
        del model
    print("%s: worst row at %.3g of the bar; state and upload %.1f s, judged half-step %.1f s, two more half-steps %.1f s"
          % (case.name, report[("users", case.f)], t1 - t0, t2 - t1, time.time() - t2))


# ---- D: the objective's grid-stride loops ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", chk.OBJECTIVE_LOOP_SETS)
def test_objective_loops_take_a_second_trip(name):
    """More than 4,096 blocks x 16 groups x 8 entries / rows: 524,288 + 129 entries over 2,000 rows, and as many rows of one
    entry each.  The same tolerance as tests/test_gpu_ials.py::test_objective_matches_float64."""
    case = chk.objective_loop_cases()[name]
    state = case.state()
    model = model_from(state, 0.0)
    got = model.implicit_objective(cu.DeviceCSR(case.csr), case.hyper, case.alpha)
    want = ref.objective(case.csr, state[0], state[1], case.hyper, case.alpha)
    print("%s: objective %.12g, float64 %.12g, off by %.3g" % (name, got, want, abs(got - want) / abs(want)))
    assert same_state(model.download(), state)
    assert abs(got - want) <= 4 * chk.OBJECTIVE_RESTATEMENT_ERROR * abs(want), (name, got, want)


# ---- E: shared objects -----------------------------------------------------------------------------------------------------------
def _then_objective(step):
    """The step, then the objective on the same objects: what the step returned and the objective's value."""
    return lambda m, d: (step(m, d), m.implicit_objective(d, HYPER, 40.0))


def test_explicit_implicit_and_objective_interleaved_on_one_csr():
    """One cu2rec_csr (ALS workspace, item-major view, g0, g0_other, the unsolved counter) serves all three: every step, and the
    objective after it (which overwrites g0 with P's Gram), equals the same on a re-created model and a fresh CSR."""
    tr, _ = synth.make_ratings(300, 80, 5000, min_degree=2, seed=84)
    start = random_state(tr.rows, tr.cols, 16, 85)
    last = interplay([_then_objective(lambda m, d: m.ials(d, HYPER, 40.0, "users")),
                      _then_objective(lambda m, d: m.als(d, SGD_HYPER, "items")),
                      lambda m, d: m.implicit_objective(d, HYPER, 40.0),
                      _then_objective(lambda m, d: m.ials(d, HYPER, 40.0, "items")),
                      _then_objective(lambda m, d: m.als(d, SGD_HYPER, "users")),
                      _then_objective(lambda m, d: m.ials(d, HYPER, 40.0, "both"))], tr, 16, state=start)
    assert all(np.isfinite(a).all() for a in last) and not same_bits(last[0], start[0]) and not same_bits(last[1], start[1])


def test_pingpong_around_implicit_half_steps_then_loss_and_topk():
    """The pending ping-pong swap is finished before an implicit half-step reads or writes Q; loss() and topk() right after one
    read what it left (loss within the bar of tests/test_gpu_als_edges.py::test_loss_right_after_a_half_step)."""
    tr, te = synth.make_ratings(300, 80, 5000, min_degree=2, seed=86)
    objects = []
    last = interplay([lambda m, d: m.sgd(d, SGD_HYPER, 42, 0, 3, mode="pingpong"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "items"),
                      lambda m, d: m.sgd(d, SGD_HYPER, 42, 3, 2, mode="pingpong"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "users")], tr, 16, objects=objects)
    model, d = objects
    got = model.loss(cu.DeviceCSR(te))["rmse"]
    want = als_reference64.rmse(te, *last, tr.global_bias)
    assert abs(got - want) <= 2e-6 * max(1.0, want), (got, want)
    fresh = model_from(last, tr.global_bias)
    for a, b in zip(model.topk(d, 10), fresh.topk(cu.DeviceCSR(tr), 10)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_ordered_and_blocksolve_around_implicit_half_steps_on_one_csr():
    tr, _ = synth.make_ratings(300, 80, 5000, min_degree=2, seed=87)
    last = interplay([lambda m, d: m.sgd(d, SGD_HYPER, 42, 0, 2, mode="ordered"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "both"),
                      lambda m, d: m.sgd(d, SGD_HYPER, 42, 2, 2, mode="blocksolve"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "users"),
                      lambda m, d: m.sgd(d, SGD_HYPER, 42, 4, 2, mode="ordered"),
                      lambda m, d: m.ials(d, HYPER, 40.0, "items"),
                      lambda m, d: m.sgd(d, SGD_HYPER, 42, 6, 2, mode="blocksolve")], tr, 16)
    assert all(np.isfinite(a).all() for a in last)


def test_one_csr_serves_implicit_models_of_different_widths():
    """One DeviceCSR: a sweep and the objective at f = 8, 252, 31, 32 and 8 again (g0 and the workspace regrown, g0's layout
    changing with NT = 1, 8, 1, 2, 1) -- each equal bit for bit to the same on a fresh DeviceCSR."""
    csr = als_checks.batch_set(40, 17).transpose()
    shared = cu.DeviceCSR(csr)
    for step, f in enumerate((8, 252, 31, 32, 8)):
        state = random_state(csr.rows, csr.cols, f, 3100 + step)
        results = []
        for d in (shared, cu.DeviceCSR(csr)):
            m = model_from(state, 0.0)
            assert m.ials(d, HYPER, 40.0, "both") == 0
            results.append((m.download(), m.implicit_objective(d, HYPER, 40.0)))
        assert same_state(results[0][0], results[1][0]) and results[0][1] == results[1][1], (step, f)
        rated_users = np.diff(csr.indptr) > 0
        assert _moved(results[0][0][0], state[0])[rated_users].all() and _moved(results[0][0][1], state[1]).all(), (step, f)


# ---- F: partner range and transposition -------------------------------------------------------------------------------------------
def test_a_user_nobody_names_moves_every_item():
    """The item side's partner range is the CSR's rows: a user row inside it without entries still enters G0 and moves every item
    that has entries (an item without stays the zero row); a model user row past csr.rows moves nothing."""
    csr = chk.messy_set()
    f = 16
    P, Q, ub, ib = random_state(csr.rows + 2, csr.cols, f, 6)
    d = cu.DeviceCSR(csr)
    silent = csr.rows // 2
    assert csr.indptr[silent] == csr.indptr[silent + 1]

    def solved(Px):
        m = model_from((Px, Q, ub, ib), 0.0)
        assert m.ials(d, HYPER, 40.0, "items") == 0
        return m.download()[1]
    base = solved(P)
    inside, outside = P.copy(), P.copy()
    inside[silent] += 1.0
    outside[csr.rows + 1] += 1.0
    rated = np.bincount(csr.indices, minlength=csr.cols) > 0
    moved = _moved(solved(inside), base)
    assert moved[rated].all() and not moved[~rated].any() and (~rated).any()
    assert same_bits(solved(outside), base)


def _messy_entries(rows, cols, nnz, seed):
    """Items unsorted inside a user, repeated (user, item) pairs with different values, values of exactly 0, users and (above a
    handful of items) items without entries."""
    rng = np.random.default_rng(seed)
    counts = rng.multinomial(nnz, np.ones(rows) / rows)
    counts[[0, rows // 2, rows - 1]] = 0
    items = rng.integers(0, cols, counts.sum())
    hot = rng.random(len(items)) < 0.3  # a few popular items: repeats within a user, and item rows past one chunk
    items[hot] = rng.integers(0, min(cols, 3), hot.sum())
    if cols > 4:
        items[items == cols - 2] = 0
        items[-1] = cols - 1
    indptr = np.zeros(rows + 1, np.int64)
    indptr[1:] = np.cumsum(counts)
    return api.HostCSR(indptr, items, rng.integers(0, 11, len(items)).astype(np.float32) / 2, rows, cols, 0.0)


@pytest.mark.parametrize("cols", [1, 2, 65, 65537])
@pytest.mark.parametrize("f", [8, 32])
def test_implicit_item_half_step_equals_user_half_step_of_the_transpose(cols, f):
    """The item half-step (device transposition, X = P[0:csr.rows], Q_reg) equals bit for bit the user half-step of the
    transposed problem: the sides, the biases and the regularisers swapped, the CSR transposed on the host."""
    R = _messy_entries(300, cols, 6000, 700 + cols % 1000)
    rows = R.rows
    P, Q, ub, ib = random_state(rows, cols, f, 800 + f)
    hyper = (0.01, 0.8, 1.2, 0.5, 0.012)
    direct = cu.Model(rows, cols, f, 0.0, P=P, Q=Q, user_bias=ub, item_bias=ib)
    assert ials(direct, cu.DeviceCSR(R), hyper, 40.0, "items") == (0, 0)
    swapped = cu.Model(cols, rows, f, 0.0, P=Q, Q=P, user_bias=ib, item_bias=ub)
    assert ials(swapped, cu.DeviceCSR(R.transpose()), (0.01, hyper[2], 7.0, 0.3, 9.0), 40.0, "users") == (0, 0)
    Pd, Qd, ubd, ibd = direct.download()
    Qs, Ps, ibs, ubs = swapped.download()
    assert same_bits(Pd, P) and same_bits(ubd, ub) and same_bits(Ps, P) and same_bits(ubs, ub)
    rated = np.bincount(R.indices, minlength=cols) > 0
    assert _moved(Qd, Q)[rated].all() and not Qd[~rated].any()
    differ = np.flatnonzero(_moved(Qd, Qs) | (ibd.view(np.uint32) != ibs.view(np.uint32)))
    assert len(differ) == 0, ("items differ from the users of the transposed problem", f, cols, differ[:8].tolist())


def test_no_entries_at_all():
    """A CSR without a single entry: both sides' rows inside it become zero rows (G0 + reg I against a zero right-hand side),
    the model rows past it keep their bits, and nothing is counted."""
    R = api.HostCSR(np.zeros(11, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 10, 7, 0.0)
    state = random_state(12, 9, 8, 5)
    model = model_from(state, 0.0)
    d = cu.DeviceCSR(R)
    for side in ("users", "items", "users"):
        check_half_step(model, d, R, side, HYPER, 40.0)
    P, Q, ub, ib = model.download()
    assert not P[:10].any() and not Q[:7].any() and not ub[:10].any() and not ib[:7].any()
    assert same_bits(P[10:], state[0][10:]) and same_bits(Q[7:], state[1][7:])
    assert model.implicit_objective(d, HYPER, 40.0) == 0.0
