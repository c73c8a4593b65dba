"""Alternating least squares on the GPU at its edges: every tile count crossed with every length class, several workspace
batches, the device transposition pinned bit for bit, conditioning and regulariser classes, the SGD modes around it on shared
objects, and sampled rows at the ML-20M shape.

A solved row is judged three ways (tests/als_checks.check_half_step): the forward bar of tests/test_gpu_als.py against the float64
optimum where the system is well conditioned; its float64 residual against the entrywise rounding bound derived in
als_reference64.row_residual everywhere; and everything the half-step does not own bit for bit.  tests/test_als_cpu.py shows on the
CPU that a plain float32 restatement of the row solve meets the bound on the conditioning sets used here and that three
deliberate mistakes do not."""
import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib

import als_checks as chk
import als_reference64 as ref
from als_checks import HYPER, als, check_half_step, model_from, random_state, same_bits

pytestmark = pytest.mark.gpu


def _same_state(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


# ---- B.1: widths x lengths ---------------------------------------------------------------------------------------------------
WIDTHS = [30, 31, 62, 63, 94, 95, 126, 127, 158, 159, 190, 191, 222, 223, 252]  # f + 2 = 32 NT and 32 NT + 1, NT = 1 .. 8


@pytest.mark.parametrize("f", WIDTHS)
def test_widths_x_lengths_both_sides(f):
    """Rows of 1, 2, 31 .. 33, 1,023 .. 1,025, 2,047 .. 2,049 and 4,097 ratings (at f = 95 and 252 also 64 x 1,024 + 1) and 200
    rows of 1 .. 64, solved as users of the set and as items of its transpose, from factors of O(0.3) and again after a sweep."""
    rows_major = chk.width_length_set(extra_long=f in (95, 252))
    for side, csr in (("users", rows_major), ("items", rows_major.transpose())):
        d = cu.DeviceCSR(csr)
        model = model_from(random_state(csr.rows + 3, csr.cols + 5, f, 1000 + f), csr.global_bias)
        check_half_step(model, d, csr, side, residual=True)
        assert model.als(d, HYPER, "both", sweeps=1) == 0
        check_half_step(model, d, csr, side, residual=True)


# ---- B.2: the item half-step is the user half-step of the transposed problem ------------------------------------------------
def _messy_csr(rows, cols, nnz, seed, csr_cols=None):
    """Items unsorted inside a user, repeated (user, item) pairs with different ratings, empty users first, in the middle and
    last, unrated items (at large cols nearly all of them)."""
    rng = np.random.default_rng(seed)
    counts = rng.multinomial(nnz, np.ones(rows) / rows)
    counts[[0, rows // 2, rows - 1]] = 0
    items = rng.integers(0, cols, counts.sum())
    hot = rng.random(len(items)) < 0.3  # a few popular items: repeats within a user, and item rows past one chunk
    items[hot] = rng.integers(0, min(cols, 3), hot.sum())
    if cols > 4:
        items[items == cols - 2] = 0  # item cols - 2 stays unrated; cols - 1 is rated so that max_item == cols - 1
        items[-1] = cols - 1
    indptr = np.zeros(rows + 1, np.int64)
    indptr[1:] = np.cumsum(counts)
    ratings = rng.integers(1, 11, len(items)).astype(np.float32) / 2
    return api.HostCSR(indptr, items, ratings, rows, cols if csr_cols is None else csr_cols, float(np.float32(ratings.mean())))


def _items_equal_users_of_transpose(R, cols, f, seed):
    rows = R.rows
    P, Q, ub, ib = random_state(rows, cols, f, seed)
    gb, hyper = R.global_bias, (0.01, 0.05, 0.15, 0.5, 0.012)
    direct = cu.Model(rows, cols, f, gb, P=P, Q=Q, user_bias=ub, item_bias=ib)
    rc, n_direct = als(direct, cu.DeviceCSR(R), hyper, "items")
    assert rc == 0, lib().cu2rec_last_error()
    # the transposed problem: items become the users (rows and cols swapped, P_reg := Q_reg, user_bias_reg := item_bias_reg)
    Rt = api.HostCSR(R.indptr, R.indices, R.data, rows, cols, gb).transpose()
    swapped = cu.Model(cols, rows, f, gb, P=Q, Q=P, user_bias=ib, item_bias=ub)
    rc, n_swapped = als(swapped, cu.DeviceCSR(Rt), (0.01, hyper[2], 7.0, hyper[4], 9.0), "users")
    assert rc == 0, lib().cu2rec_last_error()
    Pd, Qd, ubd, ibd = direct.download()
    Qs, Ps, ibs, ubs = swapped.download()
    assert n_direct == n_swapped == 0
    assert same_bits(Pd, P) and same_bits(ubd, ub) and same_bits(Ps, P) and same_bits(ubs, ub)
    rated = np.bincount(R.indices, minlength=cols) > 0
    assert same_bits(Qd[~rated], Q[~rated]) and same_bits(ibd[~rated], ib[~rated])
    assert not same_bits(Qd[rated], Q[rated]) or not rated.any()
    differ = np.flatnonzero((Qd.view(np.uint32) != Qs.view(np.uint32)).any(axis=1) | (ibd.view(np.uint32) != ibs.view(np.uint32)))
    assert len(differ) == 0, ("items differ from the users of the transposed problem", f, cols, differ[:8].tolist())


@pytest.mark.parametrize("cols", [1, 2, 64, 65, 65536, 65537, 200001])
@pytest.mark.parametrize("f", [8, 30])
def test_item_half_step_equals_user_half_step_of_the_transpose(cols, f):
    _items_equal_users_of_transpose(_messy_csr(300, cols, 6000, 500 + cols % 1000), cols, f, 600 + f)


def test_item_half_step_with_csr_cols_above_the_models():
    """A cu2rec_csr created with more columns than the model has items (legal: only max_item < cols is required)."""
    cols = 100
    R = _messy_csr(300, cols, 6000, 77, csr_cols=cols + 29)
    assert R.indices.max() == cols - 1
    _items_equal_users_of_transpose(R, cols, 8, 78)


@pytest.mark.parametrize("side", ["users", "items"])
def test_no_ratings_changes_nothing(side):
    R = api.HostCSR(np.zeros(11, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 10, 7, 3.5)
    state = random_state(10, 7, 8, 5)
    model = model_from(state, 3.5)
    d = cu.DeviceCSR(R)
    for _ in range(2):
        assert als(model, d, HYPER, side) == (0, 0)
    assert _same_state(model.download(), state)


# ---- B.3: conditioning and regulariser edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("f", [8, 100])
def test_conditioning_classes(f, side):
    """The labelled classes of als_checks.conditioning_cases.  Every row outside `singular` is solved and within the residual
    bound (the forward bar as well on the rows of Case.well_conditioned(): the ordinary classes of every case, less the rows of
    fewer ratings than factors at factor regulariser 1e-4); a `singular` row is either counted and bit-identical or finite and
    within the bound, and at least one is counted; no solved row's own objective rises above its starting value plus the slack.

    Recorded, not asserted -- worst residual / bound of the float32 numpy restatement on the same inputs (tests/test_als_cpu.py):
    f = 8: base 0.043, bias0 0.035, reg_1e-4 0.026, reg_10 0.043, cancel 0.0093; f = 100: base 0.012, bias0 0.021,
    reg_1e-4 0.0088, reg_10 0.033, cancel 0.0076; singular: all 13 rows meet a bad pivot."""
    for case in chk.conditioning_cases(f):
        csr, state, hyper = case.for_side(side)
        d = cu.DeviceCSR(csr)
        model = model_from(state, csr.global_bias)
        report = {}
        check_half_step(model, d, csr, side, hyper, forward=case.well_conditioned(), residual=True, row_objective=True,
                        singular=range(case.csr.rows) if case.singular else (), label=lambda r: (case.name, case.class_of.get(r)),
                        report=report)
        if case.singular:  # the counted-and-unchanged path is really taken: float32 cannot factorise these (the restatement: none of 13)
            assert report["unsolved"] >= 1, (f, side, "every singular row was factorised: the unsolved path did not run")
        print("f=%d %s %-9s worst residual/bound %.3g, forward/bar %.3g, unsolved %d of %d"
              % (f, side, case.name, report["residual"], report["forward"], report["unsolved"], case.csr.rows))


# ---- B.4: several workspace batches ------------------------------------------------------------------------------------------
def _batch_cuts(lengths, f):
    """Indices (into the long rows) of the first row of every batch after the first, by the header's workspace arithmetic."""
    nt = (f + 2 + 31) // 32
    batch_chunks = api.ALS_WORKSPACE_BYTES // (nt * (nt + 1) // 2 * 16 * 64 * 4)
    cuts, used = [], 0
    for i, n in enumerate(lengths):
        c = chk.chunks_of(n)
        if used and used + c > batch_chunks:
            cuts.append(i)
            used = 0
        used += c
    return cuts


def _one_item_alone(csr, state, j, f, hyper):
    """Item j's half-step from a CSR that holds only item j (as item 0), against the same users."""
    P, Q, ub, ib = state
    mask = csr.indices == j
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))[mask]
    indptr = np.zeros(csr.rows + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(users, minlength=csr.rows))
    one = api.HostCSR(indptr, np.zeros(mask.sum(), np.int32), csr.data[mask], csr.rows, 1, csr.global_bias)
    m = cu.Model(csr.rows, 1, f, csr.global_bias, P=P, Q=Q[j:j + 1], user_bias=ub, item_bias=ib[j:j + 1])
    assert m.als(cu.DeviceCSR(one), hyper, "items") == 0
    _, Q1, _, ib1 = m.download()
    return Q1[0], ib1[0]


@pytest.mark.parametrize("f,n_long,chunks_each,batches", [(252, 40, 17, 2), (252, 9, 64, 2), (30, 40, 17, 1)])
def test_long_rows_over_workspace_batches(f, n_long, chunks_each, batches):
    """An item side whose long rows need more partial Grams than the workspace holds at f = 252 (455 chunks): 40 rows of 17
    chunks (the cut falls between rows 25 and 26), 9 rows of 64 (the eighth would straddle the bound and starts the next
    batch); f = 30 fits one batch and is the control.  The rows on both sides of every cut, the first and the last equal their
    own one-row solve bit for bit."""
    rows_major = chk.batch_set(n_long, chunks_each)
    lengths = np.diff(rows_major.indptr)[:n_long]
    assert all(chk.chunks_of(int(n)) == chunks_each for n in lengths)
    cuts = _batch_cuts(lengths, f)
    assert len(cuts) == batches - 1
    csr = rows_major.transpose()  # the long rows are items 0 .. n_long - 1
    d = cu.DeviceCSR(csr)
    state = random_state(csr.rows, csr.cols, f, 2000 + f + chunks_each)
    model = model_from(state, csr.global_bias)
    got = check_half_step(model, d, csr, "items", residual=True)
    for j in sorted({0, n_long - 1} | {c - 1 for c in cuts} | set(cuts)):
        q, b = _one_item_alone(csr, state, j, f, HYPER)
        assert same_bits(q, got[1][j]) and same_bits(b, got[3][j]), ("item differs from its one-row solve", f, j, cuts)


def test_workspace_is_regrown_when_one_csr_serves_a_wider_model():
    """One DeviceCSR: an item half-step at f = 8, then at f = 252 (the cached workspace has to grow), then f = 8 again -- each
    equal bit for bit to the same half-step on a fresh DeviceCSR."""
    csr = chk.batch_set(40, 17).transpose()
    shared = cu.DeviceCSR(csr)
    for step, f in enumerate((8, 252, 8)):
        state = random_state(csr.rows, csr.cols, f, 3000 + step)
        results = []
        for d in (shared, cu.DeviceCSR(csr)):
            m = model_from(state, csr.global_bias)
            assert m.als(d, HYPER, "items") == 0
            results.append(m.download())
        assert _same_state(*results), (step, f)
        assert not same_bits(results[0][1][:40], state[1][:40])


# ---- B.5: the SGD modes around ALS on shared objects --------------------------------------------------------------------------
def test_pingpong_als_pingpong_on_one_model():
    tr, _ = synth.make_ratings(300, 80, 5000, min_degree=2, seed=81)
    hyper = (0.01, 0.05, 0.04, 0.02, 0.03)
    first = chk.interplay([lambda m, d: m.sgd(d, hyper, 42, 0, 3, mode="pingpong"),
                           lambda m, d: m.als(d, hyper, "items"),
                           lambda m, d: m.sgd(d, hyper, 42, 3, 3, mode="pingpong"),
                           lambda m, d: m.als(d, hyper, "both"),
                           lambda m, d: m.sgd(d, hyper, 42, 6, 2, mode="pingpong")], tr, 16)
    assert all(np.isfinite(a).all() for a in first)


def test_ordered_and_blocksolve_around_als_on_one_csr():
    tr, _ = synth.make_ratings(300, 80, 5000, min_degree=2, seed=82)
    hyper = (0.01, 0.05, 0.04, 0.02, 0.03)
    last = chk.interplay([lambda m, d: m.sgd(d, hyper, 42, 0, 2, mode="ordered"),
                          lambda m, d: m.als(d, hyper, "both"),
                          lambda m, d: m.sgd(d, hyper, 42, 2, 2, mode="blocksolve"),
                          lambda m, d: m.als(d, hyper, "users"),
                          lambda m, d: m.sgd(d, hyper, 42, 4, 2, mode="ordered"),
                          lambda m, d: m.als(d, hyper, "items"),
                          lambda m, d: m.sgd(d, hyper, 42, 6, 2, mode="blocksolve")], tr, 16)
    assert all(np.isfinite(a).all() for a in last)


@pytest.mark.parametrize("side", ["users", "items"])
def test_loss_right_after_a_half_step(side):
    """loss() reads the state the half-step left (after ping-pong iterations: the pending swap has been finished), within the
    bar tests/test_gpu_parity.py holds loss to against float64."""
    tr, te = synth.make_ratings(300, 80, 5000, min_degree=2, seed=83)
    d, dte = cu.DeviceCSR(tr), cu.DeviceCSR(te)
    model = cu.Model(tr.rows, tr.cols, 16, tr.global_bias)
    model.sgd(d, HYPER, 42, 0, 3, mode="pingpong")
    assert model.als(d, HYPER, side) == 0
    got = model.loss(dte)["rmse"]
    want = ref.rmse(te, *model.download(), tr.global_bias)
    assert abs(got - want) <= 2e-6 * max(1.0, want), (got, want)


# ---- B.6: the ML-20M shape, sampled --------------------------------------------------------------------------------------------
def test_full_shape_ml20m_sampled_rows():
    """One sweep at f = 100 from the seed-42 model, then one more half-step per side, each with no unsolved row; after each of the
    last two, the 64 longest rows of the side, every row of exactly 1, 1,024 and 1,025 ratings and 1,024 rows drawn with a fixed
    seed are judged in float64 (forward bar and residual bound); every other row must be finite and the other side unmoved."""
    import bench
    tr, _ = bench.load_dataset("ml-20m", 20240917, 0, lambda: None)
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, 100, tr.global_bias)
    assert model.als(d, HYPER, "both", sweeps=1) == 0
    rng = np.random.default_rng(20)
    for side in ("users", "items"):
        counts = np.diff(tr.indptr) if side == "users" else np.bincount(tr.indices, minlength=tr.cols)
        rated = np.flatnonzero(counts > 0)
        rows = np.concatenate([np.argsort(counts, kind="stable")[-64:], np.flatnonzero(np.isin(counts, (1, 1024, 1025))),
                               rng.choice(rated, min(1024, len(rated)), replace=False)])
        report = {}
        check_half_step(model, d, tr, side, residual=True, rows=np.unique(rows), report=report)
        print("ml-20m f=100 %s: %d rows judged, longest %d, worst residual/bound %.3g, forward/bar %.3g"
              % (side, len(np.unique(rows)), counts.max(), report["residual"], report["forward"]))
