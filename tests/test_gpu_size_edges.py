"""Problem sizes at which launches change shape (-m gpu): every mode and the top-k / rank-metric passes past the size thresholds
that no other test reaches, against the same references as everywhere else and as strictly as the mode allows:
  * ordered, ping-pong, Hogwild with the item side frozen and the loss pass: the CPU oracle (TREE16 dot order), bit for bit;
  * block-solve: within 2e-6 of the oracle (5e-6 across resumed calls, as in tests/test_gpu_blocksolve.py);
  * top-k: cu2rec_model_recommend bit for bit; rank metrics: tests/rank_reference.py within 1e-12.
Each test first restates the rule it targets (the helpers below, each citing its source) and asserts that its shape lies past it,
so that a change of the shapes cannot quietly move a case back to the regime every other test already covers."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd.api import HostCSR
from oracle import oracle as orc
import rank_reference as rr

pytestmark = pytest.mark.gpu

HYPER = (0.01, 0.02, 0.03, 0.04, 0.05)  # lr, P_reg, Q_reg, user_bias_reg, item_bias_reg: distinct, so a swapped term shows


# ---------------------------------------------------------------------------------------------- the rules, restated

def bits_for(n):
    """ordered.hip, bits_for: bits for values in [0, n) -- at least 1, so one item takes a bit too."""
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def schedule_window(n_rows, n_cols):
    """ordered.hip, OrderedSchedule::OrderedSchedule: max_batch, the iterations of one schedule window.  64, halved while the key
    (b << item_bits | rank, plus the sentinel bit) would not fit 32 bits, then while max_batch * n_rows > 2^27 (n_rows counts
    empty rows too)."""
    mb = 1 << min(6, 31 - bits_for(n_cols) - 1)
    while mb > 1 and mb * n_rows > (1 << 27):
        mb >>= 1
    return mb


def rank_clamp(n_cols):
    """ordered.hip, OrderedSchedule::OrderedSchedule / run(): n_hot, n_hot_bs, n_duo_bs and n_range_ranks are clamped to
    (1 << item_bits) - 1, "keep r + 1 representable"."""
    return (1 << bits_for(n_cols)) - 1


PINGPONG_CLAIM_THREADS = 4096 * 256  # kernels.hip, launch_sgd_pingpong: the claim kernel's grid is capped at 4096 blocks of 256


def pingpong_start_user(it, n_rows):
    """kernels.hip, pingpong_key (training.cu:97-98,115): thread gid handles user (gid + start_user) % n_rows."""
    return (250 * it) % n_rows


def topk_batch(n_users, n_cols, k, masked, extra=0):
    """topk.hip, TopkRunner: users per batch of a 256 MiB workspace -- 64 E 8-byte candidates (E = 4 for k <= 128, else 8), the
    exclusion bitmap (4 bytes per 32 items) if there are exclusions, 8 k bytes of output and `extra` (rank_metrics: a relevance
    bitmap and a count); whole 32-user tiles, at least one."""
    E = 4 if k + 128 <= 256 else 8
    words = (n_cols + 31) // 32
    per_pos = 64 * E * 8 + (4 * words if masked else 0) + 8 * k + extra
    fit = max(32, (256 << 20) // per_pos // 32 * 32)
    return min(fit, -(-n_users // 32) * 32)


# ---------------------------------------------------------------------------------------------- data and references

def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


def _csr(rows, cols, active, deg, items, rng):
    """HostCSR of `rows` rows: rows `active` (ascending) get deg[i] ratings, the items taken in order from `items`."""
    counts = np.zeros(rows, np.int64)
    counts[active] = deg
    indptr = np.zeros(rows + 1, np.int64)
    np.cumsum(counts, out=indptr[1:])
    assert indptr[-1] == len(items) < 2 ** 31
    data = (rng.randint(1, 11, len(items)) / 2).astype(np.float32)
    return HostCSR(indptr.astype(np.int32), np.asarray(items, np.int32), data, rows, cols, float(data.mean(dtype=np.float64)))


def _skewed(rng, n_cols, n, offset):
    """n item ids with popularity ~ 1 / (rank + offset), ranks scattered over the ids"""
    p = 1.0 / (np.arange(n_cols) + float(offset))
    return rng.permutation(n_cols)[rng.choice(n_cols, n, p=p / p.sum())]


def _rates(tr):
    """Expected updates per iteration of every item (sum over its raters of 1 / degree) and the popularity order
    (descending, ties by item id): ordered.hip, OrderedSchedule::OrderedSchedule."""
    rate = api.item_update_rates(tr)
    return rate, np.argsort(-rate, kind="stable")


def _max_diff(got, want):
    return max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want))


def _assert_equal(got, want, what):
    for name, g, w in zip(("P", "Q", "user_bias", "item_bias"), got, want):
        assert np.array_equal(g, w), "%s: %s differs from the oracle" % (what, name)


@pytest.fixture
def min_rate():
    prev = api.blocksolve_min_rate()
    yield api.blocksolve_min_rate
    api.blocksolve_min_rate(prev)  # a negative value restores the automatic threshold, a positive one the explicit value


def _schedules(tr, rate, lookahead=None):
    """DeviceCSRs whose schedules (created here: they read the block-solve settings) serve one mode each, so that every mode runs
    out of windows of its own: {"ordered", "blocksolve"[, "lookahead"]}."""
    api.blocksolve_min_rate(rate)
    out = {"ordered": cu.DeviceCSR(tr), "blocksolve": cu.DeviceCSR(tr)}
    for d in out.values():
        assert d.blocksolve_items() >= 0
    if lookahead is not None:
        prev = api.blocksolve_lookahead_blocks(lookahead)
        try:
            out["lookahead"] = cu.DeviceCSR(tr)
            assert out["lookahead"].blocksolve_items() > 0
        finally:
            api.blocksolve_lookahead_blocks(prev)
    return out


def _run_calls(tr, f, devs, calls):
    """The calls (seed, iter0, n) one after the other, one DeviceCSR per mode, and the oracle beside them (on a host thread: its
    ctypes call releases the GIL).  The ordered model runs the whole sequence and equals the oracle bit for bit after every call.
    Each block-solve call starts from the oracle's state in a fresh model: the schedule windows (ordered.hip, Window) belong to
    the DeviceCSR and still continue from call to call, while the mode's rounding does not pile up across calls -- within 2e-6
    of the oracle after the first call (from the initialisation), 5e-6 after a resumed one (trained values: larger rows, larger
    rounding; tests/test_gpu_blocksolve.py).  -> the oracle's final state."""
    state = orc.init_model(tr.rows, tr.cols, f)
    o_tr = _as_orc(tr)
    exact_model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    solved_differs = False
    with ThreadPoolExecutor(1) as pool:
        for k, (seed, it0, n) in enumerate(calls):
            solved = {name: cu.Model(tr.rows, tr.cols, f, tr.global_bias, *state) for name in devs if name != "ordered"}
            fut = pool.submit(orc.sgd_iterations, o_tr, *state, tr.global_bias, HYPER, seed, it0, n, dot_order=orc.DOT_TREE16)
            exact_model.sgd(devs["ordered"], HYPER, seed, it0, n, mode="ordered")
            for name, model in solved.items():
                model.sgd(devs[name], HYPER, seed, it0, n, mode="blocksolve")
            fut.result()
            exact = exact_model.download()
            _assert_equal(exact, state, "ordered, call %d %s" % (k, (seed, it0, n)))
            for name, model in solved.items():
                got = model.download()
                diff = _max_diff(got, state)
                assert diff <= (2e-6 if k == 0 else 5e-6), (name, k, (seed, it0, n), diff)
                solved_differs |= any(not np.array_equal(g, w) for g, w in zip(got, exact))
    assert solved_differs, "block-solve equals the ordered walk bit for bit after every call: its kernels did not run"
    return state


def _assert_loss(tr, f, state):
    """The loss pass on this shape: residuals bit for bit, RMSE / MAE equal, the double sums within 1e-11 (summed in another
    order over up to 8.4 M residuals: the bound of tests/test_gpu_parity.py's full Netflix shape)."""
    from cu2rec_amd.engine import DeviceRatings, Engine
    eng = Engine(tr.rows, tr.cols, f, tr.global_bias, *state)
    got = eng.loss(DeviceRatings(tr, eng.device), want_errors=True)
    want = orc.loss(_as_orc(tr), *state, tr.global_bias, dot_order=orc.DOT_TREE16, acc=orc.ACC_F64, want_errors=True)
    np.testing.assert_array_equal(got["errors"], want["errors"])
    assert got["rmse"] == want["rmse"] and got["mae"] == want["mae"], (got, want)
    for name in ("sum_sq", "sum_abs"):
        assert abs(got[name] - want[name]) <= 1e-11 * want[name], name


# the call sequence of test_blocksolve_calls_of_any_length_share_schedule_windows: calls that continue each other at every offset
# into a window, across window ends, then a jump back, a jump ahead and another seed
CALLS = [(42, 0, 7), (42, 7, 20), (42, 27, 50), (42, 77, 3), (42, 80, 70), (42, 5, 10), (42, 300, 9), (7, 309, 30)]


# ---------------------------------------------------------------------------------------------- A. windows of 32 and 16

def test_window_of_32_iterations_from_rows_mostly_empty(min_rate):
    """2^21 + 1 rows, 30,000 of them with ratings: past ordered.hip OrderedSchedule::OrderedSchedule's 64 * n_rows > 2^27, so the
    windows are 32 iterations, and every sort segment of 2^21 + 1 pairs ends in a tail of 2 M sentinel keys.  Ordered, block-solve
    and the look-ahead form of block-solve, over calls of any length; then the loss pass."""
    rng = np.random.RandomState(21)
    rows, cols, f = (1 << 21) + 1, 300, 8
    assert 64 * rows > 1 << 27 and 32 * rows <= 1 << 27 and schedule_window(rows, cols) == 32
    active = np.sort(np.concatenate([[0, rows - 1], rng.choice(np.arange(1, rows - 1), 29_998, replace=False)]))
    deg = rng.randint(3, 13, len(active))
    tr = _csr(rows, cols, active, deg, _skewed(rng, cols, int(deg.sum()), 5), rng)
    devs = _schedules(tr, 200.0, lookahead=2)
    rate, order = _rates(tr)
    hot = int((rate >= 200.0).sum())
    assert devs["blocksolve"].blocksolve_items() == hot > 0
    assert rate[order[0]] >= 2 * 64  # look-ahead chains (at least two 64-link blocks per iteration) exist
    state = _run_calls(tr, f, devs, CALLS)
    _assert_loss(tr, f, state)


def test_window_of_16_iterations_from_rows_all_active(min_rate):
    """2^22 + 1 rows, every one with 1-3 ratings: past ordered.hip OrderedSchedule::OrderedSchedule's 32 * n_rows > 2^27, so the
    windows are 16 iterations.  Item popularity ~ 1 / (rank + 100) over 4,096 items: the hottest chains are ~10,000 links.
    Ordered and block-solve over calls that continue each other across three windows (the CPU oracle takes ~1 s per iteration
    here: the sequence is shorter than CALLS), then a jump back, a jump ahead and another seed; then the loss pass."""
    rng = np.random.RandomState(22)
    rows, cols, f = (1 << 22) + 1, 4096, 4
    assert 32 * rows > 1 << 27 and 16 * rows <= 1 << 27 and schedule_window(rows, cols) == 16
    deg = rng.randint(1, 4, rows)
    tr = _csr(rows, cols, np.arange(rows), deg, _skewed(rng, cols, int(deg.sum()), 100), rng)
    devs = _schedules(tr, 5000.0)
    rate, _ = _rates(tr)
    assert devs["blocksolve"].blocksolve_items() == int((rate >= 5000.0).sum()) > 0
    calls = [(42, 0, 5), (42, 5, 14), (42, 19, 2), (42, 21, 13), (42, 3, 1), (42, 90, 2), (7, 92, 1)]
    state = _run_calls(tr, f, devs, calls)
    _assert_loss(tr, f, state)


def test_window_of_32_iterations_from_a_catalogue_above_2_24_items(min_rate):
    """2^24 + 1 items: item_bits = 25 > 24, so ordered.hip OrderedSchedule::OrderedSchedule's key budget (31 - item_bits - 1 bits
    of iteration) leaves windows of 32.  4,000 users, 8 ratings each: two of 8 popular items (the last item id among them), six
    anywhere in the catalogue.  Ordered and block-solve over calls of any length; then the loss pass."""
    rng = np.random.RandomState(24)
    rows, cols, f = 4000, (1 << 24) + 1, 4
    assert bits_for(cols) == 25 and schedule_window(rows, cols) == 32 and 64 * rows <= 1 << 27
    popular = np.concatenate([[cols - 1], rng.choice(cols - 1, 7, replace=False)])
    items = np.empty((rows, 8), np.int64)
    items[:, :2] = popular[rng.randint(0, 8, (rows, 2))]
    items[:, 2:] = rng.randint(0, cols, (rows, 6))
    tr = _csr(rows, cols, np.arange(rows), np.full(rows, 8), items.reshape(-1), rng)
    devs = _schedules(tr, 20.0)
    rate, _ = _rates(tr)
    assert devs["blocksolve"].blocksolve_items() == int((rate >= 20.0).sum()) == 8
    state = _run_calls(tr, f, devs, CALLS[:5] + [(42, 5, 10), (7, 309, 30)])
    _assert_loss(tr, f, state)


# ---------------------------------------------------------------------------------------------- B. power-of-two catalogues

@pytest.mark.parametrize("cols", [1, 2, 4, 64, 256, 257, 1024])
def test_power_of_two_catalogues_every_item_above_the_threshold(min_rate, cols):
    """n_cols = 2^k: ordered.hip's clamp of n_hot / n_hot_bs / n_duo_bs / n_range_ranks to (1 << item_bits) - 1 leaves the least
    popular item to the walk even though every item is above the block-solve threshold (and bits_for(1) = 1: one item is hot).
    The first `cols` users rate one item each, so every item -- the clamped one included -- is updated in every iteration.
    Ordered bit for bit, block-solve within 2e-6."""
    rng = np.random.RandomState(cols)
    users, f, iters = max(2000, 8 * cols), 8, 12
    deg = np.concatenate([np.ones(cols, np.int64), rng.randint(1, 6, users - cols)])
    items = np.concatenate([np.arange(cols), _skewed(rng, cols, int(deg[cols:].sum()), 3)])
    tr = _csr(users, cols, np.arange(users), deg, items, rng)
    rate, order = _rates(tr)
    assert rate.min() >= 1.0
    devs = _schedules(tr, 0.5)
    want_hot = min(cols, rank_clamp(cols))
    assert devs["blocksolve"].blocksolve_items() == want_hot
    if cols & (cols - 1) == 0 and cols > 1:
        assert want_hot == cols - 1  # the clamp binds: the least popular item is walked
    state0 = orc.init_model(users, cols, f)
    state = _run_calls(tr, f, devs, [(42, 0, iters)])
    last = order[-1]  # rank cols - 1
    assert not np.array_equal(state[1][last], state0[1][last]) and state[3][last] != state0[3][last]


# ---------------------------------------------------------------------------------------------- C. ping-pong beyond one grid

def _pingpong_raw(eng, d, cur, other, claim, it0, n):
    """cu2rec_sgd_update_pingpong on (current, other) buffer pairs -> swapped"""
    import ctypes as C
    from cu2rec_amd._lib import Hyper, check, lib
    swapped = C.c_int(-1)
    h = Hyper(*HYPER)
    check(lib().cu2rec_sgd_update_pingpong(d.indptr.data_ptr(), d.indices.data_ptr(), d.data.data_ptr(), d.rows, d.cols,
                                           eng.P.data_ptr(), eng.ld, cur[0].data_ptr(), other[0].data_ptr(), eng.ldq,
                                           eng.user_bias.data_ptr(), cur[1].data_ptr(), other[1].data_ptr(), claim.data_ptr(),
                                           eng.global_bias, eng.f, C.byref(h), 42, it0, n, 1, 0, 1, C.byref(swapped), None))
    return swapped.value == 1


@pytest.mark.parametrize("rows,iter0", [((1 << 20) + 1, 4193), (1_500_000, 5998)])
def test_pingpong_and_frozen_item_hogwild_above_one_claim_grid(rows, iter0):
    """More rows than kernels.hip launch_sgd_pingpong's claim grid has threads (4096 x 256 = 1,048,576): users past it are
    claimed in the grid-stride loop.  iter0 is chosen so that start_user = 250 it mod n_rows wraps inside the first call.  Two
    calls (3 + 2 iterations, continuing each other): after each, BOTH buffer pairs equal the oracle's bit for bit.  Then Hogwild
    with the item side frozen at the same shape: P and user_bias bit for bit."""
    import torch
    from cu2rec_amd.engine import DeviceRatings, Engine
    assert rows > PINGPONG_CLAIM_THREADS
    starts = [pingpong_start_user(it, rows) for it in range(iter0, iter0 + 5)]
    assert any(b < a for a, b in zip(starts, starts[1:3])), starts  # the wrap falls inside the first call
    rng = np.random.RandomState(rows)
    cols, f = 2000, 8
    active = np.flatnonzero(rng.rand(rows) > 0.1)  # a tenth of the users without ratings (sgd.cu:34)
    active = np.union1d(active, [rows - 1])
    deg = rng.randint(1, 5, len(active))
    tr = _csr(rows, cols, active, deg, _skewed(rng, cols, int(deg.sum()), 20), rng)
    P, Q, ub, ib = orc.init_model(rows, cols, f)
    eng = Engine(rows, cols, f, tr.global_bias, P, Q, ub, ib)
    d = DeviceRatings(tr, eng.device)
    bufs = [(eng.Q, eng.item_bias), (eng.Q.clone(), eng.item_bias.clone())]  # [current, other]
    claim = torch.empty(cols, dtype=torch.int64, device=eng.device)
    Qt, ibt = Q.copy(), ib.copy()
    for it0, n in ((iter0, 3), (iter0 + 3, 2)):
        if _pingpong_raw(eng, d, bufs[0], bufs[1], claim, it0, n):
            bufs.reverse()
        orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, HYPER, 42, it0, n,
                                    dot_order=orc.DOT_TREE16)
        torch.cuda.synchronize()
        for name, g, w in (("P", eng.P[:rows, :f], P), ("user_bias", eng.user_bias, ub), ("Q", bufs[0][0][:cols, :f], Q),
                           ("item_bias", bufs[0][1], ib), ("other Q", bufs[1][0][:cols, :f], Qt),
                           ("other item_bias", bufs[1][1], ibt)):
            assert np.array_equal(g.cpu().numpy(), w), (name, it0, n)
    del eng, d, bufs, claim

    P, Q, ub, ib = orc.init_model(rows, cols, f)
    Q0, ib0 = Q.copy(), ib.copy()
    model = cu.Model(rows, cols, f, tr.global_bias)
    model.sgd(cu.DeviceCSR(tr), HYPER, 42, iter0, 3, mode="hogwild", update_items=False)
    orc.sgd_iterations(_as_orc(tr), P, Q, ub, ib, tr.global_bias, HYPER, 42, iter0, 3, dot_order=orc.DOT_TREE16,
                       update_items=False)
    gP, gQ, gub, gib = model.download()
    assert np.array_equal(gQ, Q0) and np.array_equal(gib, ib0)
    assert np.array_equal(gP, P) and np.array_equal(gub, ub)


# ---------------------------------------------------------------------------------------------- D. top-k across batches

def _exclusions_csr(rows, cols, full, short, rng):
    """rows x cols exclusions: rows `full` exclude every item (shuffled, with repeats), rows `short` all but five, the rest 0-40
    random items with repeats"""
    deg = rng.randint(0, 41, rows)
    deg[full] = cols + 3
    deg[short] = cols - 5
    parts = []
    for u in range(rows):
        if u in full:
            parts.append(np.concatenate([rng.permutation(cols), [0, cols - 1, 7]]))
        elif u in short:
            parts.append(rng.permutation(cols)[: cols - 5])
        else:
            lst = rng.randint(0, cols, deg[u] - deg[u] // 3)
            parts.append(np.concatenate([lst, lst[: deg[u] // 3]]))
    return _csr(rows, cols, np.arange(rows), deg, np.concatenate(parts), rng)


def _rows_of(csr, ids):
    """the rows `ids` of a CSR as their own CSR"""
    lists = [(csr.indices[csr.indptr[u]:csr.indptr[u + 1]], csr.data[csr.indptr[u]:csr.indptr[u + 1]]) for u in ids]
    indptr = np.cumsum([0] + [len(i) for i, _ in lists])
    return HostCSR(indptr, np.concatenate([i for i, _ in lists]), np.concatenate([r for _, r in lists]), len(ids), csr.cols)


def _assert_same(got, want, what):
    (gi, gs), (wi, ws) = got, want
    assert np.array_equal(gi, wi), what
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), what


def test_topk_and_rank_metrics_across_workspace_batches():
    """A catalogue of 10^6 items, f = 16: topk.hip TopkRunner fits 2,080 users in a batch of top-k with exclusions and 1,056 in
    one of rank_metrics (the relevance bitmap besides), so 6,285 users are four top-k batches and six rank-metric batches, the
    last ones partial and not a multiple of 32 users.  Exclusions: two users exclude every item (one on each side of the first
    batch boundary), one all but five, the rest a few.  (a) the full run equals top-k on user subsets of one batch each;
    (b) a model made of sampled rows (both sides of every batch boundary included, exclusion rows sliced to match): top-k equals
    recommend bit for bit, and equals the full run's rows; (c) rank_metrics equals tests/rank_reference.py on the lists (a) and
    (b) pinned, within 1e-12."""
    rng = np.random.RandomState(6)
    cols, f, k = 1_000_000, 16, 10
    tb = topk_batch(1 << 30, cols, k, True)
    rb = topk_batch(1 << 30, cols, k, True, extra=4 * ((cols + 31) // 32) + 4)
    users = 3 * tb + 45
    assert tb == 2080 and rb == 1056 and topk_batch(users, cols, k, True) == tb
    assert -(-users // tb) == 4 and users % tb == 45 and -(-users // rb) == 6 and (users % rb) % 32 != 0
    P = (rng.randn(users, f) * 0.3).astype(np.float32)
    Q = (rng.randn(cols, f) * 0.3).astype(np.float32)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(cols) * 0.3).astype(np.float32)
    model = cu.Model(users, cols, f, 3.5, P, Q, ub, ib)
    full_rows, short_rows = [tb - 1, tb], [2 * tb + 1]
    ex_host = _exclusions_csr(users, cols, full_rows, short_rows, rng)
    ex = cu.DeviceCSR(ex_host)

    items, scores = model.topk(ex, k)
    assert (items[full_rows] == -1).all() and np.isnan(scores[full_rows]).all()
    assert (items[short_rows, :5] >= 0).all() and (items[short_rows, 5:] == -1).all()
    assert (items[np.setdiff1d(np.arange(users), full_rows + short_rows)] >= 0).all()
    # (a) subsets of 1,000 users in any order: one batch each
    perm = rng.permutation(users)
    for s in range(0, users, 1000):
        ids = perm[s:s + 1000].astype(np.int32)
        assert topk_batch(len(ids), cols, k, True) >= len(ids)
        _assert_same(model.topk(ex, k, users=ids), (items[ids], scores[ids]), "subset at %d" % s)
    # (b) sampled rows against recommend
    edges = [b + d for step in (tb, rb) for b in range(step, users, step) for d in (-1, 0)]
    ids = np.unique(np.concatenate([[0, users - 1], edges, full_rows, short_rows, rng.choice(users, 20, replace=False)]))
    sub = cu.Model(len(ids), cols, f, 3.5, P[ids], Q, ub[ids], ib)
    sub_ex = cu.DeviceCSR(_rows_of(ex_host, ids))
    want = sub.recommend(sub_ex, k)
    _assert_same(sub.topk(sub_ex, k), want, "sampled rows against recommend")
    _assert_same((items[ids], scores[ids]), want, "full run against recommend")
    # (c) rank metrics: relevant items from the user's own list, from anywhere, past the catalogue; every 7th user none
    deg = rng.randint(1, 9, users)
    deg[::7] = 0
    rel = []
    for u in range(users):
        picks = rng.randint(0, cols, deg[u])
        listed = items[u][items[u] >= 0]
        if len(listed) and deg[u] > 1:
            picks[: deg[u] // 2] = rng.choice(listed, deg[u] // 2)
        rel.append(picks)
    rel = np.concatenate(rel)
    # (a few items past the catalogue: never listed, they still count in |R_u|)
    test = _csr(users, cols + 10, np.arange(users), deg, np.where(rng.rand(len(rel)) < 0.02, cols + 3, rel), rng)
    want, want_per = rr.rank_metrics(items, test, k)
    got, per = model.rank_metrics(cu.DeviceCSR(test), k, exclude=ex, per_user=True)
    np.testing.assert_allclose(per, want_per, rtol=1e-12, atol=0)
    assert np.array_equal(np.isnan(per), np.isnan(want_per))
    assert want["users_evaluated"] > 0 and want["precision"] > 0
    for name in ("users_evaluated", "users_skipped", "k"):
        assert got[name] == want[name], name
    for name in ("precision", "recall", "ndcg", "map", "hit_rate"):
        assert abs(got[name] - want[name]) <= 1e-12, (name, got[name], want[name])
