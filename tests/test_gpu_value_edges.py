"""The values themselves (-m gpu): NaN of either sign, infinities, signed zeros, rows far from unit magnitude and a diverged
training run, through every scoring, ranking and loss path.

Scores (cu2rec_model_scores) are classified (NaN, +inf, -inf, finite) against a float64 evaluation of the same expression;
topk, recommend, top_users and similar(dot) must be tests/neighbors_reference.select over the device's own score matrix (ids
exactly, scores bit for bit); rank_metrics is tests/rank_reference.py on the device's lists.  Cosine is held to float64
from 2^-149 to 2^126 row scales, is invariant under exact power-of-two scaling, and scores a row holding an inf or a NaN as
+NaN against everything.  A learning rate that overflows within a few iterations runs in serial, ordered and ping-pong mode
against the CPU oracle: classes equal, finite values bit for bit."""
import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import synth
from cu2rec_amd.api import HostCSR
from oracle import oracle as orc
import neighbors_reference as nr
import rank_reference as rr
from test_gpu_neighbors import _check_cosine, _csr, _side_model
from test_gpu_size_edges import topk_batch

pytestmark = pytest.mark.gpu

POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000  # quiet NaNs: the default of most hardware, and x86's default (sign set)


def _nan(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _cls(x, as_float32=True):
    """0 NaN, 1 +inf, 2 -inf, 3 finite (of the value rounded to float32, by default)"""
    x = np.asarray(x, np.float32 if as_float32 else np.float64)
    return np.where(np.isnan(x), 0, np.where(x == np.inf, 1, np.where(x == -np.inf, 2, 3)))


def _scores64(P, Q, ub, ib, gb):
    """((gb + ub) + ib) + p . q in float64 (then rounded to float32 for the class)"""
    with np.errstate(all="ignore"):
        P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
        dot = (P64[:, None, :] * Q64[None, :, :]).sum(axis=2)
        return ((np.float64(np.float32(gb)) + ub.astype(np.float64)[:, None]) + ib.astype(np.float64)[None, :]) + dot, \
            (np.abs(P64)[:, None, :] * np.abs(Q64)[None, :, :]).sum(axis=2)


def _base(n, f, rng):
    X = (rng.randn(n, f) * 0.3).astype(np.float32)
    X[X == 0] = np.float32(0.01)
    return X


def _poisoned(users, items, f, seed):
    """A model with non-finite and overflowing values in chosen rows.  Returns the arrays and the ids of the user / item rows
    that hold a sign-set NaN (whose output sign the test records)."""
    rng = np.random.RandomState(seed)
    P, Q = _base(users, f, rng), _base(items, f, rng)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(items) * 0.3).astype(np.float32)
    j = f // 2
    P[1, j] = _nan(NEG_NAN)          # -NaN factor
    P[2, j] = _nan(POS_NAN)          # +NaN factor
    ub[3] = _nan(NEG_NAN | 0x1234)   # -NaN bias with a payload
    ub[4] = _nan(POS_NAN)
    ub[5] = np.inf                   # +inf bias; against ib = -inf: NaN
    ub[6] = -np.inf
    P[7] = 1e20                      # p . q overflows against the 1e20 rows
    P[8, 0] = np.inf                 # inf factor; against a zero factor: 0 * inf = NaN
    Q[1, j] = _nan(NEG_NAN)
    ib[2] = _nan(NEG_NAN)
    ib[3] = -np.inf
    ib[4] = np.inf
    Q[5] = 1e20
    Q[6, 0] = 0.0
    Q[7] = -1e20
    ib[8] = _nan(POS_NAN | 0x77)
    return P, Q, ub, ib, {"users": [1, 3], "items": [1, 2]}


# (users, items, f): tile edges and both staging paths (whole rows up to 252 factors, chunks above)
SHAPES = [(33, 129, 4), (65, 31, 31), (31, 257, 100), (129, 65, 300)]


def _nan_signs(got, mask):
    vals = got[mask & np.isnan(got)]
    return sorted({"%08X" % b for b in vals.view(np.uint32).tolist()})


@pytest.mark.parametrize("users,items,f", SHAPES)
def test_scores_classes_against_float64(users, items, f):
    P, Q, ub, ib, neg = _poisoned(users, items, f, users + f)
    gb = 3.5
    model = cu.Model(users, items, f, gb, P, Q, ub, ib)
    got = model.scores()
    want, mag = _scores64(P, Q, ub, ib, gb)
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(_cls(got), _cls(want))
    fin = np.isfinite(got)
    special = np.zeros_like(fin)
    special[:9] = True
    special[:, :9] = True
    # untouched rows: the existing 1e-5 of tests/test_gpu_predict.py; rows with 1e20 factors: float32 accumulation error
    # (f + 3 roundings of at most 2^-24 of the sum of magnitudes)
    err = np.abs(got.astype(np.float64) - want)
    assert float(err[fin & ~special].max()) <= 1e-5
    bound = np.maximum(1e-5, 2.0 ** -24 * (f + 3) * (mag + abs(gb) + np.abs(ub)[:, None] + np.abs(ib)[None, :]))
    assert (err[fin] <= bound[fin]).all()
    # record what the hardware makes of a sign-set NaN operand (v_add_f32 / MFMA); canonical NaNs from inf - inf and 0 * inf
    from_neg = np.zeros_like(fin)
    from_neg[neg["users"]] = True
    from_neg[:, neg["items"]] = True
    generated = np.zeros_like(fin)
    generated[5, 3] = generated[6, 4] = generated[8, 6] = True
    print("scores NaN bits, users=%d items=%d f=%d: from -NaN operands %s; from inf - inf / 0 * inf %s; from +NaN operands %s"
          % (users, items, f, _nan_signs(got, from_neg), _nan_signs(got, generated),
             _nan_signs(got, np.isin(np.arange(users), [2, 4])[:, None] & ~from_neg)))


def _excl_lists(rows, cols, rng, per_row):
    return [rng.choice(cols, rng.randint(per_row[0], per_row[1] + 1), replace=False).tolist() for _ in range(rows)]


def _select_rows(S, lists, k, rows=None):
    rows = range(S.shape[0]) if rows is None else rows
    out_i = np.empty((len(rows), k), np.int32)
    out_s = np.empty((len(rows), k), np.float32)
    for n, r in enumerate(rows):
        allowed = np.ones(S.shape[1], bool)
        if lists is not None and r < len(lists):
            allowed[list(lists[r])] = False
        out_i[n], out_s[n] = nr.select(S[r], allowed, k)
    return out_i, out_s


def _assert_same(got, want, what):
    (gi, gs), (wi, ws) = got, want
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.uint32) != ws.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (what, "rows", bad[:10].tolist(), gi[bad[:1]], wi[bad[:1]])


@pytest.mark.parametrize("users,items,f", SHAPES)
def test_topk_recommend_top_users_are_selections_of_the_scores(users, items, f):
    P, Q, ub, ib, _ = _poisoned(users, items, f, users * 7 + f)
    rng = np.random.RandomState(users + items)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    S = model.scores()
    lists = _excl_lists(users, items, rng, (0, min(items, 12)))
    d_ex = cu.DeviceCSR(_csr(lists, items))
    for k in (1, 7, min(items + 3, 256)):
        want = _select_rows(S, lists, k)
        _assert_same(model.topk(d_ex, k), want, "topk k=%d" % k)
        _assert_same(model.recommend(d_ex, k), want, "recommend k=%d" % k)
        _assert_same(model.topk(None, k), _select_rows(S, None, k), "topk unexcluded k=%d" % k)
        t_lists = _excl_lists(items, users, rng, (0, min(users, 12)))
        got = model.top_users(cu.DeviceCSR(_csr(t_lists, users)), k)
        _assert_same(got, _select_rows(np.ascontiguousarray(S.T), t_lists, k), "top_users k=%d" % k)


def test_recommend_leaves_no_hole_before_negative_nans():
    """m listable items, r rated ones and the rest -NaN, with m + r < k: recommend and topk list the m items, then padding --
    wherever the hardware keeps the NaN's sign.  Users whose every candidate is NaN (either sign), +inf or -inf as well."""
    users, items, f, k = 40, 96, 8, 64
    rng = np.random.RandomState(17)
    P, Q = _base(users, f, rng), _base(items, f, rng)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(items) * 0.3).astype(np.float32)
    neg_items = rng.choice(items, 70, replace=False)
    ib[neg_items] = _nan(NEG_NAN)
    ib[neg_items[:5]] = _nan(NEG_NAN | 0x3FFFFF)  # other payloads
    ub[0] = _nan(NEG_NAN)                          # every candidate: NaN from a -NaN bias
    P[1, 3] = _nan(NEG_NAN)                        # ... from a -NaN factor
    ub[2] = _nan(POS_NAN)                          # ... from a +NaN bias
    ub[3], ub[4] = np.inf, -np.inf                 # every candidate +inf (but the -NaN items), every one -inf
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    S = model.scores()
    lists = _excl_lists(users, items, rng, (2, 10))
    d_ex = cu.DeviceCSR(_csr(lists, items))
    want = _select_rows(S, lists, k)
    got_r, got_t = model.recommend(d_ex, k), model.topk(d_ex, k)
    print("recommend hole: NaN bits of a -NaN item bias in the scores: %s; of a -NaN factor: %s"
          % (_nan_signs(S, np.isin(np.arange(items), neg_items)[None, :] & (np.arange(users) > 4)[:, None]),
             _nan_signs(S[1:2], np.ones((1, items), bool))))
    _assert_same(got_t, want, "topk")
    _assert_same(got_r, want, "recommend")
    for gi, gs in (got_r, got_t):  # padding only at the end
        m = (gi >= 0).sum(axis=1)
        assert all((gi[u, :m[u]] >= 0).all() and (gi[u, m[u]:] == -1).all() and np.isnan(gs[u, m[u]:]).all()
                   for u in range(users))
    assert np.isnan(want[1][4][want[0][4] >= 0]).all()  # -inf is never listed: user 4 lists NaNs at most
    assert ((want[1][3] == np.inf) | np.isnan(want[1][3])).all()
    assert (want[0][3] >= 0).sum() >= items - len(neg_items) - len(lists[3])  # +inf on every finite-bias item not rated


def test_topk_with_non_finite_rows_across_workspace_batches():
    """Two workspace batches of top-k (tests/test_gpu_size_edges.py: topk_batch) with poisoned users on both sides of the boundary
    and in the partial last batch: rows sampled around the boundary equal the selection over the device's scores."""
    items, f, k = 40, 4, 10
    tb = topk_batch(1 << 30, items, k, True)
    users = tb + 45
    assert topk_batch(users, items, k, True) == tb and -(-users // tb) == 2
    rng = np.random.RandomState(23)
    P, Q = _base(users, f, rng), _base(items, f, rng)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(items) * 0.3).astype(np.float32)
    poison = np.array([tb - 2, tb - 1, tb, tb + 1, users - 1, 0] + rng.choice(users, 200, replace=False).tolist())
    kinds = np.arange(len(poison)) % 4
    ub[poison[kinds == 0]] = _nan(NEG_NAN)
    ub[poison[kinds == 1]] = _nan(POS_NAN)
    ub[poison[kinds == 2]] = -np.inf
    P[poison[kinds == 3], 1] = np.inf
    ib[[3, 17]] = _nan(NEG_NAN)
    ib[5] = np.inf
    Q[9, 1] = 0.0
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    lists = [rng.choice(items, rng.randint(0, 6), replace=False).tolist() for _ in range(users)]
    rows = np.unique(np.concatenate([np.arange(tb - 40, tb + 40), np.arange(users - 40, users), poison]))
    sub = cu.Model(len(rows), items, f, 3.5, P[rows], Q, ub[rows], ib)
    S = sub.scores()
    got_i, got_s = model.topk(cu.DeviceCSR(_csr(lists, items)), k)
    want = _select_rows(S, [lists[r] for r in rows], k)
    _assert_same((got_i[rows], got_s[rows]), want, "topk across batches")


@pytest.mark.parametrize("n,f,k", [(33, 4, 10), (129, 100, 40), (65, 300, 64)])
def test_similar_dot_is_a_selection_of_the_dot_products(n, f, k):
    rng = np.random.RandomState(n + f)
    X = _base(n, f, rng)
    X[1, 2] = _nan(NEG_NAN)
    X[2, 0] = _nan(POS_NAN)
    X[3, 0] = np.inf
    X[4, 0] = 0.0            # 0 * inf against row 3
    X[5] = 1e20              # overflows against itself (never a candidate of itself) and rows 6, 7
    X[6] = 3e19
    X[7] = -2e19
    X[8, 1] = -np.inf
    model = _side_model("items", X, 3, f, rng)
    companion = cu.Model(n, n, f, 0.0, X, X, np.zeros(n, np.float32), np.zeros(n, np.float32))
    D = companion.scores()  # 0 + x . y: the same floats but for -0.0 (none here: no row has a zero dot)
    want64, _ = _scores64(X, X, np.zeros(n, np.float32), np.zeros(n, np.float32), 0.0)
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(_cls(D), _cls(want64))
    lists = _excl_lists(n, n, rng, (0, 5))
    got = model.similar(None, k, side="items", metric="dot", exclude=cu.DeviceCSR(_csr(lists, n)))
    self_lists = [l + [a] for a, l in enumerate(lists)]
    _assert_same(got, _select_rows(D, self_lists, k), "similar dot")
    assert _cls(D[5, 6]) == 1 and _cls(D[5, 7]) == 2 and _cls(D[6, 7]) == 2  # products past FLT_MAX
    print("similar(dot) NaN bits from a -NaN element: %s" % _nan_signs(got[1][1:2], np.ones((1, k), bool)))


def test_rank_metrics_of_a_poisoned_model_match_the_reference():
    users, items, f, k = 65, 129, 31, 10
    P, Q, ub, ib, _ = _poisoned(users, items, f, 5)
    rng = np.random.RandomState(8)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    ex = _csr(_excl_lists(users, items, rng, (0, 8)), items)
    items_l, _ = model.topk(cu.DeviceCSR(ex), k)
    rel = [rng.choice(items, rng.randint(0, 12), replace=False).tolist() for _ in range(users)]
    for u in range(users):
        if rel[u] and (items_l[u] >= 0).any():
            rel[u][0] = int(items_l[u][0])
    test = HostCSR(np.cumsum([0] + [len(r) for r in rel]), [i for r in rel for i in r],
                   rng.randint(1, 11, sum(len(r) for r in rel)).astype(np.float32) / 2, users, items)
    for thr in (None, 3.0):
        want, want_per = rr.rank_metrics(items_l, test, k, threshold=thr)
        got, per = model.rank_metrics(cu.DeviceCSR(test), k, exclude=cu.DeviceCSR(ex), threshold=thr, per_user=True)
        np.testing.assert_allclose(per, want_per, rtol=1e-12, atol=0)
        assert np.array_equal(np.isnan(per), np.isnan(want_per))
        for name in ("precision", "recall", "ndcg", "map", "hit_rate"):
            assert abs(got[name] - want[name]) <= 1e-12, name


# ------------------------------------------------------------------------------------------------- cosine across magnitudes

EXPONENTS = [-149, -130, -100, -70, -64, -20, 0, 20, 60, 64, 100, 126]


def _unit_base(n, f, rng):
    """rows of moderate elements, |x| in [1e-3, 1.9]: every scale 2^e of EXPONENTS stays below FLT_MAX"""
    X = rng.randn(n, f) * 0.5
    X = np.sign(X) * np.clip(np.abs(X), 1e-3, 1.9)
    return X.astype(np.float32)


@pytest.mark.parametrize("f", [4, 100, 300])
@pytest.mark.parametrize("e", EXPONENTS + ["mixed"])
def test_similar_cosine_across_row_magnitudes(e, f):
    n, k = 65, 64
    rng = np.random.RandomState(f + (0 if e == "mixed" else 200 + e))
    X = _unit_base(n, f, rng)
    scales = rng.choice(EXPONENTS, n) if e == "mixed" else np.full(n, e)
    Xs = (X.astype(np.float64) * np.exp2(scales.astype(np.float64))[:, None]).astype(np.float32)
    assert np.isfinite(Xs).all()
    if e == "mixed":
        Xs[[10, 40]] = 0.0  # zero rows keep cosine 0
    for side in ("items", "users"):
        model = _side_model(side, Xs, 3, f, rng)
        _check_cosine(model, Xs, side, k)


@pytest.mark.parametrize("f", [4, 100, 300])
def test_similar_cosine_is_invariant_under_exact_power_of_two_scaling(f):
    """Rows scaled by 2^e (exactly, in float) have the same unit rows, so the same lists bit for bit."""
    n, k = 129, 40
    rng = np.random.RandomState(f)
    X = _unit_base(n, f, rng)
    exact = [-100, -70, -64, -20, 0, 20, 60, 64, 100]
    scales = rng.choice(exact, n).astype(np.float64)
    Xs = (X.astype(np.float64) * np.exp2(scales)[:, None]).astype(np.float32)
    assert np.array_equal(Xs.astype(np.float64) * np.exp2(-scales)[:, None], X.astype(np.float64))
    a = _side_model("users", X, 3, f, rng).similar(None, k, side="users", metric="cosine")
    b = _side_model("users", Xs, 3, f, rng).similar(None, k, side="users", metric="cosine")
    _assert_same(b, a, "scaled rows")


@pytest.mark.parametrize("f", [4, 100, 300])
def test_similar_cosine_of_rows_with_inf_or_nan_is_positive_nan(f):
    n, k = 70, 69
    rng = np.random.RandomState(f + 1)
    X = _unit_base(n, f, rng)
    bad = [3, 31, 32, 50, 69]
    X[3, f - 1] = np.inf
    X[31, 0] = -np.inf
    X[32, f // 2] = _nan(NEG_NAN)
    X[50, 0] = _nan(POS_NAN)
    X[69] = np.inf
    X[12] = 0.0
    good = [i for i in range(n) if i not in bad]
    for side in ("items", "users"):
        model = _side_model(side, X, 3, f, rng)
        gi, gs = model.similar(None, k, side=side, metric="cosine")
        for a in range(n):
            others = [i for i in range(n) if i != a]
            if a in bad:  # as query: every other row, all +NaN, ascending id
                np.testing.assert_array_equal(gi[a], others)
                assert (gs[a].view(np.uint32) == POS_NAN).all()
            else:  # as candidate: first, ascending id, +NaN
                nb = len(bad)
                np.testing.assert_array_equal(gi[a][:nb], bad)
                assert (gs[a][:nb].view(np.uint32) == POS_NAN).all()
        # the rest of a good row's list is its list with the bad rows excluded, which is right against float64
        ex_lists = [list(bad) for _ in range(n)]
        wi, ws = _check_cosine(model, X, side, k, exclude_lists=ex_lists, ids=good)
        np.testing.assert_array_equal(gi[good][:, len(bad):], wi[:, :k - len(bad)])
        assert np.array_equal(gs[good][:, len(bad):].view(np.uint32), ws[:, :k - len(bad)].view(np.uint32))
        assert (gs[12][len(bad):] == 0).all()


# --------------------------------------------------------------------------------------------------------- a diverged run

DIVERGE_LR = 0.8  # this set's oracle run: every value finite through iteration 3; inf and NaN at 4; nearly all NaN by 6
# (ping-pong, whose item updates read the previous iteration's Q, overflows later: inf at 10, all three classes at 12)
SPANS = {"serial": (3, 4, 5, 6), "ordered": (3, 4, 5, 6), "pingpong": (6, 10, 11, 12)}
HYPER = (DIVERGE_LR, 0.02, 0.03, 0.04, 0.05)


def _diverge_set():
    return synth.make_ratings(300, 80, 6000, min_degree=3, seed=9)


def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


def _assert_classes_and_bits(got, want, what):
    for name, g, w in zip(("P", "Q", "user_bias", "item_bias"), got, want):
        np.testing.assert_array_equal(_cls(g), _cls(w), err_msg="%s %s classes" % (what, name))
        fin = np.isfinite(w)
        assert np.array_equal(g[fin].view(np.uint32), w[fin].view(np.uint32)), "%s %s finite values" % (what, name)


def _oracle_state(tr, f, iters, mode):
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    if mode == "pingpong":
        Qt, ibt = Q.copy(), ib.copy()
        orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, HYPER, 42, 0, iters,
                                    dot_order=orc.DOT_TREE16)
    else:
        orc.sgd_iterations(_as_orc(tr), P, Q, ub, ib, tr.global_bias, HYPER, 42, 0, iters, dot_order=orc.DOT_TREE16)
    return P, Q, ub, ib


@pytest.mark.parametrize("mode", ["serial", "ordered", "pingpong"])
def test_diverging_sgd_matches_the_oracle_class_by_class(mode):
    tr, te = _diverge_set()
    f = 16
    d_tr, d_te = cu.DeviceCSR(tr), cu.DeviceCSR(te)
    seen = set()
    for iters in SPANS[mode]:
        want = _oracle_state(tr, f, iters, mode)
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(d_tr, HYPER, 42, 0, iters, mode=mode)
        got = model.download()
        _assert_classes_and_bits(got, want, "%s after %d iterations" % (mode, iters))
        allv = np.concatenate([a.ravel() for a in want])
        seen.update(np.unique(_cls(allv)).tolist())
        lg = model.loss(d_te)
        lw = orc.loss(_as_orc(te), *want, tr.global_bias, dot_order=orc.DOT_TREE16)
        for key in ("rmse", "mae", "sum_sq", "sum_abs"):
            assert _cls(lg[key], False) == _cls(lw[key], False), (key, lg, lw)
        if np.isfinite(lw["rmse"]):
            assert lg["rmse"] == lw["rmse"] and lg["mae"] == lw["mae"]
            assert abs(lg["sum_sq"] - lw["sum_sq"]) <= 1e-12 * lw["sum_sq"]
        if iters == SPANS[mode][-1]:  # the diverged model still ranks by the selection rules
            S = model.scores()
            lists = [tr.indices[tr.indptr[u]:tr.indptr[u + 1]].tolist() for u in range(tr.rows)]
            want_l = _select_rows(S, lists, 20)
            _assert_same(model.topk(d_tr, 20), want_l, "topk of the diverged model")
            _assert_same(model.recommend(d_tr, 20), want_l, "recommend of the diverged model")
    assert {0, 3} <= seen, seen  # the span crosses from finite to NaN


def test_loss_of_residuals_whose_squares_overflow_float():
    tr, te = _diverge_set()
    f = 8
    rng = np.random.RandomState(4)
    P, Q = _base(tr.rows, f, rng), _base(tr.cols, f, rng)
    ub, ib = (rng.randn(tr.rows) * 0.3).astype(np.float32), (rng.randn(tr.cols) * 0.3).astype(np.float32)
    ib[[0, 7, 11]] = np.float32(1e30)  # e^2 = 1e60: past float, well inside double
    ib[12] = np.float32(-3e29)
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias, P, Q, ub, ib)
    got = model.loss(cu.DeviceCSR(te))
    want = orc.loss(_as_orc(te), P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_TREE16)
    assert np.isfinite(want["sum_sq"]) and want["sum_sq"] > 1e59
    for key in ("rmse", "mae", "sum_sq", "sum_abs"):
        assert _cls(got[key], False) == _cls(want[key], False), (key, got, want)
    assert abs(got["sum_sq"] - want["sum_sq"]) <= 1e-12 * want["sum_sq"]
    assert abs(got["sum_abs"] - want["sum_abs"]) <= 1e-12 * want["sum_abs"]
    assert got["rmse"] == want["rmse"] and got["mae"] == want["mae"]


def test_train_through_divergence_matches_the_oracle():
    """train() in ordered mode: the logged test RMSE has the oracle's class at every check and its value where finite; lr
    matches exactly.  Once the RMSE is NaN, `last < current` is false on both sides: patience never runs out again and lr
    stays where it was."""
    tr, te = _diverge_set()
    f, total = 16, 12
    kw = dict(total_iterations=total, n_factors=f, check_error=1, learning_rate=DIVERGE_LR, patience=1.0,
              learning_rate_decay=0.5, P_reg=0.02, Q_reg=0.03, user_bias_reg=0.04, item_bias_reg=0.05)
    cfg, ocfg = cu.default_config(**kw), orc.default_config(**kw)
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    log = orc.train(_as_orc(tr), _as_orc(te), ocfg, P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_TREE16, acc=orc.ACC_F64,
                    schedule=orc.SCHED_PATIENCE)
    gP, gQ, losses, gub, gib = cu.train(tr, te, cfg, mode="ordered", verbose=False)
    rmse = np.array([e["test_rmse"] for e in log], np.float32)
    assert np.isfinite(rmse[0]) and np.isnan(rmse[-1]), rmse  # the run diverges inside the span
    for e in log:
        g = losses[e["iteration"] - 1]
        assert _cls(g) == _cls(e["test_rmse"]), (e, g)
        if np.isfinite(e["test_rmse"]):
            assert g == e["test_rmse"]
    assert cfg.learning_rate == ocfg.learning_rate
    first_nan = int(np.argmax(np.isnan(rmse)))
    lrs = [e["lr"] for e in log]
    assert len(set(lrs[first_nan:])) == 1, lrs  # NaN < NaN is false: no decay after the divergence
    _assert_classes_and_bits((gP, gQ, gub, gib), (P, Q, ub, ib), "train")
