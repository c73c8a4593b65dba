"""Neighbour queries on the device (-m gpu): cu2rec_model_similar (DOT) against cu2rec_model_topk of a companion model bit for bit,
COSINE against float64, cu2rec_model_top_users against a host selection over the columns of cu2rec_model_scores bit for bit (one
call and several workspace batches), the refusals, and bin/predict -S against Model.similar."""
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from conftest import ROOT
from cu2rec_amd import synth
from cu2rec_amd.api import HostCSR
import neighbors_reference as nr

pytestmark = pytest.mark.gpu


def _rows(n, f, rng, scale=0.3):
    """random rows without zeros: no product and no sum is -0.0 or exactly 0"""
    X = (rng.randn(n, f) * scale).astype(np.float32)
    X[X == 0] = np.float32(0.01)
    return X


def _lists(rows, cols, rng, per_row, full_row=None):
    """per-row id lists: unsorted, with repeats; row full_row (if any) names every id"""
    out = []
    for r in range(rows):
        if r == full_row:
            lst = rng.permutation(cols).tolist() + [0, cols - 1]
        else:
            lst = rng.randint(0, cols, rng.randint(per_row[0], per_row[1] + 1)).tolist() if cols else []
            lst += lst[: len(lst) // 3]
            rng.shuffle(lst)
        out.append(lst)
    return out


def _csr(lists, cols):
    indptr = np.cumsum([0] + [len(l) for l in lists])
    flat = [i for l in lists for i in l]
    return HostCSR(indptr, flat, np.full(len(flat), 4.0, np.float32), len(lists), cols)


def _assert_same(got, want):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape
    np.testing.assert_array_equal(gi, wi)
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))


def _side_model(side, X, other, f, rng):
    """a model whose `side` matrix is X; the other side random, biases random (they must not enter the neighbour scores)"""
    n = len(X)
    O = _rows(other, f, rng)
    if side == "users":
        return cu.Model(n, other, f, 3.5, X, O, rng.randn(n).astype(np.float32), rng.randn(other).astype(np.float32))
    return cu.Model(other, n, f, 3.5, O, X, rng.randn(other).astype(np.float32), rng.randn(n).astype(np.float32))


# (rows of the side, rows of the other side, f, k): every listed f, row count at the tile edges and k appears at least once
CASES = [(1, 3, 1, 1), (31, 5, 4, 10), (33, 2, 31, 100), (65, 7, 100, 256), (127, 3, 128, 10), (129, 4, 252, 256),
         (1000, 2, 253, 100), (26744, 2, 100, 10), (65, 3, 300, 100), (1000, 5, 300, 256), (129, 2, 31, 1), (33, 9, 128, 256)]


@pytest.mark.parametrize("side", ["items", "users"])
@pytest.mark.parametrize("n,other,f,k", CASES)
def test_similar_dot_equals_topk_of_the_companion_model(side, n, other, f, k):
    rng = np.random.RandomState(n * 3 + f + (side == "users"))
    X = _rows(n, f, rng)
    model = _side_model(side, X, other, f, rng)
    ex_lists = _lists(max(n - 1, 1), n, rng, (0, min(n, 60)), full_row=1 if n > 2 else None)
    ex = _csr(ex_lists, n)
    # the companion: P = Q = X, zero biases, gb = 0; the exclusion adds the diagonal
    with_self = [l + [a] for a, l in enumerate(ex_lists + [[] for _ in range(n - len(ex_lists))])]
    companion = cu.Model(n, n, f, 0.0, X, X, np.zeros(n, np.float32), np.zeros(n, np.float32))
    want = companion.topk(cu.DeviceCSR(_csr(with_self, n)), k)
    d_ex = cu.DeviceCSR(ex)
    got = model.similar(None, k, side=side, metric="dot", exclude=d_ex)
    _assert_same(got, want)
    if n > 2:
        assert (got[0][1] == -1).all() and np.isnan(got[1][1]).all()  # every candidate excluded
    assert not (got[0] == np.arange(n)[:, None]).any()
    # a subset of ids in any order, with duplicates
    ids = np.concatenate([rng.randint(0, n, 20), [n - 1, 0, n - 1]]).astype(np.int32)
    _assert_same(model.similar(ids, k, side=side, metric="dot", exclude=d_ex), (want[0][ids], want[1][ids]))
    # no exclusion at all: the companion with the diagonal only
    want0 = companion.topk(cu.DeviceCSR(_csr([[a] for a in range(n)], n)), k)
    _assert_same(model.similar(None, k, side=side, metric="dot"), want0)


def _check_cosine(model, X, side, k, exclude_lists=None, ids=None):
    n = len(X)
    d_ex = cu.DeviceCSR(_csr(exclude_lists, n)) if exclude_lists is not None else None
    got_i, got_s = model.similar(ids, k, side=side, metric="cosine", exclude=d_ex)
    q = np.arange(n) if ids is None else np.asarray(ids)
    cos = nr.cosine64(X, q)
    for row, a in enumerate(q):
        excl = set(exclude_lists[a]) if exclude_lists is not None and a < len(exclude_lists) else set()
        excl.add(int(a))
        listed = got_i[row][got_i[row] >= 0]
        m = len(listed)
        assert (got_i[row][m:] == -1).all() and np.isnan(got_s[row][m:]).all()
        assert int(a) not in listed.tolist()
        assert not (set(listed.tolist()) & excl)
        assert len(set(listed.tolist())) == m
        sc = got_s[row][:m].astype(np.float64)
        np.testing.assert_allclose(sc, cos[row, listed], rtol=0, atol=1e-5)
        assert (np.diff(sc) <= 0).all()
        same = sc[1:] == sc[:-1]
        assert (listed[1:][same] > listed[:-1][same]).all()
        free = np.ones(n, bool)
        free[list(excl)] = False
        free[listed] = False
        available = n - len(excl)
        assert m == min(k, available)
        if m == k and free.any():  # completeness: nothing left out beats the k-th listed score
            assert cos[row, free].max() <= sc[-1] + 1e-5
    return got_i, got_s


@pytest.mark.parametrize("side", ["items", "users"])
@pytest.mark.parametrize("n,f,k", [(1, 4, 1), (33, 1, 10), (129, 100, 10), (1000, 31, 100), (1000, 300, 256), (65, 253, 256)])
def test_similar_cosine_against_float64(side, n, f, k):
    rng = np.random.RandomState(n + f + 7 * (side == "users"))
    X = _rows(n, f, rng)
    model = _side_model(side, X, 3, f, rng)
    _check_cosine(model, X, side, k)
    lists = _lists(n, n, rng, (0, min(n, 40)), full_row=0 if n > 1 else None)
    got_i, _ = _check_cosine(model, X, side, k, exclude_lists=lists)
    if n > 1:
        assert (got_i[0] == -1).all()
    ids = rng.randint(0, n, 50).astype(np.int32)
    _check_cosine(model, X, side, k, exclude_lists=lists, ids=ids)


def test_similar_cosine_zero_rows_score_zero():
    rng = np.random.RandomState(5)
    n, f, k = 200, 24, 250
    X = _rows(n, f, rng)
    zero = [0, 17, 131, 199]
    X[zero] = 0.0
    model = _side_model("items", X, 4, f, rng)
    got_i, got_s = _check_cosine(model, X, "items", k)
    for z in zero:  # as query: every other row, all scores 0 (+0.0 or -0.0)
        assert (got_s[z][: n - 1] == 0).all() and sorted(got_i[z][: n - 1].tolist()) == [i for i in range(n) if i != z]
    for a in range(n):  # as candidate: listed with score 0
        row = dict(zip(got_i[a].tolist(), got_s[a].tolist()))
        for z in zero:
            if z != a:
                assert row[z] == 0.0
    # duplicated rows: cosine 1 (within float rounding), and the query is still never its own neighbour
    Y = X.copy()
    Y[50] = Y[60] = Y[70]
    m2 = _side_model("users", Y, 4, f, rng)
    gi, gs = _check_cosine(m2, Y, "users", 5, ids=[50, 50, 60])
    assert gi[0][0] in (60, 70) and abs(gs[0][0] - 1.0) <= 1e-6


def _users_exclusion(users, items, rng, per_row):
    """user-major exclusions (unsorted rows with repeats; every user names item 0) and the item-major transpose"""
    lists = _lists(users, items, rng, per_row)
    for l in lists:
        l.insert(rng.randint(len(l) + 1), 0)
    host = _csr(lists, items)
    return host, host.transpose()


def _host_top_users(scores, ex_t, k, items):
    excl = nr.excluded_sets(ex_t, scores.shape[1])
    out_i = np.empty((len(items), k), np.int32)
    out_s = np.empty((len(items), k), np.float32)
    for row, i in enumerate(items):
        allowed = np.ones(scores.shape[0], bool)
        allowed[list(excl[i])] = False
        out_i[row], out_s[row] = nr.select(scores[:, i], allowed, k)
    return out_i, out_s


# (users, items, f, k)
USER_CASES = [(1, 3, 1, 1), (31, 129, 4, 10), (33, 65, 31, 100), (65, 33, 100, 256), (127, 31, 128, 10), (129, 7, 252, 256),
              (1000, 40, 253, 100), (26744, 5, 300, 10), (26744, 33, 100, 256), (1000, 129, 300, 1)]


@pytest.mark.parametrize("users,items,f,k", USER_CASES)
def test_top_users_equals_a_selection_over_the_score_columns(users, items, f, k):
    rng = np.random.RandomState(users + items * 3 + f)
    P, Q = _rows(users, f, rng), _rows(items, f, rng)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(items) * 0.3).astype(np.float32)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    scores = model.scores()
    every = np.arange(items)
    _assert_same(model.top_users(None, k), _host_top_users(scores, HostCSR(np.zeros(1), [], [], 0, users), k, every))
    _, ex_t = _users_exclusion(users, items, rng, (0, min(items, 30)))
    want = _host_top_users(scores, ex_t, k, every)
    d_ex = cu.DeviceCSR(ex_t)
    got = model.top_users(d_ex, k)
    _assert_same(got, want)
    assert (got[0][0] == -1).all() and np.isnan(got[1][0]).all()  # item 0 excludes every user
    ids = np.concatenate([rng.randint(0, items, 15), [items - 1, 0, items - 1]]).astype(np.int32)
    _assert_same(model.top_users(d_ex, k, items=ids), (want[0][ids], want[1][ids]))


def test_top_users_ties_by_ascending_user():
    rng = np.random.RandomState(2)
    users, items, f, k = 300, 20, 16, 128
    P, Q = _rows(users, f, rng), _rows(items, f, rng)
    ub = (rng.randn(users) * 0.3).astype(np.float32)
    for src in rng.choice(users, 40, replace=False):
        for dst in rng.choice(users, 2, replace=False):
            P[dst], ub[dst] = P[src], ub[src]
    model = cu.Model(users, items, f, 3.5, P, Q, ub, (rng.randn(items) * 0.3).astype(np.float32))
    got = model.top_users(None, k)
    _assert_same(got, _host_top_users(model.scores(), HostCSR(np.zeros(1), [], [], 0, users), k, np.arange(items)))
    gi, gs = got
    same = gs[:, 1:] == gs[:, :-1]
    assert same.any() and (gi[:, 1:][same] > gi[:, :-1][same]).all()


def test_top_users_over_several_workspace_batches():
    """150,000 users x 20,000 items with a 20 M-entry exclusion: the per-item bitmap (4,688 words) makes several batches."""
    users, items, f, k = 150_000, 20_000, 8, 10
    rng = np.random.RandomState(11)
    nnz = 20_000_000
    row_of = np.sort(rng.randint(0, users, nnz))
    indptr = np.zeros(users + 1, np.int64)
    np.cumsum(np.bincount(row_of, minlength=users), out=indptr[1:])
    host = HostCSR(indptr, rng.randint(0, items, nnz), np.ones(nnz, np.float32), users, items)
    ex_t = host.transpose()
    P, Q = _rows(users, f, rng), _rows(items, f, rng)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(items) * 0.3).astype(np.float32)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    d_ex = cu.DeviceCSR(ex_t)
    whole = model.top_users(d_ex, k)
    for part in (np.arange(0, 7000), np.arange(7000, items), rng.permutation(items)[:3000]):
        _assert_same(model.top_users(d_ex, k, items=part.astype(np.int32)), (whole[0][part], whole[1][part]))
    sample = rng.choice(items, 256, replace=False)
    s64 = (np.float64(np.float32(3.5)) + ub.astype(np.float64)[:, None] + ib.astype(np.float64)[None, sample]
           + P.astype(np.float64) @ Q[sample].astype(np.float64).T)
    for col, i in enumerate(sample):
        listed = whole[0][i]
        assert (listed >= 0).all()
        np.testing.assert_allclose(whole[1][i], s64[listed, col], rtol=0, atol=1e-5)
        excl = ex_t.indices[ex_t.indptr[i]:ex_t.indptr[i + 1]]
        assert not np.isin(listed, excl).any()
        free = np.ones(users, bool)
        free[excl] = False
        free[listed] = False
        assert s64[free, col].max() <= float(whole[1][i][-1]) + 1e-5


def test_neighbor_queries_refuse_bad_arguments():
    rng = np.random.RandomState(1)
    users, items, f = 6, 10, 8
    model = cu.Model(users, items, f, 3.0, _rows(users, f, rng), _rows(items, f, rng), np.zeros(users, np.float32),
                     np.zeros(items, np.float32))

    def status(fn, *a, **kw):
        with pytest.raises(cu.Cu2recError) as e:
            fn(*a, **kw)
        return e.value.status

    for k, st in ((0, -1), (257, -6), (1000, -6)):
        assert status(model.similar, None, k) == st
        assert status(model.top_users, None, k) == st
    for side, bad in (("items", items), ("users", users)):
        assert status(model.similar, [0, bad], 3, side=side) == -1
        assert status(model.similar, [-1], 3, side=side) == -1
    assert status(model.similar, None, 3, side=2) == -1
    assert status(model.similar, None, 3, side=-1) == -1
    assert status(model.similar, None, 3, metric=2) == -1
    assert status(model.top_users, None, 3, items=[items]) == -1
    assert status(model.top_users, None, 3, items=[-2]) == -1
    # exclusions that do not fit: too many rows, or an id past the candidates
    too_many = cu.DeviceCSR(HostCSR(np.zeros(items + 2), [], [], items + 1, items))
    past = cu.DeviceCSR(HostCSR([0, 1], [items - 1], [1.0], 1, items))
    assert status(model.similar, None, 3, side="users", exclude=past) == -1  # users side: ids below 6
    assert status(model.similar, None, 3, side="items", exclude=too_many) == -1
    assert status(model.top_users, too_many, 3) == -1
    assert status(model.top_users, past, 3) == -1  # row 0 names user 9
    # n = 0 is fine
    empty = np.zeros(0, np.int32)
    assert model.similar(empty, 3)[0].shape == (0, 3)
    assert model.top_users(None, 3, items=empty)[0].shape == (0, 3)
    # a fitting exclusion is accepted on each side
    model.similar(None, 3, side="users", exclude=cu.DeviceCSR(HostCSR([0, 2], [5, 5], [1.0, 1.0], 1, users)))
    model.top_users(cu.DeviceCSR(HostCSR([0, 1], [users - 1], [1.0], 1, users)), 3)


def test_predict_similar_lists_model_similar(tmp_path):
    tr, te = synth.make_ratings(300, 150, 9000, min_degree=3, seed=6, integer_ratings=True)
    f = 8
    cfg = cu.default_config(total_iterations=30, n_factors=f, check_error=30)
    _, Q, _, _, _ = cu.train(tr, te, cfg, mode="ordered", verbose=False)
    cu.writeCSV(str(tmp_path / "q.csv"), Q)
    Qf = cu.read_array(str(tmp_path / "q.csv"))
    (tmp_path / "c.cfg").write_text("0 30 %d 0.05 42 0.015 0.03 0.045 0.08\n" % f)
    ids = [3, 0, 149, 3, 77]
    (tmp_path / "ids.txt").write_text("".join("%d\n" % i for i in ids))
    predict = os.path.join(ROOT, "bin", "predict")
    model = cu.Model(1, Qf.shape[0], f, 0.0, np.zeros((1, f), np.float32), Qf, np.zeros(1, np.float32),
                     np.zeros(Qf.shape[0], np.float32))
    for k in (None, 4, 200):
        args = [predict, "-c", str(tmp_path / "c.cfg"), "-q", str(tmp_path / "q.csv"), "-S"] + (["-k", str(k)] if k else [])
        out = subprocess.run(args + [str(tmp_path / "ids.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr
        near, cos = model.similar(np.array(ids, np.int32), k or 10, side="items", metric="cosine")
        want = []
        for row, i in enumerate(ids):
            want += ["Item: %d" % i, "Similar items:"]
            want += ["Rank: %d\tItem: %d\tCosine similarity: %f" % (j + 1, near[row][j], cos[row][j])
                     for j in range(k or 10) if near[row][j] >= 0]
        assert out.stdout.split("\n") == want + [""]
