"""Scoring and ranking on the device (-m gpu): cu2rec_model_scores / cu2rec_model_recommend and bin/predict -u against
the oracle's prediction (predict.cu:17-30 restated in oracle/cu2rec_oracle.c: orc_predict) and a host sort
(predict.cu:49-65).  The dense product associates the sum over the factors differently from the reference's sequential
loop: scores agree within 1e-5 (values are O(1..5)), rankings agree wherever neighbouring scores are further apart."""
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import synth
from conftest import ROOT
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _oracle_scores(P, Q, ub, ib, gb):
    f = P.shape[1]
    fp = orc.C.POINTER(orc.C.c_float)
    out = np.empty((P.shape[0], Q.shape[0]), np.float32)
    for u in range(P.shape[0]):
        for i in range(Q.shape[0]):
            out[u, i] = orc.lib().orc_predict(f, P[u].ctypes.data_as(fp), Q[i].ctypes.data_as(fp), float(ub[u]), float(ib[i]),
                                              gb, orc.DOT_SEQ)
    return out


@pytest.mark.parametrize("users,items,f", [(1, 5, 4), (33, 100, 10), (70, 300, 100), (40, 257, 128), (17, 64, 200)])
def test_scores_match_oracle_prediction(users, items, f):
    rng = np.random.RandomState(users + f)
    P, Q = (rng.randn(users, f) * 0.3).astype(np.float32), (rng.randn(items, f) * 0.3).astype(np.float32)
    ub, ib = (rng.randn(users) * 0.3).astype(np.float32), (rng.randn(items) * 0.3).astype(np.float32)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    got = model.scores()
    want = _oracle_scores(P, Q, ub, ib, 3.5)
    assert float(np.abs(got - want).max()) <= 1e-5


def test_recommend_is_the_sorted_unrated_items():
    tr, _ = synth.make_ratings(90, 400, 6000, min_degree=3, seed=12)
    f = 50
    rng = np.random.RandomState(5)
    P, Q = (rng.randn(tr.rows, f) * 0.3).astype(np.float32), (rng.randn(tr.cols, f) * 0.3).astype(np.float32)
    ub, ib = (rng.randn(tr.rows) * 0.3).astype(np.float32), (rng.randn(tr.cols) * 0.3).astype(np.float32)
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias, P, Q, ub, ib)
    scores = model.scores()
    for k in (1, 10, tr.cols):
        items, top = model.recommend(cu.DeviceCSR(tr), k)
        for u in range(tr.rows):
            rated = set(tr.indices[tr.indptr[u]:tr.indptr[u + 1]].tolist())
            cand = [(scores[u, i], i) for i in range(tr.cols) if i not in rated]
            cand.sort(key=lambda t: -t[0])
            n = min(k, len(cand))
            np.testing.assert_array_equal(top[u, :n], np.array([c[0] for c in cand[:n]], np.float32))  # the device's own scores, sorted
            for j in range(n):
                assert items[u, j] not in rated and scores[u, items[u, j]] == top[u, j]
            assert (items[u, n:] == -1).all() and np.isnan(top[u, n:]).all()
    items, top = model.recommend(None, 3)  # nothing excluded
    np.testing.assert_array_equal(top, -np.sort(-scores, axis=1)[:, :3])


def test_bin_predict_many_users_matches_oracle(tmp_path):
    """bin/predict -u on a file of three users (not sorted by user id): every distinct userId is a new user = one row of
    a fresh model (row u draws the sample stream of user u), all fitted in one batch with the item side frozen -- exactly
    the oracle's frozen-item SGD on the same rows -- then scored and ranked on the device: the printed recommendations
    are the oracle's predictions of the unrated items, best first."""
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    tr, te = synth.make_ratings(200, 40, 3000, min_degree=3, seed=2)
    synth.write_csv(str(tmp_path / "train.csv"), tr)
    synth.write_csv(str(tmp_path / "test.csv"), te)
    (tmp_path / "train.cfg").write_text("0 60 8 0.02 42 0.02 0.02 0.02 0.02\n")
    subprocess.run([mf, "-c", str(tmp_path / "train.cfg"), "-m", "ordered", str(tmp_path / "train.csv"), str(tmp_path / "test.csv")],
                   stdout=subprocess.PIPE, check=True)
    (tmp_path / "predict.cfg").write_text("0 150 8 0.05 42 0.02 0.02 0.02 0.02\n")
    model_args = ["-c", str(tmp_path / "predict.cfg"), "-i", str(tmp_path / "train_f8_item_bias.csv"), "-g",
                  str(tmp_path / "train_f8_global_bias.csv"), "-q", str(tmp_path / "train_f8_q.csv")]
    rng = np.random.RandomState(3)
    users = {7: rng.choice(40, 6, replace=False), 3: rng.choice(40, 4, replace=False), 12: rng.choice(40, 9, replace=False)}
    ratings = {uid: [(int(i), rng.randint(1, 11) / 2.0) for i in its] for uid, its in users.items()}
    lines = ["userId,itemId,rating"]
    for uid in (7, 3, 12):  # deliberately not sorted by user id
        lines += ["%d,%d,%.1f" % (uid, i + 1, r) for i, r in ratings[uid]]
    (tmp_path / "many.csv").write_text("\n".join(lines) + "\n")
    out = subprocess.run([predict] + model_args + ["-u", "-k", "5", str(tmp_path / "many.csv")], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    blocks = out.split("User: ")[1:]
    order = [3, 7, 12]
    assert [int(b.split("\n")[0]) for b in blocks] == order  # ascending user id
    # oracle: rows 0..2 = users 3, 7, 12, every row from the one-user seed-42 draw, 150 frozen-item iterations
    Q = cu.read_array(str(tmp_path / "train_f8_q.csv"))
    ib = cu.read_array(str(tmp_path / "train_f8_item_bias.csv")).ravel()
    gb = float(cu.read_array(str(tmp_path / "train_f8_global_bias.csv")).ravel()[0])
    indptr = np.cumsum([0] + [len(ratings[u]) for u in order]).astype(np.int32)
    indices = np.array([i for u in order for i, _ in ratings[u]], np.int32)
    data = np.array([r for u in order for _, r in ratings[u]], np.float32)
    P = np.tile(orc.normal_fill(8, 8), (3, 1))
    ub = np.tile(orc.normal_fill(1, 8), 3)
    Qc, ibc = Q.copy(), ib.copy()
    orc.sgd_iterations(orc.CSR(indptr, indices, data, 3, Q.shape[0]), P, Qc, ub, ibc, gb, (0.05, 0.02, 0.02, 0.02, 0.02), 42, 0, 150,
                       dot_order=orc.DOT_TREE16, update_items=False)
    want = _oracle_scores(P, Q, ub, ib, gb)
    for row, b in enumerate(blocks):
        rated = {i for i, _ in ratings[order[row]]}
        cand = sorted([(want[row, i], i) for i in range(Q.shape[0]) if i not in rated], key=lambda t: -t[0])[:5]
        got = [l.split("\t") for l in b.split("\n") if l.startswith("Rank:")]
        assert len(got) == 5
        for j, (fields, (score, item)) in enumerate(zip(got, cand)):
            assert fields[0] == "Rank: %d" % (j + 1) and abs(float(fields[2].split()[-1]) - score) <= 1e-5
            if j + 1 < len(cand) and cand[j][0] - cand[j + 1][0] > 1e-5 and (j == 0 or cand[j - 1][0] - cand[j][0] > 1e-5):
                assert int(fields[1].split()[1]) == item


# ------------------------------------------------------------------ against float64, with a stated bound
#
# s64 = gb + ub[u] + ib[i] + sum_k P[u,k] Q[i,k] in float64.  The device adds f + 3 terms in float32 with fused products (the
# matrix-core chain, then the three biases), whatever the association: f + 3 roundings, each at most 2^-24 times a partial
# sum no larger than the sum of the magnitudes, so |s_dev - s64| <= (f + 3) 2^-24 (|gb| + |ub[u]| + |ib[i]| + sum_k |P Q|).
# P and Q are drawn away from zero (random sign x U(0.2, 0.5)): every product is at least 0.04 in magnitude, while the bound
# stays below 4e-3 even at 512 factors -- so dropping or duplicating one factor column moves every score out of the bound,
# and misplacing one moves most of them.

FACTORS = [1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 252, 253, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512]
EPS32 = 2.0 ** -24


def _away_from_zero(rng, *shape):
    return (rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.2, 0.5, size=shape)).astype(np.float32)


def _draw(rng, users, items, f):
    P, Q = _away_from_zero(rng, users, f), _away_from_zero(rng, items, f)
    ub, ib = rng.uniform(-0.5, 0.5, users).astype(np.float32), rng.uniform(-0.5, 0.5, items).astype(np.float32)
    return P, Q, ub, ib


def _s64(P, Q, ub, ib, gb, users=None):
    """float64 scores and their bound, for the rows `users` (all when None)."""
    f = P.shape[1]
    P = P if users is None else P[users]
    ub = ub if users is None else ub[users]
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    s = float(np.float32(gb)) + ub.astype(np.float64)[:, None] + ib.astype(np.float64)[None, :] + P64 @ Q64.T
    mag = abs(float(np.float32(gb))) + np.abs(ub.astype(np.float64))[:, None] + np.abs(ib.astype(np.float64))[None, :] + \
        np.abs(P64) @ np.abs(Q64).T
    return s, (f + 3) * EPS32 * mag


def _ratio(got, s, bound):
    return float((np.abs(got.astype(np.float64) - s) / bound).max())


@pytest.mark.parametrize("f", FACTORS)
def test_scores_within_the_float64_bound_at_every_tile_edge(f):
    """Users {1, 31, 32, 33, 95} x items {1, 31, 32, 127, 128, 129, 4099}: the 32 x 128 tile of a workgroup, its edges and a
    partial last wavefront, at every row width (up to 63 slots the row is staged whole, above in chunks of 32 slots)."""
    rng = np.random.RandomState(f)
    P, Q, ub, ib = _draw(rng, 95, 4099, f)
    gb = 3.5
    worst = 0.0
    for users in (1, 31, 32, 33, 95):
        for items in (1, 31, 32, 127, 128, 129, 4099):
            model = cu.Model(users, items, f, gb, P[:users], Q[:items], ub[:users], ib[:items])
            got = model.scores()
            s, bound = _s64(P[:users], Q[:items], ub[:users], ib[:items], gb)
            r = _ratio(got, s, bound)
            assert r <= 1.0, (users, items, r)
            worst = max(worst, r)
            model.close()
    print("\nscores f=%d: max |s_dev - s64| / bound = %.4f" % (f, worst))


def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


@pytest.mark.parametrize("mode,f", [(m, f) for f in (5, 129, 251, 257, 385, 511) for m in
                                    ("serial", "ordered", "pingpong", "hogwild", "blocksolve") if m != "blocksolve" or f <= 252])
def test_scores_of_trained_models_within_the_float64_bound(mode, f):
    """Models that SGD left on the device (f % 4 != 0: the last float4 of a row is part padding), not only uploaded ones."""
    tr, _ = synth.make_ratings(300, 150, 4000, min_degree=3, seed=f)
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(cu.DeviceCSR(tr), (0.01, 0.02, 0.02, 0.02, 0.02), 42, 0, 3, mode=mode)
    P, Q, ub, ib = model.download()
    s, bound = _s64(P, Q, ub, ib, tr.global_bias)
    r = _ratio(model.scores(), s, bound)
    assert r <= 1.0, r


def _check_ranking(items, top, scores, s, bound, users, rated, k, n_items):
    """Ranking properties of rows `users` of recommend()'s (items, top): scores[u] = the device's own scores of user u,
    s / bound = float64 reference and bound for those users (one row each), rated[u] = the set excluded for user u."""
    for row, u in enumerate(users):
        excl = rated(u)
        unrated = n_items - len(excl)
        n = min(k, unrated)
        it, sc = items[u], top[u]
        assert (it[n:] == -1).all() and np.isnan(sc[n:]).all(), u           # padding exactly where fewer than k are unrated
        got = it[:n]
        assert (got >= 0).all() and (got < n_items).all(), u
        assert len(set(got.tolist())) == n and not (set(got.tolist()) & excl), u  # distinct, unrated
        assert not np.isnan(sc[:n]).any(), u
        np.testing.assert_array_equal(sc[:n], scores[row, got])             # the device's own scores, bit for bit
        if n == 0:
            continue
        assert (np.diff(sc[:n]) <= 0).all(), u                               # best first
        ties = sc[:n - 1] == sc[1:n]
        assert (got[:-1][ties] < got[1:][ties]).all(), u                     # equal scores: ascending item index (stable sort)
        # nothing the list left out beats its last entry by more than the two bounds together
        mask = np.ones(n_items, bool)
        mask[list(excl)] = False
        mask[got] = False
        last = got[-1]
        assert not (s[row, mask] > s[row, last] + bound[row, mask] + bound[row, last]).any(), u
        # and every listed score is within its bound of float64
        assert (np.abs(sc[:n].astype(np.float64) - s[row, got]) <= bound[row, got]).all(), u


def _rated_csr(rows_of, n_rows, n_items):
    indptr = np.zeros(n_rows + 1, np.int32)
    indptr[1:] = np.cumsum([len(rows_of.get(u, ())) for u in range(n_rows)])
    indices = np.array([i for u in range(n_rows) for i in sorted(rows_of.get(u, ()))], np.int32)
    return cu.HostCSR(indptr, indices, np.full(len(indices), 3.0, np.float32), n_rows, n_items, 3.0)


@pytest.mark.parametrize("f", [3, 64, 129, 253, 512])
def test_recommend_ranking_properties_ties_and_edge_users(f):
    """Users 0..39, items 0..149; the rated CSR has 30 rows (users 30..39 are not masked).  User 3 rated every item, user 5
    nothing; items 20..23 and 90, 91 (biases too) duplicate item 7's and item 60's row: bit-identical scores that must come out
    in ascending item order."""
    users, n_items = 40, 150
    rng = np.random.RandomState(f + 1)
    P, Q, ub, ib = _draw(rng, users, n_items, f)
    for dup, src in (((20, 21, 22, 23), 7), ((90, 91), 60)):
        for i in dup:
            Q[i], ib[i] = Q[src], ib[src]
    rows_of = {u: set(rng.choice(n_items, rng.randint(0, 40), replace=False).tolist()) for u in range(30)}
    rows_of[3], rows_of[5] = set(range(n_items)), set()
    model = cu.Model(users, n_items, f, 3.5, P, Q, ub, ib)
    scores = model.scores()
    assert (scores[:, [20, 21, 22, 23]] == scores[:, [7]]).all() and (scores[:, [90, 91]] == scores[:, [60]]).all()
    s, bound = _s64(P, Q, ub, ib, 3.5)
    d_rated = cu.DeviceCSR(_rated_csr(rows_of, 30, n_items))
    for k in (1, 7, n_items, n_items + 5):
        items, top = model.recommend(d_rated, k)
        _check_ranking(items, top, scores, s, bound, range(users), lambda u: rows_of.get(u, set()), k, n_items)
        assert (items[3] == -1).all() and np.isnan(top[3]).all()
        if k >= n_items:
            assert sorted(items[5].tolist()[:n_items]) == list(range(n_items))
            assert sorted(items[35].tolist()[:n_items]) == list(range(n_items))
        items, top = model.recommend(None, k)
        _check_ranking(items, top, scores, s, bound, range(users), lambda u: set(), k, n_items)


def test_recommend_across_batches():
    """model_recommend ranks users in batches of 2^28 / cols: 26,744 items (the ML-20M item count) give batches of 10,037 users;
    20,197 users = 10,037 + 10,037 + 123 (a partial last batch).  The rated CSR has 15,000 rows, so its end falls inside the
    second batch; user 10,036 (last of batch 1) rated every item, user 10,037 (first of batch 2) nothing.  Checked: the first
    and last user of every batch, both sides of the CSR's end and 50 seeded users, against float64 -- the full score matrix
    is never downloaded.  Each checked user inside the CSR rated its own five best items, so a batch masked with the wrong rows
    of the CSR lists rated items."""
    rows, cols, f, k, batch = 2 * 10037 + 123, 26744, 100, 25, 10037
    assert (1 << 28) // cols == batch
    rng = np.random.RandomState(7)
    P, Q, ub, ib = _draw(rng, rows, cols, f)
    rated_rows = 15000
    deg = rng.randint(0, 30, rated_rows)
    deg[10036], deg[10037] = cols, 0
    rows_of = {}
    for u in range(rated_rows):
        rows_of[u] = set(range(cols)) if deg[u] == cols else set(rng.randint(0, cols, deg[u]).tolist())
    check = sorted({0, batch - 1, batch, 2 * batch - 1, 2 * batch, rows - 1, rated_rows - 1, rated_rows} |
                   set(np.random.RandomState(11).choice(rows, 50, replace=False).tolist()))
    s, bound = _s64(P, Q, ub, ib, 3.5, users=check)
    for row, u in enumerate(check):  # a checked user inside the CSR rated its own five best items: masking it with another
        if u < rated_rows and u != 10037 and deg[u] < cols:  # row's ratings (or none) puts them back at the head of its list
            rows_of[u] |= set(np.argsort(-s[row])[:5].tolist())
    model = cu.Model(rows, cols, f, 3.5, P, Q, ub, ib)
    items, top = model.recommend(cu.DeviceCSR(_rated_csr(rows_of, rated_rows, cols)), k)
    # the device's own scores of the checked users: the same kernel on a model of just those rows
    sub = cu.Model(len(check), cols, f, 3.5, P[check], Q, ub[check], ib)
    scores = sub.scores()
    _check_ranking(items, top, scores, s, bound, check, lambda u: rows_of.get(u, set()), k, cols)
    assert (items[10036] == -1).all() and np.isnan(top[10036]).all()
    assert (items[10037] >= 0).all()


def test_bin_predict_many_users_at_300_factors_within_the_float64_bound(tmp_path):
    """bin/predict -u on a model bin/mf trained at 300 factors (its default mode there: ordered), three new users fitted with
    the items frozen (test_bin_predict_many_users_matches_oracle): the printed scores are the oracle fit's within the float64
    bound (plus the 5e-7 of printing with %f)."""
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    f = 300
    tr, te = synth.make_ratings(200, 40, 3000, min_degree=3, seed=2)
    synth.write_csv(str(tmp_path / "train.csv"), tr)
    synth.write_csv(str(tmp_path / "test.csv"), te)
    (tmp_path / "train.cfg").write_text("0 20 %d 0.02 42 0.02 0.02 0.02 0.02\n" % f)
    subprocess.run([mf, "-c", str(tmp_path / "train.cfg"), str(tmp_path / "train.csv"), str(tmp_path / "test.csv")],
                   stdout=subprocess.PIPE, check=True)
    (tmp_path / "predict.cfg").write_text("0 30 %d 0.05 42 0.02 0.02 0.02 0.02\n" % f)
    pre = str(tmp_path / ("train_f%d_" % f))
    model_args = ["-c", str(tmp_path / "predict.cfg"), "-i", pre + "item_bias.csv", "-g", pre + "global_bias.csv", "-q", pre + "q.csv"]
    rng = np.random.RandomState(3)
    users = {7: rng.choice(40, 6, replace=False), 3: rng.choice(40, 4, replace=False), 12: rng.choice(40, 9, replace=False)}
    ratings = {uid: [(int(i), rng.randint(1, 11) / 2.0) for i in its] for uid, its in users.items()}
    lines = ["userId,itemId,rating"]
    for uid in (7, 3, 12):
        lines += ["%d,%d,%.1f" % (uid, i + 1, r) for i, r in ratings[uid]]
    (tmp_path / "many.csv").write_text("\n".join(lines) + "\n")
    out = subprocess.run([predict] + model_args + ["-u", "-k", "40", str(tmp_path / "many.csv")], stdout=subprocess.PIPE,
                         text=True, check=True).stdout
    blocks = out.split("User: ")[1:]
    order = [3, 7, 12]
    assert [int(b.split("\n")[0]) for b in blocks] == order
    Q = cu.read_array(pre + "q.csv")
    ib = cu.read_array(pre + "item_bias.csv").ravel()
    gb = float(cu.read_array(pre + "global_bias.csv").ravel()[0])
    assert Q.shape == (40, f)
    indptr = np.cumsum([0] + [len(ratings[u]) for u in order]).astype(np.int32)
    indices = np.array([i for u in order for i, _ in ratings[u]], np.int32)
    data = np.array([r for u in order for _, r in ratings[u]], np.float32)
    P = np.tile(orc.normal_fill(f, f), (3, 1))
    ub = np.tile(orc.normal_fill(1, f), 3)
    orc.sgd_iterations(orc.CSR(indptr, indices, data, 3, Q.shape[0]), P, Q.copy(), ub, ib.copy(), gb, (0.05, 0.02, 0.02, 0.02, 0.02),
                       42, 0, 30, dot_order=orc.DOT_TREE16, update_items=False)
    s, bound = _s64(P, Q, ub, ib, gb)
    for row, b in enumerate(blocks):
        rated = {i for i, _ in ratings[order[row]]}
        got = [l.split("\t") for l in b.split("\n") if l.startswith("Rank:")]
        assert len(got) == 40 - len(rated)
        seen = []
        for j, fields in enumerate(got):
            item, score = int(fields[1].split()[1]), float(fields[2].split()[-1])
            assert fields[0] == "Rank: %d" % (j + 1) and item not in rated and item not in seen
            seen.append(item)
            assert abs(score - s[row, item]) <= bound[row, item] + 5e-7, (order[row], item, score, s[row, item])
