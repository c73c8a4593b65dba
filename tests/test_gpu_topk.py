"""Fused top-k and ranking metrics on the device (-m gpu): cu2rec_model_topk against cu2rec_model_recommend bit for bit (items and
the raw bits of the scores), cu2rec_model_rank_metrics against the float64 restatement in tests/rank_reference.py run on
recommend's lists, and bin/mf -k against Model.rank_metrics."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from conftest import ROOT, ml_small
from cu2rec_amd import prep, synth
from cu2rec_amd.api import HostCSR
import rank_reference as rr

pytestmark = pytest.mark.gpu


def _random_model(users, items, f, seed, scale=0.3):
    rng = np.random.RandomState(seed)
    P, Q = (rng.randn(users, f) * scale).astype(np.float32), (rng.randn(items, f) * scale).astype(np.float32)
    ub, ib = (rng.randn(users) * scale).astype(np.float32), (rng.randn(items) * scale).astype(np.float32)
    return P, Q, ub, ib


def _exclusions(rows, items, seed, full_row=None, per_row=(0, 40)):
    """rows x items exclusion CSR: unsorted rows with repeated items; row full_row (if any) excludes every item"""
    rng = np.random.RandomState(seed)
    lists = []
    for u in range(rows):
        if u == full_row:
            lst = rng.permutation(items).tolist() + [0, items - 1]
        else:
            n = rng.randint(per_row[0], per_row[1] + 1)
            lst = rng.randint(0, items, n).tolist()
            lst += lst[: len(lst) // 3]  # repeats
            rng.shuffle(lst)
        lists.append(lst)
    indptr = np.cumsum([0] + [len(l) for l in lists])
    flat = [i for l in lists for i in l]
    return HostCSR(indptr, flat, np.full(len(flat), 4.0, np.float32), rows, items)


def _assert_same(got, want):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape
    np.testing.assert_array_equal(gi, wi)
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))


# (users, items, f, k): every listed f, user count at the tile edges, item count and k appears at least once
CASES = [(1, 1, 1, 1), (31, 127, 4, 10), (33, 129, 31, 100), (65, 1000, 100, 256), (33, 26744, 128, 10),
         (31, 1000, 252, 256), (65, 129, 253, 100), (1, 26744, 300, 256), (65, 127, 100, 100), (33, 1000, 300, 1)]


@pytest.mark.parametrize("users,items,f,k", CASES)
def test_topk_equals_recommend_bit_for_bit(users, items, f, k):
    P, Q, ub, ib = _random_model(users, items, f, users * 7 + f)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    _assert_same(model.topk(None, k), model.recommend(None, k))
    # fewer exclusion rows than model rows; the first row (if there are two) excludes every item: all padding
    ex_rows = max(users - 1, 1)
    ex = cu.DeviceCSR(_exclusions(ex_rows, items, users + items, full_row=0 if users > 1 else None,
                                  per_row=(0, min(items, 150))))
    got = model.topk(ex, k)
    _assert_same(got, model.recommend(ex, k))
    if users > 1:
        assert (got[0][0] == -1).all() and np.isnan(got[1][0]).all()


def test_exact_ties_come_out_in_ascending_item_order():
    users, items, f, k = 40, 300, 24, 64
    P, Q, ub, ib = _random_model(users, items, f, 11)
    rng = np.random.RandomState(3)
    for src in rng.choice(items, 40, replace=False):  # 40 items get a twin or two with the same row and bias
        for dst in rng.choice(items, 2, replace=False):
            Q[dst], ib[dst] = Q[src], ib[src]
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    items_got, scores_got = model.topk(None, k)
    _assert_same((items_got, scores_got), model.recommend(None, k))
    ties = 0
    for u in range(users):
        same = scores_got[u, 1:] == scores_got[u, :-1]
        assert (items_got[u, 1:][same] > items_got[u, :-1][same]).all()
        ties += int(same.sum())
    assert ties > 0


def test_user_subset_with_duplicates_and_any_order():
    users, items, f, k = 70, 500, 100, 20
    P, Q, ub, ib = _random_model(users, items, f, 5)
    model = cu.Model(users, items, f, 3.5, P, Q, ub, ib)
    ex = cu.DeviceCSR(_exclusions(60, items, 9))
    full = model.recommend(ex, k)
    for ids in ([69, 3, 3, 0, 41, 69, 33, 32, 31], [5], list(range(69, -1, -1)) + [7] * 40):
        ids = np.array(ids, np.int32)
        _assert_same(model.topk(ex, k, users=ids), (full[0][ids], full[1][ids]))


def test_topk_refuses_bad_arguments():
    model = cu.Model(4, 10, 8, 3.0, *_random_model(4, 10, 8, 1))
    for k, users, status in ((0, None, -1), (257, None, -6), (3, [4], -1), (3, [-1], -1)):
        with pytest.raises(cu.Cu2recError) as e:
            model.topk(None, k, users=users)
        assert e.value.status == status
    assert "cu2rec_model_recommend" in str(pytest.raises(cu.Cu2recError, model.topk, None, 300).value)
    with pytest.raises(cu.Cu2recError):
        model.rank_metrics(cu.DeviceCSR(HostCSR([0, 1], [1], [4.0], 1, 10)), 3, threshold=float("nan"))
    with pytest.raises(cu.Cu2recError):  # test rows past the model's rows
        model.rank_metrics(cu.DeviceCSR(HostCSR([0] * 6, [], [], 5, 10)), 3)


def test_ml20m_items_across_recommends_batches():
    """ML-20M's catalogue and more users than one of recommend's batches ((1 << 28) / 26,744 = 10,037 users)."""
    tr, _ = synth.make_ratings(20_100, 26_744, 700_000, min_degree=3, seed=20)
    f, k = 100, 10
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias, *_random_model(tr.rows, tr.cols, f, 21, scale=0.1))
    ex = cu.DeviceCSR(tr)
    _assert_same(model.topk(ex, k), model.recommend(ex, k))


def _assert_metrics(model, test_host, k, exclude=None, threshold=None, rows=None):
    lists, _ = model.recommend(exclude, k)
    want, want_per = rr.rank_metrics(lists, test_host, k, threshold=threshold, rows=rows)
    got, per = model.rank_metrics(cu.DeviceCSR(test_host), k, exclude=exclude, threshold=threshold, per_user=True)
    np.testing.assert_allclose(per, want_per, rtol=1e-12, atol=0)
    assert np.array_equal(np.isnan(per), np.isnan(want_per))
    for name in ("users_evaluated", "users_skipped", "k"):
        assert got[name] == want[name], name
    for name in ("precision", "recall", "ndcg", "map", "hit_rate"):
        assert abs(got[name] - want[name]) <= 1e-12, (name, got[name], want[name])
    return got


def test_rank_metrics_edge_cases_match_the_reference():
    users, items, f, k = 50, 200, 16, 10
    model = cu.Model(users, items, f, 3.0, *_random_model(users, items, f, 8))
    scores = model.scores()
    rng = np.random.RandomState(4)
    rows = []
    for u in range(45):  # 5 model rows past the test set's last row
        best = np.argsort(-scores[u], kind="stable")[:15].tolist()
        lst = [(int(i), float(rng.choice([1.0, 3.5, 4.0, 5.0]))) for i in rng.choice(best, 6)]  # likely hits, duplicates
        lst += [(int(rng.randint(items)), 4.5), (items + 7, 5.0), (items + 7, 2.0)]  # past the catalogue, twice
        if u % 9 == 0:
            lst = []  # empty row
        if u % 11 == 1:
            lst = [(int(best[0]), 1.0), (int(best[1]), 2.0)]  # nothing reaches threshold 4
        rows.append(lst)
    indptr = np.cumsum([0] + [len(r) for r in rows])
    test = HostCSR(indptr, [i for r in rows for i, _ in r], [x for r in rows for _, x in r], len(rows), items + 10)
    ex = cu.DeviceCSR(_exclusions(40, items, 17, per_row=(0, 12)))
    for threshold in (None, 4.0, -math.inf, 5.0):
        for exclude in (None, ex):
            got = _assert_metrics(model, test, k, exclude=exclude, threshold=threshold, rows=users)
            assert got["users_skipped"] >= 5 + 5
    _assert_metrics(model, test, 1, exclude=ex, threshold=4.0, rows=users)
    _assert_metrics(model, test, 256, exclude=ex, rows=users)  # lists shorter than k (200 items, some excluded)


def _ml_small_split(tmp_path):
    return prep.split(ml_small(), train_dst=str(tmp_path / "train.csv"), test_dst=str(tmp_path / "test.csv"), keep_users=True)


def test_rank_metrics_of_a_trained_model_match_the_reference(tmp_path):
    train_path, test_path = _ml_small_split(tmp_path)
    tr, te = cu.createSparseMatrix(train_path), cu.createSparseMatrix(test_path)
    cfg = cu.default_config(total_iterations=100, n_factors=32, check_error=50)
    P, Q, _, ub, ib = cu.train(tr, te, cfg, mode="ordered", verbose=False)
    model = cu.Model(tr.rows, tr.cols, 32, tr.global_bias, P, Q, ub, ib)
    d_tr = cu.DeviceCSR(tr)
    for k, threshold in ((10, 4.0), (10, None), (50, 3.5)):
        got = _assert_metrics(model, te, k, exclude=d_tr, threshold=threshold, rows=tr.rows)
        assert got["users_evaluated"] > 300 and got["hit_rate"] > 0


_RANK_LINE = re.compile(r"^TEST: Precision@10: (\S+) Recall@10: (\S+) NDCG@10: (\S+) MAP@10: (\S+) HitRate@10: (\S+) "
                        r"Users: (\d+) Skipped: (\d+)$")


def test_bin_mf_k_prints_one_line_that_is_model_rank_metrics(tmp_path):
    tr, te = synth.make_ratings(300, 150, 9000, min_degree=3, seed=6, integer_ratings=True)
    synth.write_csv(str(tmp_path / "train.csv"), tr)
    synth.write_csv(str(tmp_path / "test.csv"), te)
    (tmp_path / "c.cfg").write_text("0 30 8 0.05 42 0.015 0.03 0.045 0.08\n")
    mf = os.path.join(ROOT, "bin", "mf")
    files = [str(tmp_path / "train.csv"), str(tmp_path / "test.csv")]
    comps = ["p", "q", "user_bias", "item_bias", "global_bias"]
    runs = []
    for extra in ([], ["-k", "10", "-t", "4"]):
        out = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "ordered"] + extra + files, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        csvs = {c: (tmp_path / ("train_f8_%s.csv" % c)).read_bytes() for c in comps}
        runs.append((out.stdout, csvs))
    (plain, plain_csv), (ranked, ranked_csv) = runs
    assert plain_csv == ranked_csv
    varying = ("Free memory:", "Time taken")  # free device memory and wall time differ from run to run
    keep = lambda s: [l for l in s.split("\n") if not l.startswith(varying)]  # noqa: E731
    assert keep(ranked)[:-2] == keep(plain)[:-1] and keep(ranked)[-1] == "" and keep(plain)[-1] == ""
    line = keep(ranked)[-2]
    m = _RANK_LINE.match(line)
    assert m, line

    tr_h, te_h = cu.createSparseMatrix(files[0]), cu.createSparseMatrix(files[1])
    cfg = cu.read_config(str(tmp_path / "c.cfg"))
    P, Q, _, ub, ib = cu.train(tr_h, te_h, cfg, mode="ordered", verbose=False)
    model = cu.Model(tr_h.rows, tr_h.cols, 8, tr_h.global_bias, P, Q, ub, ib)
    got = model.rank_metrics(cu.DeviceCSR(te_h), 10, exclude=cu.DeviceCSR(tr_h), threshold=4.0)
    want = ["%f" % got[n] for n in ("precision", "recall", "ndcg", "map", "hit_rate")]
    want += ["%d" % got["users_evaluated"], "%d" % got["users_skipped"]]
    assert list(m.groups()) == want
    assert got["users_evaluated"] > 0
