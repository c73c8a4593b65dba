"""ItemKNN on the device (cu2rec_knn_*) against tests/knn_reference64.py on the tables of tests/knn_checks.py: the weights within four
times float32's measured rounding, the `count` weighting on half-star data exactly (ids, values, tie order, padding), the float
weightings stage by stage within the fold's bound from the device's own outputs of the stage before, run-to-run bits, a query alone
against the query among others, the trainers on a CSR the knn calls have used, the ranking metrics, ML_SMALL, and bin/mf -m knn."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import knn_checks as chk
import knn_reference64 as ref
import rank_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def device(name):
    """(train, history, exclude) of a table on the device, once per process."""
    case = chk.cases()[name]
    return cu.DeviceCSR(case.train), cu.DeviceCSR(case.history), cu.DeviceCSR(case.exclude)


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_weights_within_four_times_float32_rounding(name):
    case = chk.cases()[name]
    d_train = device(name)[0]
    for weighting in ref.WEIGHTINGS:
        ratio = chk.weight_ratio(case.train, weighting, d_train.knn_weights(weighting))
        print("%s %s: %.3f of 4 x %.3g" % (name, weighting, ratio, chk.WEIGHT_DISTANCE))
        assert ratio <= 1.0, (name, weighting, ratio)
    assert np.array_equal(d_train.knn_weights("count"), case.train.data)


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_count_on_half_star_data_equals_float64_exactly(name):
    """ids, values, tie order and padding of neighbors() and recommend(): every product and sum is exact in float32.  The table
    `batches` needs two workspace batches for the build and for the recommend call."""
    case = chk.cases()[name]
    d_train, d_history, d_exclude = device(name)
    want = chk.exact(name)
    if name == "batches":
        batch = chk.workspace_batch(case.train.cols, 256)
        assert case.neighbours == case.k == 256 and case.train.cols > batch and len(case.users) > batch
    knn = cu.ItemKNN(d_train, "count", case.neighbours)
    ids, sims = knn.neighbors()
    assert chk.same_lists(ids, sims, want[0], want[1]), name
    k2 = min(case.neighbours, 3)
    ids, sims = knn.neighbors(case.ids, k2)  # a listed subset with duplicates, fewer than N
    assert chk.same_lists(ids, sims, want[0][case.ids][:, :k2], want[1][case.ids][:, :k2]), name
    items, scores = knn.recommend(d_history, d_exclude, case.k, case.users)
    assert chk.same_lists(items, scores, want[2], want[3]), name
    knn.close()


@pytest.mark.parametrize("weighting", chk.FLOAT_WEIGHTINGS)
@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_float_weightings_stage_by_stage(name, weighting):
    """(a) - (d) of knn_reference64.judge_lists for the build against float64 from the device's weights, and for recommend against
    float64 from the device's lists; then two calls bit for bit, and a query alone against the query among others."""
    case = chk.cases()[name]
    d_train, d_history, d_exclude = device(name)
    w = d_train.knn_weights(weighting)
    knn = cu.ItemKNN(d_train, weighting, case.neighbours)
    ids, sims = knn.neighbors()
    assert not chk.judge_neighbours(case.train, w, ids, sims, case.neighbours)
    items, scores = knn.recommend(d_history, d_exclude, case.k, case.users)
    assert not chk.judge_recommend(ids, sims, case.history, case.exclude, case.users, items, scores, case.k)
    # run to run, and a model built again
    again = cu.ItemKNN(d_train, weighting, case.neighbours)
    ids2, sims2 = again.neighbors()
    items2, scores2 = again.recommend(d_history, d_exclude, case.k, case.users)
    assert ids.tobytes() == ids2.tobytes() and sims.tobytes() == sims2.tobytes()
    assert items.tobytes() == items2.tobytes() and scores.tobytes() == scores2.tobytes()
    # one query alone
    u = int(case.users[3])
    one_items, one_scores = knn.recommend(d_history, d_exclude, case.k, [u])
    assert one_items.tobytes() == items[3:4].tobytes() and one_scores.tobytes() == scores[3:4].tobytes()
    i = int(case.ids[0])
    one_ids, one_sims = knn.neighbors([i])
    assert one_ids.tobytes() == ids[i:i + 1].tobytes() and one_sims.tobytes() == sims[i:i + 1].tobytes()
    knn.close()
    again.close()


def test_rows_that_repeat_a_column_are_refused():
    dup = cu.DeviceCSR(chk.duplicate_csr())
    with pytest.raises(cu.Cu2recError) as err:
        cu.ItemKNN(dup, "count", 5)
    assert err.value.status == -1 and "twice" in str(err.value)
    good = chk.duplicate_csr()
    good.indices[5] = 5  # the same rows without the repeat
    d_good = cu.DeviceCSR(good)
    knn = cu.ItemKNN(d_good, "count", 5)
    with pytest.raises(cu.Cu2recError) as err:
        knn.recommend(dup, None, 3)
    assert err.value.status == -1 and "twice" in str(err.value)
    knn.recommend(d_good, dup, 3)  # an exclusion may repeat


def test_refusals_on_the_device():
    case = chk.cases()["65-sparse"]
    d_train, d_history, _ = device("65-sparse")
    for args in (("count", 0), ("count", 257), (7, 5)):
        with pytest.raises(cu.Cu2recError) as err:
            cu.ItemKNN(d_train, *args)
        assert err.value.status == -1
    for kw in ({"k1": -1.0}, {"k1": np.inf}, {"b": 1.5}, {"b": -0.1}, {"b": np.nan}):
        with pytest.raises(cu.Cu2recError) as err:
            cu.ItemKNN(d_train, "bm25", 5, **kw)
        assert err.value.status == -1
    knn = cu.ItemKNN(d_train, "cosine", 5)
    other = cu.DeviceCSR(api.HostCSR([0, 1], [0], [1.0], 1, case.train.cols + 1, 0.0))
    for call in (lambda: knn.neighbors(k=6), lambda: knn.neighbors(k=0), lambda: knn.neighbors([case.train.cols]), lambda: knn.neighbors([-1]),
                 lambda: knn.recommend(d_history, None, 0), lambda: knn.recommend(d_history, None, 257),
                 lambda: knn.recommend(d_history, None, 3, [case.history.rows]), lambda: knn.recommend(other, None, 3),
                 lambda: knn.recommend(d_history, other, 3), lambda: knn.rank_metrics(d_history, other, 3),
                 lambda: knn.rank_metrics(other, d_history, 3)):
        with pytest.raises(cu.Cu2recError) as err:
            call()
        assert err.value.status == -1
    L = cu.lib()
    items, n, wt = (api.C.c_int() for _ in range(3))
    assert L.cu2rec_knn_info(knn._h, api.C.byref(items), api.C.byref(n), api.C.byref(wt)) == 0
    assert (items.value, n.value, wt.value) == (case.train.cols, 5, api.KNN_COSINE)


def test_trainers_are_unchanged_on_a_csr_the_knn_calls_have_used():
    """sgd (ordered), als and bpr from the same start on a fresh upload and on one ItemKNN has built from and recommended on."""
    case = chk.cases()["65-full"]
    hyper = (0.05, 0.02, 0.02, 0.02, 0.02)

    def run(d):
        out = []
        for step in (lambda m: m.sgd(d, hyper, 42, 0, 2, mode="ordered"), lambda m: m.als(d, hyper), lambda m: m.bpr(d, hyper)):
            m = cu.Model(case.train.rows, case.train.cols, 8, 3.0)
            step(m)
            out += [a.tobytes() for a in m.download()]
            m.close()
        return out

    fresh, used = cu.DeviceCSR(case.train), cu.DeviceCSR(case.train)
    knn = cu.ItemKNN(used, "bm25", 10)
    knn.recommend(used, used, 5)
    used.knn_weights("tfidf")
    assert run(fresh) == run(used)


def test_rank_metrics_equal_the_reference_on_the_devices_own_lists():
    for name, weighting, threshold in (("65-full", "cosine", None), ("2049-sparse", "count", 3.0)):
        case = chk.cases()[name]
        d_train, d_history, d_exclude = device(name)
        knn = cu.ItemKNN(d_train, weighting, case.neighbours)
        test = case.train.slice_users(0, case.history.rows - 1)  # fewer rows than the history: the last row is skipped
        d_test = cu.DeviceCSR(test)
        lists, _ = knn.recommend(d_history, d_exclude, case.k)
        got, per = knn.rank_metrics(d_history, d_test, case.k, exclude=d_exclude, threshold=threshold, per_user=True)
        want, want_per = rank_reference.rank_metrics(lists, test, case.k, threshold, rows=case.history.rows)
        print("%s: per-user distance %.3g, means %s" % (name, np.nanmax(np.abs(per - want_per)),
                                                       {key: got[key] - want[key] for key in ("precision", "recall", "ndcg", "map", "hit_rate")}))
        assert np.array_equal(per, want_per, equal_nan=True)
        for key in ("users_evaluated", "users_skipped", "k", "precision", "recall", "ndcg", "map", "hit_rate"):
            assert got[key] == want[key], key
        assert got["users_evaluated"] > 0


def test_ml_small_hits():
    """count: the recorded float64 hits exactly (every product and sum of half-star data is exact); cosine: within the users a float32
    run may decide differently (tests/test_knn_cpu.py measures both records)."""
    train, held = chk.ml_small()
    d_train = cu.DeviceCSR(train)
    for weighting in ("count", "cosine"):
        knn = cu.ItemKNN(d_train, weighting, chk.ML_SMALL_N)
        lists, _ = knn.recommend(d_train, d_train, chk.ML_SMALL_K)
        hits = ref.hits_at(lists, held)
        print("%s: %d hits of %d, float64 %d" % (weighting, hits, train.rows, chk.ML_SMALL_HITS[weighting]))
        slack = 0 if weighting == "count" else chk.ML_SMALL_COSINE_WITHIN_REACH
        assert abs(hits - chk.ML_SMALL_HITS[weighting]) <= slack
        res = knn.rank_metrics(d_train, cu.DeviceCSR(held), chk.ML_SMALL_K, exclude=d_train)
        assert round(res["hit_rate"] * res["users_evaluated"]) == hits and res["users_evaluated"] == train.rows
        knn.close()


def test_mf_knn_prints_the_metrics_line_and_writes_the_lists(tmp_path):
    case = chk.cases()["65-full"]
    train, test = case.train, case.history
    for name, csr in (("train.csv", train), ("test.csv", test)):
        rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
        with open(tmp_path / name, "w") as fh:
            fh.write("userId,itemId,rating\n" + "".join("%d,%d,%.1f\n" % (u + 1, i + 1, r) for u, i, r in zip(rows, csr.indices, csr.data)))
    res = subprocess.run([os.path.join(ROOT, "bin", "mf"), "-m", "knn", "-W", "tfidf", "-N", "7", "-k", "5", "-t", "2.5", str(tmp_path / "train.csv"),
                          str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    h_train, h_test = cu.createSparseMatrix(str(tmp_path / "train.csv")), cu.createSparseMatrix(str(tmp_path / "test.csv"))
    h_test = api.HostCSR(np.concatenate([h_test.indptr, np.full(h_train.rows - h_test.rows, h_test.nnz)]), h_test.indices, h_test.data,
                         h_train.rows, h_train.cols, 0.0)
    d_train = cu.DeviceCSR(h_train)
    knn = cu.ItemKNN(d_train, "tfidf", 7)
    m = knn.rank_metrics(d_train, cu.DeviceCSR(h_test), 5, exclude=d_train, threshold=2.5)
    line = "TEST: Precision@5: %f Recall@5: %f NDCG@5: %f MAP@5: %f HitRate@5: %f Users: %d Skipped: %d" % (
        m["precision"], m["recall"], m["ndcg"], m["map"], m["hit_rate"], m["users_evaluated"], m["users_skipped"])
    assert line in res.stdout.splitlines(), res.stdout
    ids, sims = knn.neighbors()
    for part, array in (("ids", ids), ("sims", sims)):
        cu.writeCSV(str(tmp_path / ("want_%s.csv" % part)), array)
        with open(tmp_path / ("want_%s.csv" % part), "rb") as a, open(tmp_path / ("train_knn_%s.csv" % part), "rb") as b:
            assert a.read() == b.read(), part
    assert re.search(r"Users: \d+ Skipped: \d+", res.stdout)
