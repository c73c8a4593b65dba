"""EASE on the device (cu2rec_ease_*) against tests/ease_reference64.py on the tables of tests/ease_checks.py, stage by stage, each stage
from the device's own output of the stage before: G exactly, B within four times the float32 restatement's recorded distance, the lists
within the fold's bound of float64 from the device's B; run-to-run bits, a rebuilt model, a query alone against the query among others;
the ranking metrics; the refused pivot; the other recommenders and trainers on a CSR EASE has used; ML_SMALL; and bin/mf -m ease."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import ease_checks as chk
import knn_reference64 as kref
import rank_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def device(name):
    """(train, history, exclude) of a table on the device, once per process."""
    case = chk.cases()[name]
    return cu.DeviceCSR(case.train), cu.DeviceCSR(case.history), cu.DeviceCSR(case.exclude)


@pytest.mark.parametrize("name", chk.inverse_tables())
def test_stages_in_turn(name):
    """(a) G equals float64 exactly; (b) B within 4 x EASE_DISTANCE of float64 from that G, zero diagonal, zero rows and columns of
    unstored items, finite; (c) recommend and neighbors against float64 from the device's B."""
    case = chk.cases()[name]
    d_train, d_history, d_exclude = device(name)
    G = d_train.ease_gram(case.l2)
    assert not chk.judge_gram(name, G)
    ease = cu.EASE(d_train, case.l2)
    B = ease.weights()
    print("%s: l2 %g, B is %.3g from float64, recorded %.3g" % (name, case.l2, chk.distance(B, chk.weights64(G)), chk.EASE_DISTANCE[name]))
    assert not chk.judge_weights(name, G, B)
    assert np.array_equal(ease.weights(case.ids), B[case.ids])  # a listed subset with duplicates
    items, scores = ease.recommend(d_history, d_exclude, case.k, case.users)
    assert not chk.judge_recommend(B, case.history, case.exclude, case.users, items, scores, case.k)
    ids, vals = ease.neighbors(case.ids, case.k)
    assert not chk.judge_neighbours(B, case.ids, ids, vals, case.k)
    if case.train.cols <= 2 * chk.block_items() + 1:  # every item, at the default k
        ids, vals = ease.neighbors()
        assert ids.shape == (case.train.cols, 10) and not chk.judge_neighbours(B, range(case.train.cols), ids, vals, 10)
    ease.close()


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_determinism(name):
    """(d) two calls and a rebuilt model bit for bit; one user alone and one id alone equal the batch's row.  `batches`: the recommend
    call takes two workspace batches, and its lists are judged here against float64 from the device's B."""
    case = chk.cases()[name]
    d_train, d_history, d_exclude = device(name)
    ease, again = cu.EASE(d_train, case.l2), cu.EASE(d_train, case.l2)
    items, scores = ease.recommend(d_history, d_exclude, case.k, case.users)
    if name == "batches":
        assert chk.workspace_batch(case.train.cols, case.k) < len(case.users)
        B = ease.weights()
        assert np.isfinite(B).all() and B.tobytes() == again.weights().tobytes()
        assert not chk.judge_recommend(B, case.history, case.exclude, case.users, items, scores, case.k)
        del B
    else:
        assert ease.weights().tobytes() == again.weights().tobytes()
    ids, vals = ease.neighbors(case.ids, case.k)
    for model in (ease, again):
        items2, scores2 = model.recommend(d_history, d_exclude, case.k, case.users)
        ids2, vals2 = model.neighbors(case.ids, case.k)
        assert items.tobytes() == items2.tobytes() and scores.tobytes() == scores2.tobytes()
        assert ids.tobytes() == ids2.tobytes() and vals.tobytes() == vals2.tobytes()
    one_items, one_scores = ease.recommend(d_history, d_exclude, case.k, [int(case.users[3])])
    assert one_items.tobytes() == items[3:4].tobytes() and one_scores.tobytes() == scores[3:4].tobytes()
    one_ids, one_vals = ease.neighbors([int(case.ids[1])], case.k)
    assert one_ids.tobytes() == ids[1:2].tobytes() and one_vals.tobytes() == vals[1:2].tobytes()
    ease.close()
    again.close()


def test_rank_metrics_equal_the_reference_on_the_devices_own_lists():
    """(e) per-user values and means at k = 1, 10 and 256.  Unlike ItemKNN's touched candidates, every item is a candidate, so a row has
    several hits and DCG, IDCG and AP are sums of up to k terms in double, whose order and log2 on the device are not Python's: the
    values, all in [0, 1], agree within 4 k 2^-53 (each of the two sums of a quotient up to k roundings of 2^-53 relative, doubled for
    the log2's own); with one hit at most (k = 1) that is equality."""
    for name, threshold in (("65-full", None), ("2048-sparse", 3.0), ("2049-sparse", 3.0)):
        case = chk.cases()[name]
        assert case.k == {"65-full": 1, "2048-sparse": 10, "2049-sparse": 256}[name]
        d_train, d_history, d_exclude = device(name)
        ease = cu.EASE(d_train, case.l2)
        test = case.train.slice_users(0, case.history.rows - 1)  # fewer rows than the history: the last row is skipped
        lists, _ = ease.recommend(d_history, d_exclude, case.k)
        got, per = ease.rank_metrics(d_history, cu.DeviceCSR(test), case.k, exclude=d_exclude, threshold=threshold, per_user=True)
        want, want_per = rank_reference.rank_metrics(lists, test, case.k, threshold, rows=case.history.rows)
        tol = 0.0 if case.k == 1 else 4 * case.k * 2.0 ** -53
        print("%s: k = %d, per-user distance %.3g, allowed %.3g" % (name, case.k, np.nanmax(np.abs(per - want_per)), tol))
        assert np.array_equal(np.isnan(per), np.isnan(want_per))
        for key in ("users_evaluated", "users_skipped", "k"):
            assert got[key] == want[key], key
        assert np.nanmax(np.abs(per - want_per)) <= tol
        assert all(abs(got[key] - want[key]) <= tol for key in ("precision", "recall", "ndcg", "map", "hit_rate"))
        assert got["users_evaluated"] > 0
        ease.close()


def twin_columns(value=5.0):
    """Two identical columns of `value` stored by the same 300 users."""
    return api.HostCSR(np.arange(301) * 2, np.tile([1, 0], 300), np.full(600, value), 300, 2, 0.0)


def test_a_bad_pivot_is_an_error_return():
    """(f) sum of squares 7,500, l2 = 1e-4 below half an ulp of it: G is [[7500, 7500], [7500, 7500]] in float.  (The second pivot is
    7500 - fl(7500 / fl(sqrt(7500)))^2; as an fmaf it is 2.25e-4, not 0 -- below 2^-22 of its diagonal entry, which is what the build
    refuses.)  CU2REC_EUNSUPPORTED and no handle; then a correct model on the same CSR with l2 = 1; a NaN value fails the same way."""
    L = cu.lib()
    d = cu.DeviceCSR(twin_columns())
    h = api.C.c_void_p()
    assert L.cu2rec_ease_create(d._h, 1e-4, api.C.byref(h)) == -6 and h.value is None
    message = L.cu2rec_last_error().decode()
    assert "item 1" in message and "not positive definite in float: raise l2" in message
    with pytest.raises(cu.Cu2recError) as err:
        cu.EASE(d, 1e-4)
    assert err.value.status == -6
    ease = cu.EASE(d, 1.0)
    G = np.array([[7501.0, 7500.0], [7500.0, 7501.0]])
    B = ease.weights()
    assert np.array_equal(d.ease_gram(1.0), G.astype(np.float32))
    assert chk.distance(B, chk.weights64(G)) <= 8 * 15001 * 2.0 ** -24 and (np.diag(B) == 0).all()  # condition number 15,001, a few roundings
    ids, vals = ease.neighbors()
    assert ids.tolist() == [[1] + [-1] * 9, [0] + [-1] * 9] and np.array_equal(vals[:, 0], [B[0, 1], B[1, 0]])
    ease.close()
    bad = twin_columns()
    bad.data[77] = np.nan
    d_bad = cu.DeviceCSR(bad)
    assert L.cu2rec_ease_create(d_bad._h, 1.0, api.C.byref(h)) == -6 and h.value is None
    ease = cu.EASE(d, 1.0)  # the device is as it was
    assert ease.weights().tobytes() == B.tobytes()
    ease.close()


def test_refusals_on_the_device():
    case = chk.cases()["65-sparse"]
    d_train, d_history, _ = device("65-sparse")
    L = cu.lib()
    h = api.C.c_void_p()
    wide = cu.DeviceCSR(api.HostCSR([0, 1], [0], [1.0], 1, api.EASE_MAX_ITEMS + 1, 0.0))
    assert L.cu2rec_ease_create(wide._h, 500.0, api.C.byref(h)) == -6 and h.value is None  # CU2REC_EUNSUPPORTED, nothing allocated
    assert "CU2REC_EASE_MAX_ITEMS" in L.cu2rec_last_error().decode()
    for l2 in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(cu.Cu2recError) as err:
            cu.EASE(d_train, l2)
        assert err.value.status == -1
    dup = cu.DeviceCSR(chk.kchk.duplicate_csr())
    with pytest.raises(cu.Cu2recError) as err:
        cu.EASE(dup, 1.0)
    assert err.value.status == -1 and "twice" in str(err.value)
    ease = cu.EASE(d_train, 20.0)
    other = cu.DeviceCSR(api.HostCSR([0, 1], [0], [1.0], 1, case.train.cols + 1, 0.0))
    for call in (lambda: ease.neighbors(k=0), lambda: ease.neighbors(k=257), lambda: ease.neighbors([case.train.cols]), lambda: ease.neighbors([-1]),
                 lambda: ease.weights([case.train.cols]), lambda: ease.recommend(d_history, None, 0), lambda: ease.recommend(d_history, None, 257),
                 lambda: ease.recommend(d_history, None, 3, [case.history.rows]), lambda: ease.recommend(other, None, 3),
                 lambda: ease.recommend(d_history, other, 3), lambda: ease.rank_metrics(d_history, other, 3),
                 lambda: ease.rank_metrics(other, d_history, 3)):
        with pytest.raises(cu.Cu2recError) as err:
            call()
        assert err.value.status == -1
    items, l2 = api.C.c_int(), api.C.c_float()
    assert L.cu2rec_ease_info(ease._h, api.C.byref(items), api.C.byref(l2)) == 0 and (items.value, l2.value) == (case.train.cols, 20.0)
    # a history row may store a column twice: each entry counts
    good = chk.kchk.duplicate_csr()
    good.indices[5] = 5
    twice = cu.EASE(cu.DeviceCSR(good), 1.0)
    got, scores = twice.recommend(dup, None, 6)
    B = twice.weights()
    assert not chk.judge_recommend(B, chk.kchk.duplicate_csr(), None, range(3), got, scores, 6)
    empty = cu.EASE(cu.DeviceCSR(api.HostCSR([0, 0, 0], [], [], 2, 3, 0.0)), 2.0)  # nnz == 0: a valid model, B = 0
    assert not empty.weights().any() and empty.neighbors(k=2)[0].tolist() == [[1, 2], [0, 2], [0, 1]]


def test_interoperation_with_the_trainers_and_itemknn():
    """(g) sgd (ordered), als, bpr and ItemKNN on a fresh upload and on one EASE has built from and recommended on; and EASE on a CSR
    they have used."""
    case = chk.cases()["65-full"]
    hyper = (0.05, 0.02, 0.02, 0.02, 0.02)

    def run(d):
        out = []
        for step in (lambda m: m.sgd(d, hyper, 42, 0, 2, mode="ordered"), lambda m: m.als(d, hyper), lambda m: m.bpr(d, hyper)):
            m = cu.Model(case.train.rows, case.train.cols, 8, 3.0)
            step(m)
            out += [a.tobytes() for a in m.download()]
            m.close()
        knn = cu.ItemKNN(d, "bm25", 10)
        out += [a.tobytes() for a in knn.neighbors() + knn.recommend(d, d, 5)]
        knn.close()
        return out

    def ease_run(d):
        ease = cu.EASE(d, 20.0)
        out = [ease.weights().tobytes()] + [a.tobytes() for a in ease.recommend(d, d, 5)] + [d.ease_gram(20.0).tobytes()]
        ease.close()
        return out

    fresh, used = cu.DeviceCSR(case.train), cu.DeviceCSR(case.train)
    first = ease_run(used)
    want = run(fresh)
    assert run(used) == want
    assert ease_run(fresh) == first == ease_run(used)


def test_ml_small_hits():
    """(h) l2 = 500: within the users a float32 run may decide differently of the recorded float64 hits, and above ItemKNN cosine's."""
    train, held = chk.ml_small()
    d_train = cu.DeviceCSR(train)
    ease = cu.EASE(d_train, chk.ML_SMALL_L2)
    lists, _ = ease.recommend(d_train, d_train, chk.ML_SMALL_K)
    hits = kref.hits_at(lists, held)
    print("EASE l2 = %g: %d hits of %d, float64 %d" % (chk.ML_SMALL_L2, hits, train.rows, chk.ML_SMALL_EASE_HITS))
    assert abs(hits - chk.ML_SMALL_EASE_HITS) <= chk.ML_SMALL_EASE_WITHIN_REACH
    assert hits > chk.kchk.ML_SMALL_HITS["cosine"]
    res = ease.rank_metrics(d_train, cu.DeviceCSR(held), chk.ML_SMALL_K, exclude=d_train)
    assert round(res["hit_rate"] * res["users_evaluated"]) == hits and res["users_evaluated"] == train.rows
    ease.close()


def test_mf_ease_prints_the_metrics_line_and_writes_b(tmp_path):
    """(i) bin/mf -m ease -L 500 -k 10 on ML_SMALL prints the Python call's ranking line (9,724 items: no B file, a word on stderr);
    on a small table it writes B; each refusal exits non-zero with the usage text."""
    mf = os.path.join(ROOT, "bin", "mf")
    train, held = chk.ml_small()

    def write(path, csr):
        rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
        with open(path, "w") as fh:
            fh.write("userId,itemId,rating\n" + "".join("%d,%d,%.1f\n" % (u + 1, i + 1, r) for u, i, r in zip(rows, csr.indices, csr.data)))

    def line_of(ease, d_train, d_test, k, threshold=None):
        m = ease.rank_metrics(d_train, d_test, k, exclude=d_train, threshold=threshold)
        return "TEST: Precision@%d: %f Recall@%d: %f NDCG@%d: %f MAP@%d: %f HitRate@%d: %f Users: %d Skipped: %d" % (
            k, m["precision"], k, m["recall"], k, m["ndcg"], k, m["map"], k, m["hit_rate"], m["users_evaluated"], m["users_skipped"])

    def loaded(train_path, test_path):
        h_train, h_test = cu.createSparseMatrix(train_path), cu.createSparseMatrix(test_path)
        h_test = api.HostCSR(np.concatenate([h_test.indptr, np.full(h_train.rows - h_test.rows, h_test.nnz)]), h_test.indices, h_test.data,
                             h_train.rows, h_train.cols, 0.0)
        return cu.DeviceCSR(h_train), cu.DeviceCSR(h_test)

    write(tmp_path / "ml.csv", train)
    write(tmp_path / "ml_test.csv", held)
    res = subprocess.run([mf, "-m", "ease", "-L", "500", "-k", "10", str(tmp_path / "ml.csv"), str(tmp_path / "ml_test.csv")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    d_train, d_test = loaded(str(tmp_path / "ml.csv"), str(tmp_path / "ml_test.csv"))
    ease = cu.EASE(d_train, 500.0)
    assert line_of(ease, d_train, d_test, 10) in res.stdout.splitlines(), res.stdout
    assert "ml_ease_b.csv is skipped" in res.stderr and not os.path.exists(tmp_path / "ml_ease_b.csv")
    ease.close()

    case = chk.cases()["65-full"]
    write(tmp_path / "train.csv", case.train)
    write(tmp_path / "test.csv", case.history)
    res = subprocess.run([mf, "-m", "ease", "-k", "5", "-t", "2.5", str(tmp_path / "train.csv"), str(tmp_path / "test.csv")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    d_train, d_test = loaded(str(tmp_path / "train.csv"), str(tmp_path / "test.csv"))
    ease = cu.EASE(d_train)  # the default l2 on both sides
    assert line_of(ease, d_train, d_test, 5, 2.5) in res.stdout.splitlines(), res.stdout
    cu.writeCSV(str(tmp_path / "want_b.csv"), ease.weights())
    with open(tmp_path / "want_b.csv", "rb") as a, open(tmp_path / "train_ease_b.csv", "rb") as b:
        assert a.read() == b.read()
    for args in (["-m", "ease"], ["-m", "ease", "-k", "5", "-L", "0"], ["-L", "500", "-k", "5"], ["-m", "ease", "-k", "5", "-N", "20"],
                 ["-m", "ease", "-k", "5", "-W", "cosine"], ["-m", "ease", "-k", "5", "-c", "some.cfg"], ["-m", "ease", "-k", "5", "-a", "2"],
                 ["-m", "ease", "-k", "5", "-C", "3"], ["-m", "ease", "-k", "5", "-g", "2"], ["-m", "ease", "-k", "5", "-s", "4"],
                 ["-m", "ease", "-k", "5", "-w", "mean"]):
        res = subprocess.run([mf] + args + [str(tmp_path / "train.csv"), str(tmp_path / "test.csv")], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)
