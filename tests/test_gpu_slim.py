"""SLIM on the device (cu2rec_slim_create) against tests/slim_reference64.py on the tables of tests/slim_checks.py: W sweep by sweep
within four times the float32 restatement's recorded distance of float64 at the same sweep count; the EASE limit against the device's
own cu2rec_ease_create; optimality and the early stop of runs to a tol; run-to-run bits; the lists a SLIM handle serves; the refusals;
ML_SMALL; and bin/mf -m slim."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import ease_checks as echk
import ease_reference64 as eref
import knn_reference64 as kref
import slim_checks as chk
import slim_reference64 as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def device(name):
    """(train, history, exclude) of a table on the device, once per process."""
    case = chk.cases()[name]
    return cu.DeviceCSR(case.train), cu.DeviceCSR(case.history), cu.DeviceCSR(case.exclude)


def slim_of(name, sweeps, tol=0.0):
    case = chk.cases()[name]
    return cu.SLIM(device(name)[0], case.l1, case.l2, case.positive, sweeps, tol)


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_sweep_by_sweep(name):
    """(1) after 1, 2 and 3 sweeps (tol = 0): W within 4 x SLIM_DISTANCE of float64 at the same count, finite, a zero diagonal, zero
    rows and columns of unstored items, no negative weight under `positive`; the report's sweeps and nonzeros."""
    for sweeps in chk.COUNTS:
        slim = slim_of(name, sweeps)
        W = slim.weights()
        print("%s: %d sweeps, W is %.3g from float64, recorded %.3g; report %s" %
              (name, sweeps, chk.distance(W, chk.weights64(name, sweeps)), chk.SLIM_DISTANCE[name], slim.report))
        assert not chk.judge_weights(name, W, sweeps)
        assert slim.report["sweeps"] == sweeps and slim.report["nonzeros"] == np.count_nonzero(W)
        assert slim.report["last_delta"] >= 0
        slim.close()


@pytest.mark.parametrize("name", sorted(chk.EASE_LIMIT))
def test_the_ease_limit(name):
    """(2) l1 = 0, free signs, the recorded sweeps: W against the device's own EASE B, over max |B64|, within 4 x the distance of the
    two float32 restatements."""
    case = chk.cases()[name]
    sweeps, recorded = chk.EASE_LIMIT[name]
    d_train = device(name)[0]
    slim = cu.SLIM(d_train, 0.0, case.l2, False, sweeps, 0.0)
    ease = cu.EASE(d_train, case.l2)
    W, B = slim.weights(), ease.weights()
    top = float(np.abs(eref.weights(chk.gram64(name))).max())
    dist = float(np.abs(W.astype(np.float64) - B).max() / top)
    print("%s: %d sweeps, W is %.3g from the device's B, the restatements %.3g" % (name, sweeps, dist, recorded))
    assert slim.report["sweeps"] == sweeps and dist <= 4 * recorded
    slim.close()
    ease.close()


@pytest.mark.parametrize("name", sorted(chk.STOPS))
def test_early_stop_and_optimality(name):
    """(3), (4) a run to a tol stop ends at the sweep float64 ends at, with last_delta <= tol; the float64 KKT residual of its W is at
    most 4 x that of the float32 restatement stopped by the same tol."""
    l1, l2, positive, tol, stop = chk.STOPS[name]
    case = chk.cases()[name]
    slim = cu.SLIM(device(name)[0], l1, l2, positive, chk.STOP_CAP, tol)
    W = slim.weights()
    assert slim.report["sweeps"] == stop and 0 < slim.report["last_delta"] <= tol
    W32, tops = ref.blocked(eref.gram_f32(case.train, l2), l1, positive, chk.STOP_CAP, chk.block_items(), tol=tol)
    A = eref.gram(case.train, l2)
    mine, want = ref.kkt_residual(A, W, l1, positive), ref.kkt_residual(A, W32, l1, positive)
    print("%s: stopped after %d sweeps at %.3g; KKT residual %.3g, the restatement's %.3g" % (name, stop, slim.report["last_delta"], mine, want))
    assert len(tops) == stop and np.isfinite(W).all() and mine <= 4 * want
    slim.close()


@pytest.mark.parametrize("name", ["2-full", "65-sparse", "323-full", "2049-sparse"])
def test_determinism(name):
    """(5) two builds give bit-identical W, reports and lists."""
    case = chk.cases()[name]
    _, d_history, d_exclude = device(name)
    a, b = slim_of(name, 3), slim_of(name, 3)
    assert a.weights().tobytes() == b.weights().tobytes() and a.report == b.report
    for x, y in zip(a.recommend(d_history, d_exclude, case.k, case.users) + a.neighbors(case.ids, case.k),
                    b.recommend(d_history, d_exclude, case.k, case.users) + b.neighbors(case.ids, case.k)):
        assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["65-full", "129-sparse", "323-sparse", "2049-sparse"])
def test_serving(name):
    """(6) the lists of a SLIM handle against float64 scores from the device's own W (the sparse tables' W has all-zero rows)."""
    case = chk.cases()[name]
    _, d_history, d_exclude = device(name)
    slim = slim_of(name, 3)
    W = slim.weights()
    if name.endswith("sparse"):
        assert (~W.any(axis=1)).any() and W.any()
    assert np.array_equal(slim.weights(case.ids), W[case.ids])
    items, scores = slim.recommend(d_history, d_exclude, case.k, case.users)
    assert not echk.judge_recommend(W, case.history, case.exclude, case.users, items, scores, case.k)
    ids, vals = slim.neighbors(case.ids, case.k)
    assert not echk.judge_neighbours(W, case.ids, ids, vals, case.k)
    slim.close()


def test_refusals_on_the_device():
    """(7) every refusal returns its code and leaves the device clean; a SLIM and an EASE handle serve side by side."""
    case = chk.cases()["65-sparse"]
    d_train, d_history, d_exclude = device("65-sparse")
    L = cu.lib()
    h = api.C.c_void_p()
    wide = cu.DeviceCSR(api.HostCSR([0, 1], [0], [1.0], 1, api.EASE_MAX_ITEMS + 1, 0.0))
    assert L.cu2rec_slim_create(wide._h, 5.0, 500.0, 1, 3, 0.0, None, api.C.byref(h)) == -6 and h.value is None  # CU2REC_EUNSUPPORTED
    assert "CU2REC_EASE_MAX_ITEMS" in L.cu2rec_last_error().decode()
    for kw in ([dict(l1=v) for v in (-1.0, np.nan, np.inf)] + [dict(l2=v) for v in (0.0, -1.0, np.nan, np.inf)] +
               [dict(sweeps=v) for v in (0, -1)] + [dict(tol=v) for v in (-1.0, np.nan)]):
        with pytest.raises(cu.Cu2recError) as err:
            cu.SLIM(d_train, **kw)
        assert err.value.status == -1, kw
    with pytest.raises(cu.Cu2recError) as err:
        cu.SLIM(cu.DeviceCSR(chk.kchk.duplicate_csr()), 1.0, 1.0)
    assert err.value.status == -1 and "twice" in str(err.value)
    slim = slim_of("65-sparse", 3)  # the fault record is clean: the next entry point reports nothing
    ease = cu.EASE(d_train, case.l2)
    W, B = slim.weights(), ease.weights()
    assert W.tobytes() != B.tobytes()
    items, l2 = api.C.c_int(), api.C.c_float()
    for model in (slim, ease):
        assert L.cu2rec_ease_info(model._h, api.C.byref(items), api.C.byref(l2)) == 0 and (items.value, l2.value) == (case.train.cols, case.l2)
    for model, M in ((slim, W), (ease, B), (slim, W)):
        got, scores = model.recommend(d_history, d_exclude, 5, case.users)
        assert not echk.judge_recommend(M, case.history, case.exclude, case.users, got, scores, 5)
    with pytest.raises(cu.Cu2recError) as err:
        slim.neighbors(k=257)
    assert err.value.status == -1
    empty = cu.SLIM(cu.DeviceCSR(api.HostCSR([0, 0, 0], [], [], 2, 3, 0.0)), 1.0, 2.0)  # nnz == 0: a valid model of zeros
    assert not empty.weights().any() and empty.report["nonzeros"] == 0 and empty.neighbors(k=2)[0].tolist() == [[1, 2], [0, 2], [0, 1]]
    none = cu.SLIM(cu.DeviceCSR(api.HostCSR([0, 0], [], [], 1, 0, 0.0)))  # no items: an empty model
    assert none.weights().shape == (0, 0) and none.report == {"sweeps": 0, "last_delta": 0.0, "nonzeros": 0}
    d_bad = cu.DeviceCSR(api.HostCSR([0, 2, 4], [0, 1, 0, 1], [1.0, np.nan, 2.0, 3.0], 2, 2, 0.0))
    assert L.cu2rec_slim_create(d_bad._h, 1.0, 1.0, 1, 3, 0.0, None, api.C.byref(h)) == -6 and h.value is None
    assert "not a finite number" in L.cu2rec_last_error().decode()
    again = slim_of("65-sparse", 3)  # the device is as it was
    assert again.weights().tobytes() == W.tobytes()


def test_ml_small_hits():
    """(8) l1 = 5, l2 = 500, non-negative, 3 sweeps: within the users a float32 run may decide differently of the recorded float64
    hits."""
    train, held = chk.ml_small()
    d_train = cu.DeviceCSR(train)
    slim = cu.SLIM(d_train, chk.ML_SMALL_L1, chk.ML_SMALL_L2, True, chk.ML_SMALL_SWEEPS, 0.0)
    lists, _ = slim.recommend(d_train, d_train, chk.ML_SMALL_K)
    hits = kref.hits_at(lists, held)
    nonzero = slim.report["nonzeros"] / float(train.cols) ** 2
    print("SLIM: %d hits of %d, float64 %d; %.4f of W nonzero, float64 %.4f; report %s" %
          (hits, train.rows, chk.ML_SMALL_SLIM_HITS, nonzero, chk.ML_SMALL_SLIM_NONZERO, slim.report))
    assert abs(hits - chk.ML_SMALL_SLIM_HITS) <= chk.ML_SMALL_SLIM_WITHIN_REACH
    assert slim.report["sweeps"] == chk.ML_SMALL_SWEEPS and abs(nonzero - chk.ML_SMALL_SLIM_NONZERO) <= 1e-3
    res = slim.rank_metrics(d_train, cu.DeviceCSR(held), chk.ML_SMALL_K, exclude=d_train)
    assert round(res["hit_rate"] * res["users_evaluated"]) == hits and res["users_evaluated"] == train.rows
    slim.close()


def test_mf_slim_prints_the_report_and_writes_w(tmp_path):
    """(9) bin/mf -m slim on a small table prints the report line and the Python call's ranking line and writes W."""
    mf = os.path.join(ROOT, "bin", "mf")
    case = chk.cases()["65-full"]

    def write(path, csr):
        rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
        with open(path, "w") as fh:
            fh.write("userId,itemId,rating\n" + "".join("%d,%d,%.1f\n" % (u + 1, i + 1, r) for u, i, r in zip(rows, csr.indices, csr.data)))

    write(tmp_path / "train.csv", case.train)
    write(tmp_path / "test.csv", case.history)
    res = subprocess.run([mf, "-m", "slim", "-l", "2", "-L", "20", "-n", "4", "-k", "5", "-t", "2.5", str(tmp_path / "train.csv"), str(tmp_path / "test.csv")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    h_train, h_test = cu.createSparseMatrix(str(tmp_path / "train.csv")), cu.createSparseMatrix(str(tmp_path / "test.csv"))
    h_test = api.HostCSR(np.concatenate([h_test.indptr, np.full(h_train.rows - h_test.rows, h_test.nnz)]), h_test.indices, h_test.data,
                         h_train.rows, h_train.cols, 0.0)
    d_train, d_test = cu.DeviceCSR(h_train), cu.DeviceCSR(h_test)
    slim = cu.SLIM(d_train, 2.0, 20.0, True, 4, 1e-3)
    m = slim.rank_metrics(d_train, d_test, 5, exclude=d_train, threshold=2.5)
    line = "TEST: Precision@%d: %f Recall@%d: %f NDCG@%d: %f MAP@%d: %f HitRate@%d: %f Users: %d Skipped: %d" % (
        5, m["precision"], 5, m["recall"], 5, m["ndcg"], 5, m["map"], 5, m["hit_rate"], m["users_evaluated"], m["users_skipped"])
    out = res.stdout.splitlines()
    report = [x for x in out if x.startswith("SLIM: ")]
    assert line in out and len(report) == 1 and out.index(report[0]) < out.index(line), res.stdout
    assert report[0].startswith("SLIM: l1: 2 l2: 20 Sweeps: %d LastDelta: " % slim.report["sweeps"])
    assert report[0].endswith(" Nonzeros: %d of %d" % (slim.report["nonzeros"], h_train.cols ** 2))
    cu.writeCSV(str(tmp_path / "want_w.csv"), slim.weights())
    with open(tmp_path / "want_w.csv", "rb") as a, open(tmp_path / "train_slim_w.csv", "rb") as b:
        assert a.read() == b.read()
    assert not os.path.exists(tmp_path / "train_ease_b.csv")
    slim.close()
