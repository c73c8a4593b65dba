"""PureSVD on the device (cu2rec_model_svd and its two stages) against tests/svd_reference64.py with the judgements of
tests/svd_checks.py, stage by stage, each stage from the device's own output of the stage before: the product against float64 by the
order-free bound; orth within four times the float32 restatement's recorded figures, and its refusals; the whole iteration on the tables;
bit-level determinism; a refused call; serving through topk and rank_metrics; ML_SMALL; bin/mf -m svd and bin/predict -P; and the other
trainers and recommenders on a CSR the iteration has used."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import knn_reference64 as kref
import rank_reference
import svd_checks as chk
import svd_reference64 as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def product_device(name):
    return cu.DeviceCSR(chk.product_csrs()[name])


@functools.lru_cache(maxsize=None)
def table_device(name):
    return cu.DeviceCSR(chk.tables()[name].csr)


def fresh_model(name):
    t = chk.tables()[name]
    return cu.Model(t.csr.rows, t.csr.cols, t.f, 0.0)


@functools.lru_cache(maxsize=None)
def built(name):
    """(P, Q, user_bias, item_bias, report) of a table from a fresh model, once per process and read-only."""
    t = chk.tables()[name]
    m = fresh_model(name)
    rep = m.svd(table_device(name), t.sweeps)
    out = m.download() + (rep,)
    m.close()
    for a in out[:4]:
        a.setflags(write=False)
    return out


# ---- the product -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", chk.FS)
def test_product_both_sides_every_width(f):
    """X D with D at the item side's stride and the result at the user side's, X^T D the other way round, over rows of every length of
    ROW_LENGTHS, a row that stores a column twice, and the LONGEST column on the item-major side."""
    for name, transposes in (("lengths", (False, True)), ("lengths_t", (False, True)), ("longest", (True,))):
        if name == "longest" and f not in (5, 65, 129, 252):  # one width per E = 1 .. 4 is enough of the 65,537-entry column
            continue
        csr, d = chk.product_csrs()[name], product_device(name)
        for transpose in transposes:
            D = chk.operand(csr.rows if transpose else csr.cols, f, 7 * f + transpose)
            padded = d.multiply(D, transpose=transpose, padded=True)
            stride = f + (-f) % (32 if transpose else 4)
            assert padded.shape == (csr.cols if transpose else csr.rows, stride)
            assert not chk.judge_padding(padded, f), (name, transpose)
            assert not chk.judge_product(csr, D, padded[:, :f], transpose=transpose), (name, transpose)
            assert np.array_equal(d.multiply(D, transpose=transpose), padded[:, :f])  # and again: the same bits


def test_product_rows_without_entries_and_duplicates():
    csr, d = chk.product_csrs()["lengths"], product_device("lengths")
    D = chk.operand(csr.cols, 5, 3)
    out = d.multiply(D)
    assert not out[0].any()  # the row of length 0
    lo = csr.indptr[-2]
    want = sum(np.float64(csr.data[lo + j]) * D[csr.indices[lo + j]].astype(np.float64) for j in range(4))  # column 5 counted twice
    assert np.abs(out[-1] - want).max() <= chk.gamma(4) * np.abs(want).max() * 4
    never = np.bincount(csr.indices, minlength=csr.cols) == 0
    assert never.any() and not d.multiply(chk.operand(csr.rows, 5, 4), transpose=True)[never].any()
    with pytest.raises(cu.Cu2recError) as e:
        d.multiply(chk.operand(csr.cols, 253, 1))
    assert e.value.status == -6
    with pytest.raises(ValueError):
        d.multiply(chk.operand(csr.cols + 1, 4, 1))


# ---- orth ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", chk.ORTH_FS)
def test_orthonormalize(f):
    for n, ff in chk.orth_sizes():
        if ff != f:
            continue
        for kind in chk.ORTH_KINDS:
            Y = chk.orth_input(n, f, kind)
            Q = cu.orthonormalize(Y)
            rec = chk.ORTH_DISTANCE[chk.orth_key(n, f, kind)]
            print("%4d x %3d %-6s |QtQ - I| %.3g (recorded %.3g)  span %.3g (recorded %.3g)"
                  % (n, f, kind, ref.orth_error(Q), rec[0], ref.span_error(Q, Y), rec[1]))
            assert not chk.judge_orth(Q, Y, rec), (n, f, kind)
            assert np.array_equal(cu.orthonormalize(Y), Q)


def test_orthonormalize_refusals():
    Y = chk.orth_input(33, 5, "gauss").copy()
    Y[:, 3] = Y[:, 1]
    with pytest.raises(cu.Cu2recError) as e:
        cu.orthonormalize(Y)
    assert e.value.status == -6 and e.value.bad_column == 3 and "column 3" in str(e.value)
    Q = cu.orthonormalize(np.delete(Y, 3, axis=1))  # the same data with the column removed
    assert Q.shape == (33, 4) and ref.orth_error(Q) <= chk.MARGIN * 4e-7
    with pytest.raises(cu.Cu2recError) as e:
        cu.orthonormalize(chk.orth_input(31, 32, "gauss"))  # n < f
    assert e.value.status == -6 and e.value.bad_column == 31
    Y = chk.orth_input(33, 5, "gauss").copy()
    Y[7, 2] = np.nan
    with pytest.raises(cu.Cu2recError) as e:
        cu.orthonormalize(Y)
    assert e.value.status == -6 and 0 <= e.value.bad_column <= 2
    with pytest.raises(cu.Cu2recError) as e:
        cu.orthonormalize(np.zeros((9, 3), np.float32))
    assert e.value.status == -6 and e.value.bad_column == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(chk.tables()))
def test_tables_end_to_end(name):
    t = chk.tables()[name]
    P, Q, ub, ib, rep = built(name)
    P64, Q64, c64, _ = chk.run64(name)
    print("%s: scores %.3g from float64 (recorded %.3g), |QtQ - I| %.3g (recorded %.3g), captured %.3g (recorded %.3g), share %.4f"
          % (name, ref.score_distance(P, Q, P64, Q64), chk.SVD_DISTANCE[name][0], ref.orth_error(Q), chk.SVD_DISTANCE[name][1],
             abs(rep["captured"] - c64) / c64, chk.SVD_DISTANCE[name][2], rep["captured"] / rep["total"]))
    assert rep["sweeps"] == t.sweeps
    assert not chk.judge_model(name, P, Q, rep["captured"], rep["total"], ub, ib)
    assert not chk.judge_product(t.csr, Q, P)  # P is X Q of the device's own Q
    assert rep["captured"] <= rep["total"]


@pytest.mark.parametrize("name", sorted(chk.tables()))
def test_determinism(name):
    """A second model is bit-identical; two sweeps twice are four sweeps once; project(train) is the model's P."""
    d = table_device(name)
    first = built(name)
    t = chk.tables()[name]
    m = fresh_model(name)
    m.svd(d, t.sweeps)
    again = m.download()
    assert all(np.array_equal(a, b) for a, b in zip(again, first[:4]))
    assert np.array_equal(m.project(d), again[0])
    m.close()
    if name == "300x400-f252":
        return  # the widest table's sweeps are the slowest: the split is shown on the other three
    once, twice = fresh_model(name), fresh_model(name)
    once.svd(d, 4)
    twice.svd(d, 2)
    twice.svd(d, 2)
    assert all(np.array_equal(a, b) for a, b in zip(once.download(), twice.download()))
    once.close()
    twice.close()


def test_a_refused_call_leaves_the_model_as_it_was():
    """16 identical rows of small integers and an integer start: every product and every Gram entry is exact, the second pivot is
    exactly zero.  And the argument checks, before anything is touched."""
    rng = np.random.RandomState(9)
    row_items, row_vals = np.array([0, 2, 3, 5, 7]), np.array([1, 2, 1, 3, 2], np.float32)
    host = api.HostCSR(np.arange(17) * 5, np.tile(row_items, 16), np.tile(row_vals, 16), 16, 8, 0.0)
    d = cu.DeviceCSR(host)
    Q0 = rng.randint(-3, 4, size=(8, 4)).astype(np.float32)
    Q0[:, 0] = 1.0  # column 0 of X Q is 9 in every row: the first pivot is 16 x 81, its root exact
    P0, ub0, ib0 = rng.standard_normal((16, 4)).astype(np.float32), np.arange(16, dtype=np.float32), np.arange(8, dtype=np.float32) - 3
    m = cu.Model(16, 8, 4, 0.0, P=P0, Q=Q0, user_bias=ub0, item_bias=ib0)
    with pytest.raises(cu.Cu2recError) as e:
        m.svd(d, 3)
    assert e.value.status == -6 and "column 1" in str(e.value) and "sweep 0" in str(e.value)
    for got, want in zip(m.download(), (P0, Q0, ub0, ib0)):
        assert got.tobytes() == want.tobytes()
    with pytest.raises(cu.Cu2recError) as e:
        m.svd(d, 0)
    assert e.value.status == -1
    m.close()
    wide = cu.Model(16, 8, 9, 0.0)  # more factors than columns
    with pytest.raises(cu.Cu2recError) as e:
        wide.svd(d, 1)
    assert e.value.status == -6
    wide.close()
    small = cu.Model(15, 8, 4, 0.0)  # fewer rows than the ratings
    with pytest.raises(cu.Cu2recError) as e:
        small.svd(d, 1)
    assert e.value.status == -1
    with pytest.raises(cu.Cu2recError) as e:
        small.project(cu.DeviceCSR(api.HostCSR([0, 1], [0], [1.0], 1, 9, 0.0)))  # another column count
    assert e.value.status == -1
    small.close()


# ---- serving ---------------------------------------------------------------------------------------------------------------------
def test_serving_through_topk_and_rank_metrics():
    name = "300x200-f33"
    t, d = chk.tables()[name], table_device(name)
    P, Q, ub, ib, _ = built(name)
    m = fresh_model(name)
    m.svd(d, t.sweeps)
    same = cu.Model(t.csr.rows, t.csr.cols, t.f, 0.0, P=P, Q=Q, user_bias=ub, item_bias=ib)  # the device's own P and Q, uploaded
    items, scores = m.topk(d, 10)
    want_items, want_scores = same.topk(d, 10)
    assert not chk.judge_lists(items, want_items) and np.array_equal(scores, want_scores)
    S = P.astype(np.float64) @ Q.astype(np.float64).T  # and against float64 scores of that P and Q: the lists' values are theirs
    assert np.abs(scores - np.take_along_axis(S, items.astype(np.int64), axis=1)).max() <= chk.gamma(t.f) * np.abs(P).max() * np.abs(Q).max() * t.f
    rng = np.random.RandomState(2)
    held = api.HostCSR(np.arange(t.csr.rows + 1), rng.randint(0, t.csr.cols, t.csr.rows), np.ones(t.csr.rows, np.float32), t.csr.rows,
                       t.csr.cols, 0.0)
    got, per = m.rank_metrics(cu.DeviceCSR(held), 10, exclude=d, per_user=True)
    want, want_per = rank_reference.rank_metrics(items, held, 10, rows=t.csr.rows)
    np.testing.assert_allclose(per, want_per, rtol=1e-12, atol=0)
    for key in ("precision", "recall", "ndcg", "map", "hit_rate"):
        assert abs(got[key] - want[key]) <= 1e-12
    assert got["users_evaluated"] == want["users_evaluated"]
    ids, _ = m.similar([0, 5], k=3)
    assert ids.shape == (2, 3) and (ids >= 0).all()
    m.close()
    same.close()


def test_ml_small_hits():
    train, held = chk.ml_small()
    d = cu.DeviceCSR(train)
    m = cu.Model(train.rows, train.cols, chk.ML_SMALL_F, 0.0)
    rep = m.svd(d, chk.ML_SMALL_SWEEPS)
    lists, _ = m.topk(d, chk.ML_SMALL_K)
    hits = kref.hits_at(lists, held)
    print("PureSVD f = %d, %d sweeps: %d hits of %d, float64 %d; share %.4f" % (chk.ML_SMALL_F, chk.ML_SMALL_SWEEPS, hits, train.rows,
                                                                              chk.ML_SMALL_SVD_HITS, rep["captured"] / rep["total"]))
    assert abs(hits - chk.ML_SMALL_SVD_HITS) <= chk.ML_SMALL_SVD_WITHIN_REACH
    res = m.rank_metrics(cu.DeviceCSR(held), chk.ML_SMALL_K, exclude=d)
    assert round(res["hit_rate"] * res["users_evaluated"]) == hits
    m.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def write_csv(path, csr):
    rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    with open(path, "w") as fh:
        fh.write("userId,itemId,rating\n" + "".join("%d,%d,%.1f\n" % (u + 1, i + 1, r) for u, i, r in zip(rows, csr.indices, csr.data)))


COMPONENTS = ("p", "q", "user_bias", "item_bias", "global_bias")


def test_mf_svd_writes_what_train_returns_and_predict_projects(tmp_path):
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    t = chk.tables()["300x200-f33"]
    train_path, test_path, cfg_path = str(tmp_path / "train.csv"), str(tmp_path / "test.csv"), str(tmp_path / "c.cfg")
    write_csv(train_path, t.csr)
    write_csv(test_path, chk.tables()["70x90-f5"].csr)
    with open(cfg_path, "w") as fh:
        fh.write("0 3 33 0.01 42 0.02 0.02 0.02 0.02\n")
    res = subprocess.run([mf, "-m", "svd", "-c", cfg_path, "-k", "10", train_path, test_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    host = cu.createSparseMatrix(train_path)
    assert (host.rows, host.cols) == (t.csr.rows, t.csr.cols)
    cfg = cu.read_config(cfg_path)
    P, Q, report, ub, ib = cu.train(host, None, cfg, mode="svd", verbose=False)
    assert cfg.cur_iterations == 3 and not ub.any() and not ib.any()
    os.mkdir(tmp_path / "want")
    for comp, a, rows, cols in (("p", P, host.rows, 33), ("q", Q, host.cols, 33), ("user_bias", ub, host.rows, 1), ("item_bias", ib, host.cols, 1),
                                ("global_bias", np.zeros(1, np.float32), 1, 1)):
        cu.writeToFile(str(tmp_path / "want"), "train", comp, a, rows, cols, 33)
        with open(tmp_path / "want" / ("train_f33_%s.csv" % comp), "rb") as a_, open(tmp_path / ("train_f33_%s.csv" % comp), "rb") as b_:
            assert a_.read() == b_.read(), comp
    line = [x for x in res.stdout.splitlines() if x.startswith("SVD: ")]
    assert len(line) == 1 and line[0] == "SVD: Factors: 33 Sweeps: 3 Captured: %f Total: %f Share: %f" % (report[0], report[1], report[0] / report[1])
    assert [x for x in res.stdout.splitlines() if x.startswith("TEST: Precision@10")]
    assert res.stdout.splitlines().index(line[0]) < [i for i, x in enumerate(res.stdout.splitlines()) if x.startswith("TEST: ")][0]
    for flag, value in (("-a", "2"), ("-C", "3"), ("-g", "2"), ("-s", "4"), ("-w", "mean"), ("-W", "cosine"), ("-N", "20"), ("-L", "500"),
                        ("-l", "5"), ("-n", "3")):
        bad = subprocess.run([mf, "-m", "svd", "-c", cfg_path, flag, value, train_path, test_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True)
        assert bad.returncode != 0 and "usage: mf" in bad.stderr and "Free memory" not in bad.stdout, (flag, bad.stderr)

    # bin/predict -P: three new users, folded in by projection on the files just written
    new = api.HostCSR(t.csr.indptr[:4], t.csr.indices[:t.csr.indptr[3]], t.csr.data[:t.csr.indptr[3]], 3, t.csr.cols, 0.0)
    new_path = str(tmp_path / "new.csv")
    write_csv(new_path, new)
    files = {c: str(tmp_path / ("train_f33_%s.csv" % c)) for c in COMPONENTS}
    res = subprocess.run([predict, "-c", cfg_path, "-i", files["item_bias"], "-g", files["global_bias"], "-q", files["q"], "-P", "-u", "-k", "5",
                          new_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    got = [int(x) for x in re.findall(r"^Rank: \d+\tItem: (\d+)\t", res.stdout, flags=re.M)]
    Qf = cu.read_array(files["q"])
    d_new = cu.DeviceCSR(new)
    holder = cu.Model(3, t.csr.cols, 33, 0.0, P=np.zeros((3, 33), np.float32), Q=Qf, user_bias=np.zeros(3, np.float32),
                      item_bias=np.zeros(t.csr.cols, np.float32))
    proj = holder.project(d_new)
    assert not chk.judge_product(new, Qf, proj)
    served = cu.Model(3, t.csr.cols, 33, 0.0, P=proj, Q=Qf, user_bias=np.zeros(3, np.float32), item_bias=np.zeros(t.csr.cols, np.float32))
    want, _ = served.topk(d_new, 5)
    assert got == want.reshape(-1).tolist()
    for other in (["-A"], ["-I", "40"]):
        bad = subprocess.run([predict, "-c", cfg_path, "-i", files["item_bias"], "-g", files["global_bias"], "-q", files["q"], "-P"] + other +
                             [new_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert bad.returncode != 0 and "-P excludes" in bad.stderr
    holder.close()
    served.close()


# ---- the shared row plans and views ----------------------------------------------------------------------------------------------
def test_interoperation_with_the_trainers_and_recommenders():
    """ALS, ItemKNN and EASE on a fresh upload and on one the iteration has run and projected on (the row plans, the item-major view and
    the ALS workspace are shared); and the iteration on a CSR they have used."""
    t = chk.tables()["long-f64"]
    hyper = (0.05, 0.02, 0.02, 0.02, 0.02)

    def run(d):
        m = cu.Model(t.csr.rows, t.csr.cols, 8, 3.0)
        m.als(d, hyper)
        out = [a.tobytes() for a in m.download()]
        m.close()
        knn = cu.ItemKNN(d, "cosine", 10)
        out += [a.tobytes() for a in knn.neighbors(range(40))]
        knn.close()
        ease = cu.EASE(d, 20.0)
        out += [a.tobytes() for a in ease.recommend(d, d, 5, range(20))]
        ease.close()
        return out

    def svd_run(d):
        m = cu.Model(t.csr.rows, t.csr.cols, 8, 0.0)
        m.svd(d, 2)
        out = [a.tobytes() for a in m.download()] + [m.project(d).tobytes()]
        m.close()
        return out

    fresh, used = cu.DeviceCSR(t.csr), cu.DeviceCSR(t.csr)
    first = svd_run(used)
    want = run(fresh)
    assert run(used) == want
    assert svd_run(fresh) == first == svd_run(used)
