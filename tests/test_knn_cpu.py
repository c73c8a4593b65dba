"""ItemKNN without a GPU: what the header, the C ABI, the Python front end and bin/mf declare and refuse before any device is touched;
that the float32 restatement of tests/knn_reference64.py in the kernels' order passes the judgements of tests/knn_checks.py on every
table (the tables are fair) and that every deliberate mistake fails them on some table (they discriminate); the weights' measured
rounding; and the ML_SMALL experiment in float64, whose figures the GPU test is held to."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import knn_checks as chk
import knn_reference64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cu2rec_knn_create", "cu2rec_knn_info", "cu2rec_knn_slice_items", "cu2rec_csr_knn_weights", "cu2rec_knn_neighbors",
         "cu2rec_knn_recommend", "cu2rec_knn_rank_metrics")


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cu._lib.SIGNATURES
    assert re.search(r"\bvoid cu2rec_knn_destroy\(", header) and "cu2rec_knn_destroy" in cu._lib.SIGNATURES


def test_null_arguments_are_einval_without_a_device():
    L = cu.lib()
    assert L.cu2rec_knn_create(None, 1, 100.0, 0.8, 20, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_knn_info(None, None, None, None) == -1
    assert L.cu2rec_csr_knn_weights(None, 1, 100.0, 0.8, None) == -1
    assert L.cu2rec_knn_neighbors(None, None, 0, 1, None, None) == -1
    assert L.cu2rec_knn_recommend(None, None, None, None, 0, 1, None, None) == -1
    assert L.cu2rec_knn_rank_metrics(None, None, None, None, 1, 0.0, None, None) == -1
    L.cu2rec_knn_destroy(None)


def test_slice_width_needs_no_device():
    s = cu.lib().cu2rec_knn_slice_items()
    assert s > 0 and s % 256 == 0
    assert {c.train.cols for c in chk.cases().values()} >= {1, 2, 63, 64, 65, s - 1, s, s + 1, 2 * s + 1}


def test_python_front_end():
    assert "knn" not in api.MODES and sorted(api.MODES) == ["als", "blocksolve", "hogwild", "ordered", "pingpong", "serial"]
    params = inspect.signature(cu.ItemKNN.__init__).parameters
    assert [params[k].default for k in ("weighting", "neighbours", "k1", "b")] == ["cosine", 20, 100.0, 0.8]
    params = inspect.signature(cu.DeviceCSR.knn_weights).parameters
    assert [params[k].default for k in ("k1", "b")] == [100.0, 0.8]
    for method, names in (("neighbors", ["ids", "k"]), ("recommend", ["history", "exclude", "k", "users"]),
                          ("rank_metrics", ["history", "test", "k", "exclude", "threshold", "per_user"]), ("close", [])):
        assert list(inspect.signature(getattr(cu.ItemKNN, method)).parameters)[1:] == names
    blank = object.__new__(cu.DeviceCSR)  # no device object behind it: the name is refused before anything is called
    blank._h, blank.nnz = None, 0
    with pytest.raises(ValueError):
        cu.ItemKNN(blank, weighting="jaccard")
    with pytest.raises(ValueError):
        blank.knn_weights("Cosine")


def test_mf_usage_and_refusals_before_the_gpu():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bbpr\|knn\b", usage[0]) and "[-a alpha]" in usage[0], res.stderr
    assert "[-W count|cosine|tfidf|bm25]" in usage[0] and "[-N neighbours]" in usage[0]
    refused = (["-m", "knn"], ["-m", "knn", "-k", "5", "-a", "2"], ["-m", "knn", "-k", "5", "-C", "3"], ["-m", "knn", "-k", "5", "-g", "2"],
               ["-W", "cosine", "-k", "5"], ["-N", "20", "-k", "5"], ["-m", "bpr", "-W", "cosine"], ["-m", "knn", "-k", "5", "-W", "jaccard"],
               ["-m", "knn", "-k", "5", "-c", "some.cfg"], ["-m", "knn", "-k", "5", "-s", "4"], ["-m", "knn", "-k", "5", "-w", "mean"],
               ["-m", "knn", "-k", "5", "-N", "0"], ["-m", "knn", "-k", "5", "-N", "257"], ["-m", "knn", "-k", "5", "-N", "many"])
    for args in refused:
        res = subprocess.run([mf] + args + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)
    res = subprocess.run([mf, "-z", "a", "b"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 1 and "Unknown option." in res.stdout


def test_weights_restatement_distance():
    """The device's evaluation (double, rounded once) against float64 on every table and weighting: the figure knn_checks records."""
    worst = 0.0
    for name, case in chk.cases().items():
        for weighting in ref.WEIGHTINGS:
            want, got = ref.weights(case.train, weighting), ref.weights_f32(case.train, weighting).astype(np.float64)
            nz = want != 0
            assert (got[~nz] == 0).all()
            worst = max(worst, float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()))
            assert chk.weight_ratio(case.train, weighting, got) <= 0.25 + 1e-9
    print("worst relative distance %.4g" % worst)
    assert 0.9 * chk.WEIGHT_DISTANCE <= worst <= chk.WEIGHT_DISTANCE


def test_duplicates_are_seen_on_the_sorted_copy():
    assert ref.sorted_rows(chk.duplicate_csr())[1]
    assert not any(ref.sorted_rows(c.train)[1] or ref.sorted_rows(c.history)[1] for c in chk.cases().values())
    case = chk.cases()["2049-sparse"]
    assert ref.sorted_rows(case.exclude)[1]  # exclusions may repeat
    assert any((np.diff(case.train.indices[case.train.indptr[u]:case.train.indptr[u + 1]]) < 0).any() for u in range(case.train.rows))


def test_tables_cover_what_the_issue_lists():
    cases = chk.cases()
    assert {c.neighbours for c in cases.values()} == {c.k for c in cases.values()} == {1, 10, 256}
    for name, case in cases.items():
        lengths = set(np.diff(case.train.indptr).tolist())
        if case.train.cols >= 2047:
            assert lengths >= set(chk.ROW_LENGTHS), name
        if name.endswith("full"):
            assert case.train.cols in lengths  # a user who stores everything
        elif case.train.cols >= 63:
            stored = np.bincount(case.train.indices, minlength=case.train.cols)
            assert (stored == 0).any()  # items nobody stores
            ids = chk.exact(name)[0]
            assert (ids[:, -1] < 0).any() or case.neighbours == 1  # fewer touched candidates than N: padding
        assert len(set(case.ids.tolist())) < len(case.ids) and len(set(case.users.tolist())) < len(case.users)
    assert any((chk.exact(name)[0] < 0).any() for name in cases)
    big = cases["batches"]
    batch = chk.workspace_batch(big.train.cols, 256)
    assert batch < big.train.cols < 2 * batch and batch < len(big.users) < 2 * batch


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_restatement_in_the_kernels_order_passes_every_judgement(name):
    """count: the float32 folds equal float64 exactly; the float weightings: inside the bounds, stage by stage.  Every table under
    every weighting (of `batches`' 5,961 listed rows the first 40, which name all 8 distinct ones)."""
    case = chk.cases()[name]
    for weighting in ref.WEIGHTINGS:
        w = ref.weights_f32(case.train, weighting)
        ids, vals = ref.neighbours_f32(case.train, w, case.neighbours)
        users = case.users[:40]
        items, scores = ref.recommend_f32(ids, vals, case.history, case.exclude, users, case.k)
        if weighting == "count":
            want = chk.exact(name)
            assert chk.same_lists(ids, vals, want[0], want[1]) and chk.same_lists(items, scores, want[2][:40], want[3][:40])
        assert not chk.judge_neighbours(case.train, w, ids, vals, case.neighbours)
        assert not chk.judge_recommend(ids, vals, case.history, case.exclude, users, items, scores, case.k)


def test_every_deliberate_mistake_is_caught_on_some_table():
    caught = dict.fromkeys(ref.MUTATIONS, None)
    tables = [c for n, c in chk.cases().items() if c.train.cols <= 65]
    for mutation in ref.MUTATIONS:
        for case in tables:
            if mutation in ("norm_over_users", "log_n"):
                weighting = "cosine" if mutation == "norm_over_users" else "tfidf"
                bad = chk.weight_ratio(case.train, weighting, ref.weights(case.train, weighting, mutation=mutation)) > 1.0
            else:
                w = ref.weights_f32(case.train, "cosine")
                ids, vals = ref.neighbours(case.train, w, case.neighbours)
                bad = False
                if mutation in ("self_listed", "zeros_listed", "ties_descending", "last_partner_dropped"):
                    m_ids, m_vals = ref.neighbours(case.train, w, case.neighbours, mutation=mutation)
                    bad = bool(chk.judge_neighbours(case.train, w, m_ids, m_vals, case.neighbours))
                if not bad and mutation in ("excluded_listed", "ties_descending", "last_partner_dropped", "untruncated"):
                    lists = ref.neighbours(case.train, w, case.train.cols) if mutation == "untruncated" else (ids, vals)
                    items, scores = ref.recommend(lists[0], lists[1], case.history, case.exclude, case.users, case.k, mutation=mutation)
                    bad = bool(chk.judge_recommend(ids, vals, case.history, case.exclude, case.users, items, scores, case.k))
            if bad:
                caught[mutation] = case.name
                break
    print(caught)
    assert all(caught.values()), caught
    # and the unmutated float64 results pass
    for case in tables:
        w = ref.weights_f32(case.train, "cosine")
        ids, vals = ref.neighbours(case.train, w, case.neighbours)
        items, scores = ref.recommend(ids, vals, case.history, case.exclude, case.users, case.k)
        assert not chk.judge_neighbours(case.train, w, ids, vals, case.neighbours)
        assert not chk.judge_recommend(ids, vals, case.history, case.exclude, case.users, items, scores, case.k)


def test_ml_small_experiment_in_float64():
    """Every user's last stored entry held out, N = 20, hits @10 of 610 users for the four weightings and the popularity baseline: the
    records of knn_checks, which the GPU test is held to.  No float lists are compared: about half of the item rows tie at the N-th
    place."""
    train, held = chk.ml_small()
    hits = {"popularity": ref.hits_at(ref.popularity_lists(train, chk.ML_SMALL_K), held)}
    for weighting in ref.WEIGHTINGS:
        hits[weighting] = chk.ml_small_run(weighting)[0]
    reach = chk.within_reach("cosine")
    print("hits @%d of %d users: %s; cosine users within reach of a float32 flip: %d" % (chk.ML_SMALL_K, train.rows, hits, reach))
    assert hits == chk.ML_SMALL_HITS and reach == chk.ML_SMALL_COSINE_WITHIN_REACH
    assert hits["cosine"] >= 2 * hits["popularity"] > 0
    assert reach < hits["cosine"]
