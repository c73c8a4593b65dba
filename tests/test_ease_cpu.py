"""EASE without a GPU: what the header, the C ABI, the Python front end and bin/mf declare and refuse before any device is touched; that
the float32 restatement of tests/ease_reference64.py in the kernels' order passes the judgements of tests/ease_checks.py on every table
(the tables are fair) and that every deliberate mistake fails them on some table (they discriminate); the restatement's measured
distance from float64 per table; and the ML_SMALL experiment in float64, whose figures the GPU test is held to."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import ease_checks as chk
import ease_reference64 as ref
import knn_reference64 as kref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cu2rec_ease_create", "cu2rec_ease_info", "cu2rec_ease_block_items", "cu2rec_csr_ease_gram", "cu2rec_ease_weights",
         "cu2rec_ease_neighbors", "cu2rec_ease_recommend", "cu2rec_ease_rank_metrics")


@functools.lru_cache(maxsize=None)
def restated(name):
    """(G32, B32) of a table: the float32 restatement, once per process."""
    case = chk.cases()[name]
    G = ref.gram_f32(case.train, case.l2)
    B = ref.weights_f32(G, chk.block_items())
    for a in (G, B):
        a.setflags(write=False)
    return G, B


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cu._lib.SIGNATURES
    assert re.search(r"\bvoid cu2rec_ease_destroy\(", header) and "cu2rec_ease_destroy" in cu._lib.SIGNATURES
    for name, value in (("CU2REC_EASE_MAX_ITEMS", api.EASE_MAX_ITEMS), ("CU2REC_EASE_MAX_K", api.EASE_MAX_K)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    assert re.search(r"\bCU2REC_EASE_WORKSPACE_BYTES = 64 << 20\b", header) and api.EASE_WORKSPACE_BYTES == 64 << 20


def test_refusals_without_a_device():
    """Bad l2 and bad k are CU2REC_EINVAL from the arguments alone: before the handles are looked at and before any device is touched.
    (More than CU2REC_EASE_MAX_ITEMS columns needs a cu2rec_csr, which needs a device: tests/test_gpu_ease.py.)"""
    L = cu.lib()
    h = api.C.c_void_p()
    for l2 in (0.0, -1.0, float("nan"), float("inf")):
        assert L.cu2rec_ease_create(None, l2, api.C.byref(h)) == -1 and h.value is None
        assert "l2" in L.cu2rec_last_error().decode()
        assert L.cu2rec_csr_ease_gram(None, l2, None) == -1 and "l2" in L.cu2rec_last_error().decode()
    for k in (0, -3, 257):
        for call in (lambda: L.cu2rec_ease_neighbors(None, None, 0, k, None, None),
                     lambda: L.cu2rec_ease_recommend(None, None, None, None, 0, k, None, None),
                     lambda: L.cu2rec_ease_rank_metrics(None, None, None, None, k, 0.0, None, None)):
            assert call() == -1 and "k must be in [1, 256]" in L.cu2rec_last_error().decode()
    assert L.cu2rec_ease_create(None, 500.0, api.C.byref(h)) == -1 and "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_ease_create(None, 500.0, None) == -1
    assert L.cu2rec_ease_info(None, None, None) == -1
    assert L.cu2rec_csr_ease_gram(None, 1.0, None) == -1
    assert L.cu2rec_ease_weights(None, None, 0, None) == -1
    assert L.cu2rec_ease_neighbors(None, None, 0, 1, None, None) == -1 and "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_ease_recommend(None, None, None, None, 0, 1, None, None) == -1
    assert L.cu2rec_ease_rank_metrics(None, None, None, None, 1, 0.0, None, None) == -1
    L.cu2rec_ease_destroy(None)


def test_block_order_needs_no_device_and_the_tables_cover_it():
    nb, s = chk.block_items(), chk.slice_items()
    assert nb > 0 and s % nb == 0
    cases = chk.cases()
    for cols in (1, 2, nb - 1, nb, nb + 1, 2 * nb + 1, 5 * nb + 3, s - 1, s, s + 1, 2 * s + 1):
        for kind in ("full", "sparse"):
            case = cases["%d-%s" % (cols, kind)]
            assert case.train.cols == cols
            lengths = set(np.diff(case.train.indptr).tolist())
            assert (cols in lengths) if kind == "full" else (cols < 3 or chk.unstored(case.train).any())
            if cols >= s - 1:
                assert lengths >= set(chk.kchk.ROW_LENGTHS)
            assert len(set(case.ids.tolist())) < len(case.ids) and len(set(case.users.tolist())) < len(case.users)
            assert not kref.sorted_rows(case.train)[1] and not kref.sorted_rows(case.history)[1]
    assert {c.l2 for c in cases.values()} == set(chk.L2S) and {c.k for c in cases.values()} == {1, 10, 256}
    big = cases["batches"]
    batch = chk.workspace_batch(big.train.cols, 256)
    assert big.train.cols == 4 * s + 1 and big.k == 256 and batch < len(big.users) < 2 * batch
    assert set(chk.EASE_DISTANCE) == set(chk.inverse_tables())


def test_python_front_end():
    assert inspect.signature(cu.EASE.__init__).parameters["l2"].default == 500.0
    for method, names in (("weights", ["ids"]), ("neighbors", ["ids", "k"]), ("recommend", ["history", "exclude", "k", "users"]),
                          ("rank_metrics", ["history", "test", "k", "exclude", "threshold", "per_user"]), ("close", [])):
        assert list(inspect.signature(getattr(cu.EASE, method)).parameters)[1:] == names
    assert inspect.signature(cu.EASE.neighbors).parameters["k"].default == 10
    assert list(inspect.signature(cu.DeviceCSR.ease_gram).parameters)[1:] == ["l2"]


def test_mf_usage_and_refusals_before_the_gpu():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bknn\|ease\b", usage[0]) and "[-L l2]" in usage[0], res.stderr
    refused = (["-m", "ease"], ["-L", "500", "-k", "5"], ["-m", "knn", "-L", "500", "-k", "5"], ["-m", "ease", "-k", "5", "-L", "0"],
               ["-m", "ease", "-k", "5", "-L", "-2"], ["-m", "ease", "-k", "5", "-L", "lots"], ["-m", "ease", "-k", "5", "-L", "nan"],
               ["-m", "ease", "-k", "5", "-c", "some.cfg"], ["-m", "ease", "-k", "5", "-a", "2"], ["-m", "ease", "-k", "5", "-C", "3"],
               ["-m", "ease", "-k", "5", "-g", "2"], ["-m", "ease", "-k", "5", "-s", "4"], ["-m", "ease", "-k", "5", "-w", "mean"],
               ["-m", "ease", "-k", "5", "-W", "cosine"], ["-m", "ease", "-k", "5", "-N", "20"])
    for args in refused:
        res = subprocess.run([mf] + args + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_restatement_in_the_kernels_order_passes_every_judgement(name):
    """G exactly, B within its recorded distance, the lists within the fold's bound of float64 from the restatement's own B (of
    `batches`' listed rows the first 40, which name all 8 distinct ones; its inverse is not judged)."""
    case = chk.cases()[name]
    G, B = restated(name)
    if name != "batches":
        assert not chk.judge_gram(name, G)
        assert not chk.judge_weights(name, G, B)
    users = case.users[:40]
    ids, vals = ref.recommend_f32(B, case.history, case.exclude, users, case.k)
    assert not chk.judge_recommend(B, case.history, case.exclude, users, ids, vals, case.k)
    k2 = min(case.k, 3)
    ids, vals = ref.neighbours_f32(B, case.ids, k2)
    assert not chk.judge_neighbours(B, case.ids, ids, vals, k2)
    want = min(k2, case.train.cols - 1)
    assert ((ids >= 0).sum(axis=1) == want).all()  # every other item is a candidate, stored or not


def test_restatement_distance():
    """max |B - B64| / max |B64| of the restatement per table: the figures ease_checks records."""
    for name in chk.inverse_tables():
        G, B = restated(name)
        dist = chk.distance(B, chk.weights64(G))
        print("%-12s l2 %-5g distance %.3g (recorded %.3g)" % (name, chk.cases()[name].l2, dist, chk.EASE_DISTANCE[name]))
        assert 0.5 * chk.EASE_DISTANCE[name] <= dist <= chk.EASE_DISTANCE[name], name


def test_every_deliberate_mistake_is_caught_on_some_table():
    nb = chk.block_items()
    caught = dict.fromkeys(ref.MUTATIONS, None)
    tables = [chk.cases()[n] for n in chk.inverse_tables() if chk.cases()[n].train.cols <= 5 * nb + 3]
    for mutation in ref.MUTATIONS:
        for case in tables:
            G = chk.gram64(case.name)
            if mutation in ("no_l2", "l2_twice"):
                bad = bool(chk.judge_gram(case.name, ref.gram(case.train, case.l2, mutation)))
            elif mutation in ("row_scaling", "diagonal_kept", "sign", "upper_not_mirrored", "tile_skipped"):
                try:
                    bad = bool(chk.judge_weights(case.name, G, ref.weights(G, mutation, nb)))
                except ref.NotPositiveDefinite:
                    bad = True
            else:
                B = chk.weights64(G)
                ids, vals = ref.neighbours(B, case.ids, case.k, mutation)
                bad = bool(chk.judge_neighbours(B, case.ids, ids, vals, case.k))
                if not bad and mutation == "untouched_dropped":
                    ids, vals = ref.recommend(B, case.history, case.exclude, case.users, case.k, mutation)
                    bad = bool(chk.judge_recommend(B, case.history, case.exclude, case.users, ids, vals, case.k))
            if bad:
                caught[mutation] = case.name
                break
    print(caught)
    assert all(caught.values()), caught
    # and the unmutated float64 results pass, the blocked algorithm in float64 included
    for case in tables:
        G = chk.gram64(case.name)
        B = chk.weights64(G)
        assert not chk.judge_weights(case.name, G, B) and not chk.judge_gram(case.name, ref.gram(case.train, case.l2))
        assert not chk.judge_weights(case.name, G, ref.weights_from_inverse(ref.blocked_inverse(G, nb, np.float64)))
        ids, vals = ref.recommend(B, case.history, case.exclude, case.users, case.k)
        assert not chk.judge_recommend(B, case.history, case.exclude, case.users, ids, vals, case.k)
        ids, vals = ref.neighbours(B, case.ids, case.k)
        assert not chk.judge_neighbours(B, case.ids, ids, vals, case.k)


def test_ml_small_experiment_in_float64():
    """Every user's last stored entry held out, l2 = 500, hits @10 of 610 users; the restatement's distance at that order and the users
    within reach of a float32 flip: the records of ease_checks, which the GPU test is held to."""
    train, held = chk.ml_small()
    hits, B64, _, _ = chk.ml_small_run()
    B32 = ref.weights_f32(ref.gram_f32(train, chk.ML_SMALL_L2), chk.block_items())
    dist = chk.distance(B32, B64)
    reach = chk.within_reach(chk.ML_SMALL_EASE_DISTANCE)
    lists32, _ = ref.recommend_f32(B32, train, train, None, chk.ML_SMALL_K)
    print("EASE l2 = %g: %d hits @%d of %d users (float32 restatement: %d); distance %.3g; users within reach: %d"
          % (chk.ML_SMALL_L2, hits, chk.ML_SMALL_K, train.rows, kref.hits_at(lists32, held), dist, reach))
    assert hits == chk.ML_SMALL_EASE_HITS and reach == chk.ML_SMALL_EASE_WITHIN_REACH
    assert 0.5 * chk.ML_SMALL_EASE_DISTANCE <= dist <= chk.ML_SMALL_EASE_DISTANCE
    assert abs(kref.hits_at(lists32, held) - hits) <= reach
    assert hits > chk.kchk.ML_SMALL_HITS["cosine"] > chk.kchk.ML_SMALL_HITS["popularity"]
