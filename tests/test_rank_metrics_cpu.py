"""Ranking metrics without a GPU: the float64 reference (tests/rank_reference.py) on hand-computed cases, the argument checks
of cu2rec_model_topk / cu2rec_model_rank_metrics that come before the device check, and bin/mf's -k / -t flags."""
import math
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from conftest import ROOT
from cu2rec_amd.api import HostCSR
import rank_reference as rr

MF = os.path.join(ROOT, "bin", "mf")


def _csr(rows, cols=100):
    """rows: list of [(item, rating), ...] per user"""
    indptr = np.cumsum([0] + [len(r) for r in rows])
    items = [i for r in rows for i, _ in r]
    ratings = [x for r in rows for _, x in r]
    return HostCSR(indptr, items, ratings, len(rows), cols)


def test_known_answer_one_hit_at_rank_two():
    # L = [7, 3, 9], R = {3, 5}: one hit, at position j = 1
    res, per = rr.rank_metrics(np.array([[7, 3, 9]]), _csr([[(3, 4.0), (5, 5.0)]]), 3)
    assert per[0, 0] == 1 / 3
    assert per[0, 1] == 1 / 2
    assert per[0, 2] == (1 / math.log2(3)) / (1 + 1 / math.log2(3))
    assert per[0, 3] == (1 / 2) * (1 / 2)  # 1 / min(3, 2) * (1 hit so far / rank 2)
    assert per[0, 4] == 1.0
    assert res["precision"] == 1 / 3 and res["map"] == 0.25 and res["users_evaluated"] == 1 and res["users_skipped"] == 0


def test_known_answer_several_hits():
    # L = [1, 2, 3, 4], R = {1, 3, 8}: hits at j = 0 and j = 2
    _, per = rr.rank_metrics(np.array([[1, 2, 3, 4]]), _csr([[(8, 1.0), (3, 1.0), (1, 1.0)]]), 4)
    dcg = 1 / math.log2(2) + 1 / math.log2(4)
    idcg = 1 / math.log2(2) + 1 / math.log2(3) + 1 / math.log2(4)
    np.testing.assert_array_equal(per[0], [2 / 4, 2 / 3, dcg / idcg, (1 / 1 + 2 / 3) / 3, 1.0])


def test_duplicate_test_items_count_once():
    _, once = rr.rank_metrics(np.array([[3, 4]]), _csr([[(3, 5.0), (6, 5.0)]]), 2)
    _, twice = rr.rank_metrics(np.array([[3, 4]]), _csr([[(6, 5.0), (3, 5.0), (6, 4.0), (3, 1.0)]]), 2)
    np.testing.assert_array_equal(once, twice)
    assert once[0, 1] == 0.5


def test_threshold_filters_relevance():
    test = _csr([[(1, 5.0), (2, 3.5), (3, 4.0)]])
    lists = np.array([[2, 1, 3]])
    _, every = rr.rank_metrics(lists, test, 3)
    _, four = rr.rank_metrics(lists, test, 3, threshold=4.0)
    assert every[0, 1] == 1.0 and every[0, 3] == 1.0
    # R = {1, 3}: hits at j = 1, 2
    assert four[0, 0] == 2 / 3 and four[0, 1] == 1.0
    assert four[0, 3] == (1 / 2 + 2 / 3) / 2
    assert rr.rank_metrics(lists, test, 3, threshold=-math.inf)[1].tolist() == every.tolist()
    # a rating counts at the threshold itself; an item that only has ratings below it is not relevant
    _, high = rr.rank_metrics(lists, _csr([[(2, 3.5), (2, 5.0)]]), 3, threshold=5.0)
    assert high[0, 1] == 1.0 and high[0, 0] == 1 / 3


def test_items_past_the_catalogue_count_but_never_hit():
    # the model has 10 items; item 50 can never be listed, but is relevant
    _, per = rr.rank_metrics(np.array([[4, 5]]), _csr([[(4, 5.0), (50, 5.0), (50, 4.0)]], cols=60), 2)
    assert per[0, 1] == 0.5  # |R| = 2: 50 counts once
    assert per[0, 2] == 1 / (1 + 1 / math.log2(3))


def test_short_lists_divide_by_k():
    _, per = rr.rank_metrics(np.array([[5, -1, -1, -1]]), _csr([[(5, 3.0)]]), 4)
    assert per[0, 0] == 1 / 4 and per[0, 1] == 1.0 and per[0, 2] == 1.0 and per[0, 3] == 1.0
    _, per = rr.rank_metrics(np.array([[-1, -1]]), _csr([[(5, 3.0)]]), 2)  # nothing left to list: evaluated, no hit
    np.testing.assert_array_equal(per[0], [0.0, 0.0, 0.0, 0.0, 0.0])


def test_users_without_relevant_items_are_skipped():
    lists = np.array([[1, 2], [1, 2], [1, 2], [1, 2]])
    test = _csr([[(1, 5.0)], [], [(2, 1.0)]])  # row 3 is past the test set's rows
    res, per = rr.rank_metrics(lists, test, 2, threshold=3.0)
    assert res["users_evaluated"] == 1 and res["users_skipped"] == 3
    assert np.isnan(per[1:]).all() and not np.isnan(per[0]).any()
    assert res["precision"] == 0.5 and res["hit_rate"] == 1.0
    with pytest.raises(ValueError):
        rr.rank_metrics(lists[:2], test, 2)


def test_null_model_is_refused_before_the_device_check():
    L = cu.lib()
    items, scores = np.empty(4, np.int32), np.empty(4, np.float32)
    p = lambda a: a.ctypes.data_as(cu.api.C.c_void_p)  # noqa: E731
    assert L.cu2rec_model_topk(None, None, None, 0, 2, p(items), p(scores)) == -1  # CU2REC_EINVAL
    out = cu.api.RankMetrics()
    assert L.cu2rec_model_rank_metrics(None, None, None, 2, -math.inf, cu.api.C.byref(out), None) == -1


def _mf(*args):
    if not os.path.exists(MF):
        pytest.skip("bin/mf is not built")
    return subprocess.run([MF, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def test_mf_accepts_k_and_reaches_the_device_check(tmp_path):
    if cu.device_count() > 0:
        pytest.skip("a GPU is present")
    for extra in ([], ["-t", "4"]):
        res = _mf("-k", "10", *extra, str(tmp_path / "train.csv"), str(tmp_path / "test.csv"))
        assert res.returncode == 2 and "no HIP device" in res.stderr, res
        assert "Unknown option." not in res.stdout


def test_mf_refuses_bad_k_and_sharded_ranking(tmp_path):
    files = [str(tmp_path / "train.csv"), str(tmp_path / "test.csv")]
    for args in (["-k", "0"], ["-k", "257"], ["-k", "10", "-g", "2"], ["-g", "2", "-k", "5"]):
        res = _mf(*args, *files)
        assert res.returncode == 1, (args, res)
        assert "-k" in res.stderr and "Unknown option." not in res.stdout
    for bad in ("abc", "4x", "nan"):
        res = _mf("-k", "10", "-t", bad, *files)
        assert res.returncode == 1 and "-t" in res.stderr, (bad, res)
