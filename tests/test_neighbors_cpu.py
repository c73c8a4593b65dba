"""Neighbour queries without a GPU: HostCSR.transpose() against a dense transpose, the host selection of
tests/neighbors_reference.py on hand cases, the argument checks of cu2rec_model_similar / cu2rec_model_top_users that come before
the device, and the usage errors of bin/predict -S."""
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from conftest import ROOT
from cu2rec_amd.api import C, HostCSR
import neighbors_reference as nr

PREDICT = os.path.join(ROOT, "bin", "predict")


def _dense(csr):
    """rows x cols counts of (row, index) pairs and the sum of their data"""
    count = np.zeros((csr.rows, csr.cols), np.int64)
    total = np.zeros((csr.rows, csr.cols), np.float64)
    for r in range(csr.rows):
        for e in range(csr.indptr[r], csr.indptr[r + 1]):
            count[r, csr.indices[e]] += 1
            total[r, csr.indices[e]] += csr.data[e]
    return count, total


@pytest.mark.parametrize("rows,cols,nnz", [(1, 1, 0), (5, 3, 12), (40, 17, 300), (3, 60, 9)])
def test_transpose_is_the_dense_transpose(rows, cols, nnz):
    rng = np.random.RandomState(rows * 100 + cols)
    per_row = np.bincount(rng.randint(0, rows, nnz), minlength=rows)
    indptr = np.concatenate([[0], np.cumsum(per_row)])
    indices = rng.randint(0, cols, nnz)  # unsorted rows with repeats
    data = rng.rand(nnz).astype(np.float32) * 5
    csr = HostCSR(indptr, indices, data, rows, cols, 3.25)
    t = csr.transpose()
    assert (t.rows, t.cols, t.nnz, t.global_bias) == (cols, rows, nnz, csr.global_bias)
    assert t.indptr.dtype == np.int32 and t.indices.dtype == np.int32 and t.data.dtype == np.float32
    count, total = _dense(csr)
    t_count, t_total = _dense(t)
    np.testing.assert_array_equal(t_count, count.T)
    np.testing.assert_allclose(t_total, total.T, rtol=1e-6)
    for i in range(t.rows):  # each row of the transpose lists its rows in ascending order
        assert (np.diff(t.indices[t.indptr[i]:t.indptr[i + 1]]) >= 0).all()
    tt = t.transpose()
    np.testing.assert_array_equal(_dense(tt)[0], count)


def test_host_selection_order_ties_and_padding():
    s = np.array([1.0, 3.0, -0.0, 3.0, -np.inf, 0.0, 2.0], np.float32)
    ids, sc = nr.select(s, np.ones(7, bool), 7)
    # 3.0 twice (ids 1, 3), 2.0, 1.0, then +0.0 / -0.0 tied: ascending id; -inf never listed; one slot of padding
    np.testing.assert_array_equal(ids, [1, 3, 6, 0, 2, 5, -1])
    assert sc[4].tobytes() == np.float32(-0.0).tobytes() and sc[5].tobytes() == np.float32(0.0).tobytes()
    assert np.isnan(sc[6])
    allowed = np.ones(7, bool)
    allowed[[1, 6]] = False
    np.testing.assert_array_equal(nr.select(s, allowed, 2)[0], [3, 0])


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_radix_code_hand_values():
    # rocPRIM's codes: sign clear -> bits ^ 0x80000000, sign set -> ~bits, with -0.0 first turned into +0.0
    bits = [0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF,
            0xFFC00000, 0xFF800001, 0x00000001, 0x80000001]
    want = [0x80000000, 0x80000000, 0xBF800000, 0x407FFFFF, 0xFF800000, 0x007FFFFF, 0xFFC00000, 0xFF800001, 0xFFFFFFFF,
            0x003FFFFF, 0x007FFFFE, 0x80000001, 0x7FFFFFFE]
    np.testing.assert_array_equal(nr.radix_code(_f32(bits)), np.array(want, np.uint32))
    assert nr.radix_code(_f32([0xFF800000]))[0] == nr.NEG_INF_CODE


def test_select_signed_zeros_tie_by_ascending_id():
    s = _f32([0x80000000, 0x00000000, 0x80000000, 0x3F800000, 0x00000000])  # -0, +0, -0, 1, +0
    ids, sc = nr.select(s, np.ones(5, bool), 5)
    np.testing.assert_array_equal(ids, [3, 0, 1, 2, 4])
    np.testing.assert_array_equal(sc.view(np.uint32), [0x3F800000, 0x80000000, 0x00000000, 0x80000000, 0x00000000])


def test_select_positive_nans_above_inf_and_negative_nans_never():
    # ids: 0 +inf, 1 quiet +NaN, 2 +NaN of payload 1, 3 -inf, 4 -NaN (x86's default), 5 2.0, 6 +NaN of the largest payload,
    # 7 -NaN of payload 1, 8 +inf, 9 -3.0, 10 quiet +NaN again
    bits = [0x7F800000, 0x7FC00000, 0x7F800001, 0xFF800000, 0xFFC00000, 0x40000000, 0x7FFFFFFF, 0xFF800001, 0x7F800000,
            0xC0400000, 0x7FC00000]
    s = _f32(bits)
    ids, sc = nr.select(s, np.ones(len(bits), bool), 12)
    # +NaNs by their codes (payload), equal NaNs by ascending id; then the two +inf by ascending id; 2.0, -3.0; -inf and
    # the sign-set NaNs never; padding only at the end
    np.testing.assert_array_equal(ids, [6, 1, 10, 2, 0, 8, 5, 9, -1, -1, -1, -1])
    np.testing.assert_array_equal(sc[:8].view(np.uint32), [bits[i] for i in (6, 1, 10, 2, 0, 8, 5, 9)])
    assert np.isnan(sc[8:]).all()
    # a short list is the head of the long one
    for k in (1, 3, 5, 8):
        np.testing.assert_array_equal(nr.select(s, np.ones(len(bits), bool), k)[0], ids[:k])


def test_select_padding_comes_only_at_the_end():
    # m listable entries, r excluded ones and some unlistable ones, m + r < k: the m entries, then padding
    rng = np.random.RandomState(3)
    for trial in range(200):
        n = rng.randint(1, 40)
        kinds = rng.randint(0, 6, n)
        vals = np.where(kinds == 0, -np.inf, np.where(kinds == 1, np.inf, rng.randn(n))).astype(np.float32)
        b = vals.view(np.uint32)
        b[kinds == 2] = 0xFFC00000 | rng.randint(0, 1 << 22, (kinds == 2).sum()).astype(np.uint32)  # -NaN
        b[kinds == 3] = 0x7FC00000 | rng.randint(0, 1 << 22, (kinds == 3).sum()).astype(np.uint32)  # +NaN
        allowed = rng.rand(n) < 0.7
        k = rng.randint(1, n + 5)
        ids, sc = nr.select(vals, allowed, k)
        listable = allowed & ~((kinds == 0) | (kinds == 2))
        m = min(k, int(listable.sum()))
        assert (ids[:m] >= 0).all() and (ids[m:] == -1).all() and np.isnan(sc[m:]).all()
        assert listable[ids[:m]].all() and len(set(ids[:m].tolist())) == m
        code = nr.radix_code(vals).astype(np.int64)
        key = code[ids[:m]] * 64 - ids[:m]  # (code, smaller id) descending: one strictly falling key
        assert (np.diff(key) < 0).all()
        if m < k:
            assert m == int(listable.sum())
        elif m:
            rest = listable.copy()
            rest[ids[:m]] = False
            assert not rest.any() or (code[rest] * 64 - np.nonzero(rest)[0]).max() < key[-1]


def test_cosine64_zero_rows():
    X = np.array([[1.0, 0.0], [0.0, 0.0], [3.0, 4.0]])
    c = nr.cosine64(X)
    assert c[0, 2] == pytest.approx(0.6) and c[2, 2] == pytest.approx(1.0)
    assert (c[1] == 0).all() and (c[:, 1] == 0).all()


def test_null_model_is_refused_before_the_device_check():
    L = cu.lib()
    out_i, out_s = np.empty(4, np.int32), np.empty(4, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.cu2rec_model_similar(None, 1, 1, None, None, 0, 2, p(out_i), p(out_s)) == -1  # CU2REC_EINVAL
    assert L.cu2rec_model_top_users(None, None, None, 0, 2, p(out_i), p(out_s)) == -1


def test_bad_side_and_metric_names_are_refused_in_python():
    model = object.__new__(cu.Model)  # no device object needed: the names are checked first
    with pytest.raises(ValueError):
        cu.Model.similar(model, side="rows")
    with pytest.raises(ValueError):
        cu.Model.similar(model, metric="euclidean")


def _predict(*args):
    if not os.path.exists(PREDICT):
        pytest.skip("bin/predict is not built")
    return subprocess.run([PREDICT, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def _files(tmp_path):
    (tmp_path / "c.cfg").write_text("0 5 4 0.01 42 0.01 0.01 0.01 0.01\n")
    (tmp_path / "q.csv").write_text("1,2,3,4\n5,6,7,8\n0,1,0,1\n")
    (tmp_path / "ids.txt").write_text("2\n0\n")
    return str(tmp_path / "c.cfg"), str(tmp_path / "q.csv"), str(tmp_path / "ids.txt")


def test_predict_similar_usage_errors(tmp_path):
    cfg, q, ids = _files(tmp_path)
    for args in (["-S", ids], ["-c", cfg, "-S", ids], ["-q", q, "-S", ids], ["-c", cfg, "-q", q, "-S"],
                 ["-c", cfg, "-q", q, "-S", "-k", "0", ids], ["-c", cfg, "-q", q, "-S", "-k", "257", ids],
                 ["-c", cfg, "-q", q, "-S", "-k", "5x", ids], ["-c", cfg, "-q", q, "-S", "-u", ids],
                 ["-c", cfg, "-q", q, "-S", ids, ids]):
        res = _predict(*args)
        assert res.returncode == 2 and "-S" in res.stderr and res.stdout == "", (args, res)


def test_predict_similar_refuses_bad_id_files(tmp_path):
    cfg, q, _ = _files(tmp_path)
    for text, what in (("0\n3\n", "not below"), ("1\nabc\n", "not an item index"), ("-1\n", "not an item index"),
                       ("1.5\n", "not an item index")):
        (tmp_path / "bad.txt").write_text(text)
        res = _predict("-c", cfg, "-q", q, "-S", str(tmp_path / "bad.txt"))
        assert res.returncode == 3 and what in res.stderr, (text, res)
    res = _predict("-c", cfg, "-q", q, "-S", str(tmp_path / "missing.txt"))
    assert res.returncode == 3 and "cannot open" in res.stderr


def test_predict_similar_reaches_the_device_check(tmp_path):
    if cu.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg, q, ids = _files(tmp_path)
    for extra in ([], ["-k", "2"], ["-i", "ignored.csv", "-g", "ignored.csv"]):
        res = _predict("-c", cfg, "-q", q, "-S", *extra, ids)
        assert res.returncode == 3 and "no HIP device" in res.stderr, (extra, res)
