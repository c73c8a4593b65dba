"""PureSVD without a GPU: what the header, the C ABI, the Python front end and bin/mf / bin/predict declare and refuse before any device
is touched; that the float64 reference of tests/svd_reference64.py finds numpy.linalg.svd's subspace; that its float32 restatement passes
the judgements of tests/svd_checks.py on every table, at the distances svd_checks records; that every judge catches a planted error; and
the ML_SMALL experiment in float64, whose figures the GPU test is held to."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import knn_reference64 as kref
import svd_checks as chk
import svd_reference64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cu2rec_model_svd", "cu2rec_model_project", "cu2rec_train_svd", "cu2rec_csr_multiply", "cu2rec_csr_multiply_stride",
         "cu2rec_orthonormalize")


@functools.lru_cache(maxsize=None)
def restated(name):
    """(P, Q, captured, total) of a table by the float32 restatement, once per process."""
    t = chk.tables()[name]
    return ref.svd32(t.csr, chk.start(name), t.sweeps)


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cu._lib.SIGNATURES
    assert re.search(r"typedef struct \{ int sweeps; double captured; double total; \} cu2rec_svd_report;", header)
    assert [n for n, _ in cu._lib.SvdReport._fields_] == ["sweeps", "captured", "total"]


def test_refusals_without_a_device():
    L = cu.lib()
    rep = cu._lib.SvdReport()
    assert L.cu2rec_model_svd(None, None, 4, api.C.byref(rep)) == -1 and "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_model_project(None, None, None) == -1
    assert L.cu2rec_train_svd(None, None, None, 0, None) == -1
    assert L.cu2rec_csr_multiply(None, 0, None, 4, None) == -1
    Y = np.ones((3, 5), np.float32)
    bad = api.C.c_int(-7)
    assert L.cu2rec_orthonormalize(api._ptr(Y), 3, 5, api.C.byref(bad)) == -6 and bad.value == 3  # n < f: before the device
    assert "column 3" in L.cu2rec_last_error().decode()
    for f in (0, 253):
        assert L.cu2rec_orthonormalize(api._ptr(Y), 300, f, api.C.byref(bad)) == -6
    assert L.cu2rec_orthonormalize(None, 3, 2, None) == -1
    assert [L.cu2rec_csr_multiply_stride(0, f) for f in (1, 4, 5, 252)] == [4, 4, 8, 252]
    assert [L.cu2rec_csr_multiply_stride(1, f) for f in (1, 32, 33, 252)] == [32, 32, 64, 256]
    with pytest.raises(cu.Cu2recError) as e:
        cu.orthonormalize(Y)
    assert e.value.status == -6 and e.value.bad_column == 3


def test_python_front_end():
    assert list(inspect.signature(cu.Model.svd).parameters)[1:] == ["train", "sweeps"]
    assert inspect.signature(cu.Model.svd).parameters["sweeps"].default == 4
    assert list(inspect.signature(cu.Model.project).parameters)[1:] == ["history"]
    assert list(inspect.signature(cu.DeviceCSR.multiply).parameters)[1:3] == ["D", "transpose"]
    assert inspect.signature(cu.DeviceCSR.multiply).parameters["transpose"].default is False
    assert callable(cu.orthonormalize)
    assert api.default_mode(50) == api.SGD_BLOCKSOLVE and api.default_mode(300) == api.SGD_ORDERED


def test_mf_and_predict_usage_and_refusals_before_the_gpu():
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bsvd\b", usage[0]), res.stderr
    for flag, value in (("-a", "2"), ("-C", "3"), ("-g", "2"), ("-s", "4"), ("-w", "mean"), ("-W", "cosine"), ("-N", "20"), ("-L", "500"),
                        ("-l", "5"), ("-n", "3")):
        res = subprocess.run([mf, "-m", "svd", flag, value, "missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (flag, res.stderr)
    res = subprocess.run([predict, "-u", "missing_new.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "usage: predict" in res.stderr and "[-P]" in res.stderr
    for other in (["-A"], ["-I", "-a", "40"]):
        res = subprocess.run([predict, "-P"] + other + ["-c", "missing.cfg", "missing_train.csv", "missing_new.csv"], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "-P" in res.stderr, (other, res.stderr)


def test_float64_reference_finds_the_dominant_subspace():
    """A 60 x 80 matrix with a planted gap after sigma_6: after enough sweeps the projector Q Q^T is numpy.linalg.svd's top-6 projector
    to 1e-9, and captured never exceeds the optimum sum of sigma^2."""
    rng = np.random.RandomState(5)
    U_, _ = np.linalg.qr(rng.standard_normal((60, 60)))
    V_, _ = np.linalg.qr(rng.standard_normal((80, 60)))
    s = np.concatenate([np.linspace(40, 25, 6), np.linspace(1.0, 0.01, 54)])
    X = (U_ * s) @ V_.T
    f = 6
    proj, best = ref.optimum(X, f)
    Q0 = ref.start(80, f)
    last = 0.0
    for sweeps in (1, 2, 4, 8, 12):
        P, Q, captured, total = ref.svd64(X, Q0, sweeps)
        assert captured <= best * (1 + 1e-12) and captured >= last * (1 - 1e-12) and captured <= total
        last = captured
        assert ref.orth_error(Q) < 1e-13
    assert np.abs(Q @ Q.T - proj).max() <= 1e-9
    assert abs(captured - best) <= 1e-9 * best


def test_tables_meet_what_they_are_for():
    t = chk.tables()
    assert [(x.csr.rows, x.csr.cols, x.f) for x in t.values()] == [(70, 90, 5), (300, 200, 33), (1100, 1100, 64), (300, 400, 252)]
    long = t["long-f64"].csr
    assert np.diff(long.indptr).max() > api.ALS_CHUNK and np.bincount(long.indices).max() > api.ALS_CHUNK
    p = chk.product_csrs()
    assert set(chk.ROW_LENGTHS) <= set(np.diff(p["lengths"].indptr).tolist())
    assert set(chk.ROW_LENGTHS) <= set(np.bincount(p["lengths_t"].indices, minlength=p["lengths_t"].cols).tolist())
    assert kref.sorted_rows(p["lengths"])[1]  # a row stores a column twice
    assert np.bincount(p["longest"].indices, minlength=3).tolist()[:2] == [chk.LONGEST, 0]
    assert chk.LONGEST > api.ALS_CHUNK * api.ALS_MAX_CHUNKS
    assert set(chk.ORTH_DISTANCE) == {chk.orth_key(n, f, k) for n, f in chk.orth_sizes() for k in chk.ORTH_KINDS}
    assert set(chk.SVD_DISTANCE) == set(t)


@pytest.mark.parametrize("name", sorted(chk.tables()))
def test_restatement_passes_every_judgement(name):
    t = chk.tables()[name]
    P, Q, captured, total = restated(name)
    assert not chk.judge_model(name, P, Q, captured, total, margin=1.0)
    assert not chk.judge_product(t.csr, Q, P)  # P is X Q of its own Q
    Y = ref.multiply32(t.csr, P, transpose=True)
    assert not chk.judge_product(t.csr, P, Y, transpose=True)


def test_restatement_distance():
    """The figures svd_checks.SVD_DISTANCE records, per table."""
    for name in chk.tables():
        P64, Q64, c64, _ = chk.run64(name)
        P, Q, captured, _ = restated(name)
        got = (ref.score_distance(P, Q, P64, Q64), ref.orth_error(Q), abs(captured - c64) / c64)
        print("%-14s scores %.3g  |QtQ - I| %.3g  captured %.3g  (recorded %s)" % ((name,) + got + (chk.SVD_DISTANCE[name],)))
        for measured, recorded in zip(got, chk.SVD_DISTANCE[name]):
            assert chk.pinned(measured, recorded), (name, measured, recorded)


def test_orth_restatement_figures():
    """The figures svd_checks.ORTH_DISTANCE records, per input; every input is accepted."""
    for n, f in chk.orth_sizes():
        for kind in chk.ORTH_KINDS:
            Y = chk.orth_input(n, f, kind)
            Q = ref.orth32(Y)
            key = chk.orth_key(n, f, kind)
            got = (ref.orth_error(Q), ref.span_error(Q, Y))
            for measured, recorded in zip(got, chk.ORTH_DISTANCE[key]):
                assert chk.pinned(measured, recorded), (key, got, chk.ORTH_DISTANCE[key])
            assert not chk.judge_orth(Q, Y, chk.ORTH_DISTANCE[key], margin=1.0)


def test_refused_inputs_are_refused_by_the_restatement_too():
    Y = chk.orth_input(33, 5, "gauss").copy()
    Y[:, 3] = Y[:, 1]
    with pytest.raises(ref.BadPivot) as e:
        ref.orth32(Y)
    assert e.value.column == 3
    ref.orth32(np.delete(Y, 3, axis=1))
    Y = chk.orth_input(33, 5, "gauss").copy()
    Y[7, 2] = np.nan
    with pytest.raises(ref.BadPivot):
        ref.orth32(Y)
    with pytest.raises(ref.BadPivot):
        ref.orth32(np.zeros((9, 3), np.float32))


def test_every_judge_catches_a_planted_error():
    name = "300x200-f33"
    t = chk.tables()[name]
    P, Q, captured, total = (np.array(a) if isinstance(a, np.ndarray) else a for a in restated(name))
    # one wrong entry in a product
    bad = P.copy()
    bad[17, 4] += 64 * np.spacing(np.abs(bad[17]).max())
    assert chk.judge_product(t.csr, Q, bad) and not chk.judge_product(t.csr, Q, P)
    padded = np.zeros((4, 8), np.float32)
    assert not chk.judge_padding(padded, 5)
    padded[2, 6] = 1e-30
    assert chk.judge_padding(padded, 5)
    # one swapped pair in a list
    lists = chk.lists_of(P.astype(np.float64) @ Q.astype(np.float64).T, t.csr, 10)
    swapped = lists.copy()
    swapped[3, [4, 5]] = swapped[3, [5, 4]]
    assert chk.judge_lists(swapped, lists) and not chk.judge_lists(lists.copy(), lists)
    # a Q with one column scaled by 1 + 1e-3: orth's judge, and the model's
    scaled = Q.copy()
    scaled[:, 7] *= np.float32(1 + 1e-3)
    assert chk.judge_model(name, P, scaled, captured, total) and not chk.judge_model(name, P, Q, captured, total)
    Y = chk.orth_input(1025, 33, "gauss")
    good = ref.orth32(Y)
    worse = good.copy()
    worse[:, 7] *= np.float32(1 + 1e-3)
    rec = chk.ORTH_DISTANCE[chk.orth_key(1025, 33, "gauss")]
    assert chk.judge_orth(worse, Y, rec) and not chk.judge_orth(good, Y, rec)
    lost = good.copy()
    lost[:, 7] = good[:, 6]  # a column of the span lost
    assert any("span" in c for c in chk.judge_orth(lost, Y, rec))
    # captured past total, biases left behind
    assert chk.judge_model(name, P, Q, total * 1.001, total)
    assert chk.judge_model(name, P, Q, captured, total, user_bias=np.array([0.0, 1e-9]))


def test_ml_small_experiment_in_float64():
    """Every user's last stored entry held out, f = 252, 8 sweeps from the library's seed-42 start, hits @10 of 610 users: the records
    of svd_checks, which the GPU test and the README are held to."""
    train, held = chk.ml_small()
    hits, P64, Q64 = chk.ml_small_run()
    P, Q, captured, total = ref.svd32(train, ref.start(train.cols, chk.ML_SMALL_F), chk.ML_SMALL_SWEEPS)
    dist = ref.score_distance(P, Q, P64, Q64)
    reach = chk.within_reach(chk.ML_SMALL_SVD_DISTANCE)
    hits32 = kref.hits_at(chk.lists_of(P.astype(np.float64) @ Q.astype(np.float64).T, train, chk.ML_SMALL_K), held)
    print("PureSVD f = %d, %d sweeps: %d hits @%d of %d users (float32 restatement: %d); distance %.3g; within reach: %d; share %.4f"
          % (chk.ML_SMALL_F, chk.ML_SMALL_SWEEPS, hits, chk.ML_SMALL_K, train.rows, hits32, dist, reach, captured / total))
    assert hits == chk.ML_SMALL_SVD_HITS and reach == chk.ML_SMALL_SVD_WITHIN_REACH
    assert chk.pinned(dist, chk.ML_SMALL_SVD_DISTANCE)
    assert abs(hits32 - hits) <= reach
