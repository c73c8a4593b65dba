"""Alternating least squares on the GPU (cu2rec_model_als, cu2rec_train with CU2REC_ALS, bin/mf -m als, bin/predict -A) against
the float64 reference of tests/als_reference64.py.

The bar for a solved row x (factors and bias) against the float64 optimum x* of the same system, built from the same float32
inputs: max |x - x*| <= 1e-3 max(1, |x*|_inf), and the float64 objective after the GPU half-step at most the optimum's (1 + 1e-6).
Rows the half-step does not own or cannot solve stay bit for bit.  That forward bar says little where a system is badly conditioned
and is loose where it is not: tests/test_gpu_als_edges.py also judges a row by its residual against the rounding bound derived in
als_reference64.row_residual.  The judge itself (_check_half_step) lives in tests/als_checks.py, shared with that file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib
from conftest import ROOT, ml_small

import als_reference64 as ref
from als_checks import HYPER, als as _als, bigger_model as _bigger_model, check_half_step as _check_half_step
from als_checks import rows_with_ratings as _rows_with_ratings

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6
_CACHE = {}


@pytest.mark.parametrize("f", [1, 3, 4, 31, 32, 33, 64, 100, 127, 128, 129, 200, 252])
def test_half_steps_match_float64(f):
    tr, _ = synth.make_ratings(240, 90, 4000, min_degree=1, seed=100 + f)
    d = cu.DeviceCSR(tr)
    model = _bigger_model(tr, f)
    _check_half_step(model, d, tr, "users")  # at initialisation
    _check_half_step(model, d, tr, "items")
    assert model.als(d, HYPER, "both", sweeps=2) == 0
    _check_half_step(model, d, tr, "users")  # after two sweeps
    _check_half_step(model, d, tr, "items")


def _lengths():
    s, c, m = api.ALS_STEP, api.ALS_CHUNK, api.ALS_MAX_CHUNKS
    out = [1, 2]
    for t in (s, c, 2 * c, m * c):  # stage, chunk, first multi-chunk and chunk-count cap boundaries
        out += [t - 1, t, t + 1]
    return out


def _threshold_set():
    """User i has the i-th length of _lengths() (distinct items); plus users of 1 rating."""
    if "thr" not in _CACHE:
        rng = np.random.default_rng(7)
        lengths = _lengths() + [1, 1, 3]
        cols = max(lengths) + 40
        indptr = np.zeros(len(lengths) + 1, np.int64)
        indptr[1:] = np.cumsum(lengths)
        items = np.concatenate([np.sort(rng.choice(cols, n, replace=False)) for n in lengths]).astype(np.int32)
        ratings = rng.integers(1, 11, len(items)).astype(np.float32) / 2
        gb = float(np.float32(ratings.astype(np.float64).mean()))
        _CACHE["thr"] = api.HostCSR(indptr, items, ratings, len(lengths), cols, gb)
    return _CACHE["thr"]


def test_length_thresholds_users():
    tr = _threshold_set()
    d = cu.DeviceCSR(tr)
    model = _bigger_model(tr, 4)
    _check_half_step(model, d, tr, "users")
    _check_half_step(model, d, tr, "items")
    _check_half_step(model, d, tr, "users")


def test_item_rated_by_every_user_of_70k():
    """70,000 users; item 0 rated by all of them (past the chunk-count cap), items 1.. at every threshold length."""
    rng = np.random.default_rng(8)
    n_users = 70_000
    lengths = [n_users] + [n for n in _lengths() if n < n_users]
    per_user = [[] for _ in range(n_users)]
    for item, n in enumerate(lengths):
        for u in (np.arange(n) if n == n_users else rng.choice(n_users, n, replace=False)):
            per_user[u].append(item)
    indptr = np.zeros(n_users + 1, np.int64)
    indptr[1:] = np.cumsum([len(p) for p in per_user])
    items = np.concatenate([np.array(sorted(p), np.int32) for p in per_user])
    ratings = rng.integers(1, 11, len(items)).astype(np.float32) / 2
    tr = api.HostCSR(indptr, items, ratings, n_users, len(lengths), float(np.float32(ratings.mean())))
    d = cu.DeviceCSR(tr)
    model = _bigger_model(tr, 8)
    _check_half_step(model, d, tr, "items")
    _check_half_step(model, d, tr, "users")
    _check_half_step(model, d, tr, "items")


def test_deterministic_and_independent_of_the_batch():
    tr = _threshold_set()
    f = 100
    d = cu.DeviceCSR(tr)
    runs = []
    for _ in range(2):
        m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        assert m.als(d, HYPER, "both", sweeps=2) == 0
        assert m.als(d, HYPER, "users") == 0
        runs.append(m.download())
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs differ"
    # every user fitted alone (a one-user CSR against the same items) equals the same user in the batch, bit for bit
    P0, Q0, ub0, ib0 = runs[0]
    batch = cu.Model(tr.rows, tr.cols, f, tr.global_bias, P=P0, Q=Q0, user_bias=ub0, item_bias=ib0)
    assert batch.als(d, HYPER, "users") == 0
    Pb, _, ubb, _ = batch.download()
    for u in range(tr.rows):
        lo, hi = tr.indptr[u], tr.indptr[u + 1]
        one = api.HostCSR([0, hi - lo], tr.indices[lo:hi], tr.data[lo:hi], 1, tr.cols, tr.global_bias)
        m = cu.Model(1, tr.cols, f, tr.global_bias, P=P0[u:u + 1], Q=Q0, user_bias=ub0[u:u + 1], item_bias=ib0)
        assert m.als(cu.DeviceCSR(one), HYPER, "users") == 0
        P1, _, ub1, _ = m.download()
        assert np.array_equal(P1[0], Pb[u]) and ub1[0] == ubb[u], u


def _ml_small_split():
    if "ml" not in _CACHE:
        full = cu.createSparseMatrix(ml_small())
        pos = np.arange(full.nnz) - np.repeat(full.indptr[:-1], np.diff(full.indptr))
        test = pos % 5 == 4  # every fifth rating of each user
        users = np.repeat(np.arange(full.rows), np.diff(full.indptr))

        def part(mask):
            indptr = np.zeros(full.rows + 1, np.int64)
            indptr[1:] = np.cumsum(np.bincount(users[mask], minlength=full.rows))
            return api.HostCSR(indptr, full.indices[mask], full.data[mask], full.rows, full.cols, full.global_bias)
        _CACHE["ml"] = (part(~test), part(test))
    return _CACHE["ml"]


def _ml_small_run():
    """10 sweeps at f = 32 on ML_SMALL: the GPU state after every half-step, from the seed-42 initial model."""
    if "ml_run" not in _CACHE:
        tr, te = _ml_small_split()
        d = cu.DeviceCSR(tr)
        model = cu.Model(tr.rows, tr.cols, 32, tr.global_bias)
        states = [model.download()]
        for _ in range(10):
            for side in ("users", "items"):
                assert model.als(d, HYPER, side) == 0
                states.append(model.download())
        _CACHE["ml_run"] = states
    return _CACHE["ml_run"]


def test_objective_never_rises_on_ml_small():
    tr, _ = _ml_small_split()
    L = [ref.objective(tr, *s, tr.global_bias, HYPER) for s in _ml_small_run()]
    for k in range(1, len(L)):
        assert L[k] <= L[k - 1] * (1 + 1e-6), (k, L[k - 1], L[k])
    assert L[-1] < L[0]


def test_trajectory_matches_float64_on_ml_small():
    tr, te = _ml_small_split()
    states = _ml_small_run()
    *_, curve = ref.run(tr, *states[0], tr.global_bias, HYPER, 10, test=te)
    for sweep in range(10):
        got = ref.rmse(te, *states[2 * sweep + 2], tr.global_bias)
        assert abs(got - curve[sweep]) <= 1e-4, (sweep, got, curve[sweep])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_item_row_leaves_its_users_unchanged(bad):
    tr, _ = synth.make_ratings(200, 60, 3000, min_degree=2, seed=31)
    f = 16
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    P, Q, ub, ib = model.download()
    j = int(np.bincount(tr.indices, minlength=tr.cols).argmax())
    Q[j, 3] = bad
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias, P=P, Q=Q, user_bias=ub, item_bias=ib)
    rc, unsolved = _als(model, cu.DeviceCSR(tr), HYPER, "users")
    assert rc == 0
    users = np.repeat(np.arange(tr.rows), np.diff(tr.indptr))
    raters = np.unique(users[tr.indices == j])
    assert unsolved == len(raters) > 0
    Pg, Qg, ubg, ibg = model.download()
    assert np.array_equal(Pg[raters], P[raters]) and np.array_equal(ubg[raters], ub[raters])
    assert np.array_equal(Qg, Q, equal_nan=True) and np.array_equal(ibg, ib)
    Qz = Q.copy()
    Qz[j] = 0.0  # (only the raters of item j read it, and they are checked above)
    want = ref.half_step(tr, P, Qz, ub, ib, tr.global_bias, HYPER, "users")
    others = np.setdiff1d(_rows_with_ratings(tr, "users"), raters)
    x = np.concatenate([Pg[others], ubg[others, None]], axis=1).astype(np.float64)
    xs = np.concatenate([want[0][others], want[2][others, None]], axis=1)
    assert (np.abs(x - xs).max(axis=1) <= 1e-3 * np.maximum(1.0, np.abs(xs).max(axis=1))).all()


def test_errors_leave_the_model_alone():
    tr, _ = synth.make_ratings(100, 40, 1500, min_degree=2, seed=41)
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, 8, tr.global_bias)
    before = model.download()
    lr, P_reg, Q_reg, ubr, ibr = HYPER
    cases = [((lr, 0.0, Q_reg, ubr, ibr), "users"), ((lr, np.nan, Q_reg, ubr, ibr), "users"), ((lr, -1.0, Q_reg, ubr, ibr), "users"),
             ((lr, P_reg, 0.0, ubr, ibr), "items"), ((lr, P_reg, np.inf, ubr, ibr), "items"),
             ((lr, P_reg, Q_reg, -0.5, ibr), "users"), ((lr, P_reg, Q_reg, np.nan, ibr), "users"),
             ((lr, P_reg, Q_reg, ubr, -0.5), "items"), ((lr, P_reg, Q_reg, ubr, np.nan), "items")]
    for hyper, side in cases:
        assert _als(model, d, hyper, side)[0] == EINVAL, (hyper, side)
    h = cu.Hyper(*HYPER)
    for side in (2, -1):
        assert lib().cu2rec_model_als(model._h, d._h, C.byref(h), side, None) == EINVAL
    small = cu.Model(tr.rows, tr.cols - 1, 8, tr.global_bias)  # ratings past the model's items
    if tr.indices.max() == tr.cols - 1:
        assert _als(small, d, HYPER, "users")[0] == EINVAL
    wide = cu.Model(tr.rows, tr.cols, 253, tr.global_bias)
    wide_before = wide.download()
    assert _als(wide, d, HYPER, "users")[0] == EUNSUPPORTED
    for a, b in zip(wide.download(), wide_before):
        assert np.array_equal(a, b)
    for a, b in zip(model.download(), before):
        assert np.array_equal(a, b)
    with pytest.raises(cu.Cu2recError):
        model.sgd(d, HYPER, 42, 0, 1, mode="als")
    for a, b in zip(model.download(), before):
        assert np.array_equal(a, b)


def test_train_with_als(capfd):
    tr, te = synth.make_ratings(300, 80, 5000, min_degree=2, seed=51)
    f = 12
    cfg = api.default_config(total_iterations=5, n_factors=f, check_error=2, patience=0.0, learning_rate=0.125,
                             P_reg=HYPER[1], Q_reg=HYPER[2], user_bias_reg=HYPER[3], item_bias_reg=HYPER[4])
    capfd.readouterr()
    P, Q, losses, ub, ib, stats = cu.train(tr, te, cfg, mode="als", verbose=True, return_stats=True)
    out = capfd.readouterr().out
    assert cfg.learning_rate == np.float32(0.125) and cfg.cur_iterations == 5
    assert "New Learning Rate" not in out
    lines = [l for l in out.splitlines() if l.startswith(("TRAIN:", "TEST:"))]
    assert [l.split()[2] for l in lines] == ["1", "1", "2", "2", "4", "4", "5", "5"], lines
    checked = [0, 1, 3, 4]
    assert np.isfinite(losses[checked]).all() and np.isnan(np.delete(losses, checked)).all()
    # the same as five sweeps of Model.als from the same initial model
    d = cu.DeviceCSR(tr)
    m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    assert m.als(d, HYPER, "both", sweeps=5) == 0
    for a, b in zip((P, Q, ub, ib), m.download()):
        assert np.array_equal(a, b)
    assert losses[4] == np.float32(m.loss(cu.DeviceCSR(te))["rmse"])
    rows = len(_rows_with_ratings(tr, "users")) + len(_rows_with_ratings(tr, "items"))
    assert stats.updates == 5 * rows
    # is_train = 0: the item side is frozen bit for bit; the users are their half-step against it
    cfg2 = api.default_config(total_iterations=3, n_factors=f, check_error=10, is_train=0, P_reg=HYPER[1], Q_reg=HYPER[2],
                              user_bias_reg=HYPER[3], item_bias_reg=HYPER[4])
    P2, Q2, _, ub2, ib2 = cu.train(tr, te, cfg2, mode="als", verbose=False)
    init = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    P0, Q0, ub0, ib0 = init.download()
    assert np.array_equal(Q2, Q0) and np.array_equal(ib2, ib0)
    assert init.als(d, HYPER, "users") == 0
    Pw, _, ubw, _ = init.download()
    assert np.array_equal(P2, Pw) and np.array_equal(ub2, ubw)


def test_bin_mf_als_and_predict_A(tmp_path):
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    tr0, te0 = synth.make_ratings(200, 50, 3000, min_degree=3, seed=61)
    synth.write_csv(str(tmp_path / "train.csv"), tr0)
    synth.write_csv(str(tmp_path / "test.csv"), te0)
    f = 8
    (tmp_path / "c.cfg").write_text("0 4 %d 0.01 42 %g %g %g %g\n" % ((f,) + HYPER[1:]))
    res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "als", "-k", "5", str(tmp_path / "train.csv"),
                          str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    assert "New Learning Rate" not in res.stdout and "Precision@5" in res.stdout
    tr = cu.createSparseMatrix(str(tmp_path / "train.csv"))
    m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    assert m.als(cu.DeviceCSR(tr), HYPER, "both", sweeps=4) == 0
    pre = str(tmp_path / ("train_f%d_" % f))
    for name, want in zip(("p", "q", "user_bias", "item_bias"), m.download()):
        got = cu.read_array(pre + name + ".csv").reshape(want.shape)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), name
    assert np.isclose(cu.read_array(pre + "global_bias.csv")[0, 0], tr.global_bias)
    # several GPUs and too many factors are refused
    assert subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "als", "-g", "2", str(tmp_path / "train.csv"),
                           str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0
    (tmp_path / "wide.cfg").write_text("0 2 253 0.01 42 0.05 0.05 0.02 0.02\n")
    assert subprocess.run([mf, "-c", str(tmp_path / "wide.cfg"), "-m", "als", str(tmp_path / "train.csv"),
                           str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0

    # bin/predict -A -u: a user half-step against the model's frozen items, then the usual ranking
    (tmp_path / "p.cfg").write_text("0 30 %d 0.05 42 %g %g %g %g\n" % ((f,) + HYPER[1:]))
    rng = np.random.default_rng(3)
    ratings = {uid: sorted(rng.choice(tr.cols, n, replace=False).tolist()) for uid, n in ((7, 6), (3, 1), (12, 9))}
    lines = ["userId,itemId,rating"]
    for uid in (3, 7, 12):  # grouped by ascending user, as the ratings reader wants
        lines += ["%d,%d,%.1f" % (uid, i + 1, rng.integers(1, 11) / 2) for i in ratings[uid]]
    (tmp_path / "many.csv").write_text("\n".join(lines) + "\n")
    k = 10
    out = subprocess.run([predict, "-c", str(tmp_path / "p.cfg"), "-i", pre + "item_bias.csv", "-g", pre + "global_bias.csv", "-q",
                          pre + "q.csv", "-A", "-u", "-k", str(k), str(tmp_path / "many.csv")], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    users = cu.createSparseMatrix(str(tmp_path / "many.csv"))
    keep = np.diff(users.indptr) > 0  # the file's users 3, 7, 12 in ascending id order
    order = np.flatnonzero(keep)
    rows = [users.slice_users(int(u), int(u) + 1) for u in order]
    indptr = np.concatenate([[0], np.cumsum([r.nnz for r in rows])])
    fit = api.HostCSR(indptr, np.concatenate([r.indices for r in rows]), np.concatenate([r.data for r in rows]), len(rows), tr.cols)
    Qf, ibf = cu.read_array(pre + "q.csv"), cu.read_array(pre + "item_bias.csv").reshape(-1)
    gbf = float(cu.read_array(pre + "global_bias.csv")[0, 0])
    m2 = cu.Model(len(rows), tr.cols, f, gbf, P=np.zeros((len(rows), f), np.float32), Q=Qf, user_bias=np.zeros(len(rows), np.float32),
                  item_bias=ibf)
    dfit = cu.DeviceCSR(fit)
    assert m2.als(dfit, HYPER, "users") == 0
    items, scores = m2.topk(dfit, k)
    blocks = out.split("User: ")[1:]
    assert [int(b.split("\n")[0]) for b in blocks] == [int(u) + 1 for u in order]
    for row, b in enumerate(blocks):
        got = [l.split("\t") for l in b.split("\n") if l.startswith("Rank:")]
        assert len(got) == k
        for j, fields in enumerate(got):
            assert fields[0] == "Rank: %d" % (j + 1)
            assert abs(float(fields[2].split()[-1]) - scores[row, j]) <= 5e-7 + 1e-6 * abs(scores[row, j]), (row, j)
            assert int(fields[1].split()[1]) == items[row, j], (row, j)
