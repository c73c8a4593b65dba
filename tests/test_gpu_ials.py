"""Implicit-feedback alternating least squares on the GPU (cu2rec_model_als_implicit, cu2rec_model_implicit_objective,
cu2rec_train_implicit, bin/mf -m ials, bin/predict -I) against the float64 reference of tests/ials_reference64.py.

The bar for a solved row x against the float64 optimum x* of the same system, built from the same float32 state, is the
project's: max |x - x*| <= 1e-3 max(1, |x*|_inf).  tests/test_ials_cpu.py shows on the CPU that a float32 restatement of the
kernels' arithmetic meets it on every row judged here (at 3e-5 .. 9e-4 of the bar on the large sets, 0.19 on the small-partner
set) and that five deliberate mistakes in the model do not.  The judge itself lives in tests/ials_checks.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib
from conftest import ROOT, ml_small

import ials_checks as chk
import ials_reference64 as ref
from als_checks import model_from, random_state, same_bits
from ials_checks import HYPER, check_half_step, ials

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6


def _same_state(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(chk.cases()))
def test_half_step_matches_float64(name):
    """Widths 1, 8, 30, 31, 100, 126, 252 and both edges of every tile count (ials_checks.EDGE_WIDTHS) x rows of 1 .. 4,097
    entries (at 31, 95 and 252 also 64 x 1,024 + 1) on both sides, long item rows over one and two workspace batches, 40
    partners at f = 100, and the messy set (entries of 0, repeated pairs, rows without entries) at alpha 40 and 0, and partner
    matrices of exactly 1,024, 1,025 and 2,049 rows (the G0 tile edges)."""
    case = chk.cases()[name]
    model = model_from(case.state(), case.csr.global_bias)
    report = {}
    check_half_step(model, cu.DeviceCSR(case.csr), case.csr, case.side, case.hyper, case.alpha, report=report)
    print("%s: worst row at %.3g of the bar" % (name, max(report.values())))


def test_a_partner_nobody_names_moves_every_row():
    """Every partner row inside the CSR enters G0: changing one that no entry names changes every solved row; one past the CSR's
    cols changes nothing."""
    csr = chk.messy_set()
    f = 16
    P, Q, ub, ib = random_state(csr.rows, csr.cols + 2, f, 5)
    d = cu.DeviceCSR(csr)

    def solved(Qx):
        m = model_from((P, Qx, ub, ib), 0.0)
        assert m.ials(d, HYPER, 40.0, "users") == 0
        return m.download()[0]
    base = solved(Q)
    inside, outside = Q.copy(), Q.copy()
    inside[csr.cols - 1] += 1.0   # named by nobody, inside the CSR
    outside[csr.cols + 1] += 1.0  # a model row past the CSR
    rated = np.diff(csr.indptr) > 0
    moved = (solved(inside).view(np.uint32) != base.view(np.uint32)).any(axis=1)
    assert moved[rated].all() and not moved[~rated].any()
    assert same_bits(solved(outside), base)


def test_deterministic_and_independent_of_the_other_rows():
    csr = chk.chk.width_length_set()
    f = 100
    d = cu.DeviceCSR(csr)
    state = random_state(csr.rows, csr.cols, f, 77)
    runs = []
    for _ in range(2):
        m = model_from(state, 0.0)
        assert m.ials(d, HYPER, 40.0, "both", sweeps=2) == 0
        runs.append(m.download())
    assert _same_state(*runs), "two runs differ"
    # every user solved from a one-user CSR of the same cols equals the same user among all the others, bit for bit
    P0, Q0, ub0, ib0 = runs[0]
    batch = model_from(runs[0], 0.0)
    assert batch.ials(d, HYPER, 40.0, "users") == 0
    Pb = batch.download()[0]
    for u in list(range(14)) + [50, 211]:
        lo, hi = csr.indptr[u], csr.indptr[u + 1]
        one = api.HostCSR([0, hi - lo], csr.indices[lo:hi], csr.data[lo:hi], 1, csr.cols, 0.0)
        m = cu.Model(1, csr.cols, f, 0.0, P=P0[u:u + 1], Q=Q0, user_bias=ub0[u:u + 1], item_bias=ib0)
        assert m.ials(cu.DeviceCSR(one), HYPER, 40.0, "users") == 0
        assert same_bits(m.download()[0][0], Pb[u]), u


OBJECTIVE_TOLERANCE = 4 * chk.OBJECTIVE_RESTATEMENT_ERROR


@pytest.mark.parametrize("name", chk.OBJECTIVE_SETS)
def test_objective_matches_float64(name):
    """cu2rec_model_implicit_objective against the float64 objective, relative.  The tolerance is measured: the float32
    restatement of the objective (float32 Grams summed in the kernels' order, everything else float64:
    ials_reference64.objective_f32) is off by at most 4.7e-8 on these sets (tests/test_ials_cpu.py prints 3.69e-9, 2.25e-9,
    2.04e-9, 7.9e-11 on the first four and up to 4.68e-8 on the edge widths, listed beside ials_checks.OBJECTIVE_SETS); times 4 for
    the freedom in accumulation order: 1.88e-7."""
    case = chk.cases()[name]
    state = case.state()
    model = model_from(state, 0.0)
    got = model.implicit_objective(cu.DeviceCSR(case.csr), case.hyper, case.alpha)
    want = ref.objective(case.csr, state[0], state[1], case.hyper, case.alpha)
    print("%s: objective %.12g, float64 %.12g, off by %.3g" % (name, got, want, abs(got - want) / abs(want)))
    assert _same_state(model.download(), state)  # the model is only read
    assert abs(got - want) <= OBJECTIVE_TOLERANCE * abs(want), (name, got, want)


def _ml_small_train(f, hyper, alpha, sweeps):
    tr = cu.createSparseMatrix(ml_small())
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    states = [model.download()]
    for _ in range(sweeps):
        for side in ("users", "items"):
            assert model.ials(d, hyper, alpha, side) == 0
            states.append(model.download())
    return tr, states


def test_objective_never_rises_on_ml_small():
    hyper, alpha = (0.01, 0.1, 0.1, 0.0, 0.0), 40.0
    tr, states = _ml_small_train(32, hyper, alpha, 5)
    L = [ref.objective(tr, s[0], s[1], hyper, alpha) for s in states]
    for k in range(1, len(L)):
        assert L[k] <= L[k - 1], (k, L[k - 1], L[k])
    assert L[-1] < 0.5 * L[0]


def test_train_ials_equals_the_sweeps(capfd):
    tr, te = synth.make_ratings(300, 80, 5000, min_degree=2, seed=51)
    f, alpha = 12, 10.0
    cfg = api.default_config(total_iterations=5, n_factors=f, check_error=2, patience=0.0, learning_rate=0.125, P_reg=HYPER[1],
                             Q_reg=HYPER[2])
    capfd.readouterr()
    P, Q, objectives, ub, ib, stats = cu.train(tr, None, cfg, mode="ials", alpha=alpha, verbose=True, return_stats=True)
    out = capfd.readouterr().out
    assert cfg.learning_rate == np.float32(0.125) and cfg.cur_iterations == 5 and "New Learning Rate" not in out
    lines = [l for l in out.splitlines() if l.startswith("TRAIN:")]
    assert [l.split()[2] for l in lines] == ["1", "2", "4", "5"] and all("implicit objective" in l for l in lines), lines
    assert not [l for l in out.splitlines() if l.startswith("TEST:")]
    checked = [0, 1, 3, 4]
    assert objectives.dtype == np.float64 and np.isfinite(objectives[checked]).all() and np.isnan(np.delete(objectives, checked)).all()
    d = cu.DeviceCSR(tr)
    m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    hyper = (0.0, HYPER[1], HYPER[2], 0.0, 0.0)
    assert m.ials(d, hyper, alpha, "both", sweeps=5) == 0
    assert _same_state((P, Q, ub, ib), m.download())
    assert objectives[4] == m.implicit_objective(d, hyper, alpha)
    assert all(b <= a for a, b in zip(objectives[checked], objectives[checked][1:]))
    rows = int((np.diff(tr.indptr) > 0).sum()) + int((np.bincount(tr.indices, minlength=tr.cols) > 0).sum())
    assert stats.updates == 5 * rows
    # is_train = 0: the item side is frozen bit for bit
    cfg2 = api.default_config(total_iterations=2, n_factors=f, check_error=10, is_train=0, P_reg=HYPER[1], Q_reg=HYPER[2])
    P2, Q2, _, _, ib2 = cu.train(tr, None, cfg2, mode="ials", alpha=alpha, verbose=False)
    init = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    _, Q0, _, ib0 = init.download()
    assert same_bits(Q2, Q0) and same_bits(ib2, ib0)
    assert init.ials(d, hyper, alpha, "users") == 0
    assert same_bits(P2, init.download()[0])


def test_bin_mf_ials_and_predict_I(tmp_path):
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    tr0, te0 = synth.make_ratings(200, 50, 3000, min_degree=3, seed=61)
    synth.write_csv(str(tmp_path / "train.csv"), tr0)
    synth.write_csv(str(tmp_path / "test.csv"), te0)
    f = 8
    hyper = (0.01, 0.3, 0.2, 0.02, 0.03)
    (tmp_path / "c.cfg").write_text("0 4 %d 0.01 42 %g %g %g %g\n" % ((f,) + hyper[1:]))
    res = subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "ials", "-a", "10", "-k", "10", str(tmp_path / "train.csv"),
                          str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    assert "implicit objective" in res.stdout and "Precision@10" in res.stdout and "TEST: Iteration" not in res.stdout
    tr = cu.createSparseMatrix(str(tmp_path / "train.csv"))
    m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    assert m.ials(cu.DeviceCSR(tr), hyper, 10.0, "both", sweeps=4) == 0
    pre = str(tmp_path / ("train_f%d_" % f))
    for name, want in zip(("p", "q", "user_bias", "item_bias"), m.download()):
        got = cu.read_array(pre + name + ".csv").reshape(want.shape)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), name
    assert np.isclose(cu.read_array(pre + "global_bias.csv")[0, 0], tr.global_bias)
    assert subprocess.run([mf, "-c", str(tmp_path / "c.cfg"), "-m", "ials", "-g", "2", str(tmp_path / "train.csv"),
                           str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0

    # bin/predict -I 10 -u: one implicit user half-step against the frozen q.csv, then the usual ranking
    rng = np.random.default_rng(3)
    named = {uid: sorted(rng.choice(tr.cols, n, replace=False).tolist()) for uid, n in ((7, 6), (3, 1), (12, 9))}
    lines = ["userId,itemId,rating"]
    for uid in (3, 7, 12):
        lines += ["%d,%d,%.1f" % (uid, i + 1, rng.integers(1, 11) / 2) for i in named[uid]]
    (tmp_path / "many.csv").write_text("\n".join(lines) + "\n")
    k = 10
    args = [predict, "-c", str(tmp_path / "c.cfg"), "-i", pre + "item_bias.csv", "-g", pre + "global_bias.csv", "-q", pre + "q.csv"]
    out = subprocess.run(args + ["-I", "10", "-u", "-k", str(k), str(tmp_path / "many.csv")], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    assert subprocess.run(args + ["-I", "10", "-A", "-u", str(tmp_path / "many.csv")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE).returncode != 0
    users = cu.createSparseMatrix(str(tmp_path / "many.csv"))
    order = np.flatnonzero(np.diff(users.indptr) > 0)
    rows = [users.slice_users(int(u), int(u) + 1) for u in order]
    indptr = np.concatenate([[0], np.cumsum([r.nnz for r in rows])])
    fit = api.HostCSR(indptr, np.concatenate([r.indices for r in rows]), np.concatenate([r.data for r in rows]), len(rows), tr.cols)
    Qf, ibf = cu.read_array(pre + "q.csv"), cu.read_array(pre + "item_bias.csv").reshape(-1)
    gbf = float(cu.read_array(pre + "global_bias.csv")[0, 0])
    m2 = cu.Model(len(rows), tr.cols, f, gbf, P=np.zeros((len(rows), f), np.float32), Q=Qf, user_bias=np.zeros(len(rows), np.float32),
                  item_bias=ibf)
    dfit = cu.DeviceCSR(fit)
    assert m2.ials(dfit, hyper, 10.0, "users") == 0
    items, scores = m2.topk(dfit, k)
    blocks = out.split("User: ")[1:]
    assert [int(b.split("\n")[0]) for b in blocks] == [int(u) + 1 for u in order]
    for row, b in enumerate(blocks):
        got = [l.split("\t") for l in b.split("\n") if l.startswith("Rank:")]
        assert len(got) == k
        for j, fields in enumerate(got):
            assert abs(float(fields[2].split()[-1]) - scores[row, j]) <= 5e-7 + 1e-6 * abs(scores[row, j]), (row, j)
            assert int(fields[1].split()[1]) == items[row, j], (row, j)


def test_errors_leave_the_model_alone():
    tr, _ = synth.make_ratings(100, 40, 1500, min_degree=2, seed=41)
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, 8, tr.global_bias)
    before = model.download()
    lr, P_reg, Q_reg, ubr, ibr = HYPER
    cases = [((lr, 0.0, Q_reg, ubr, ibr), 40.0, "users"), ((lr, np.nan, Q_reg, ubr, ibr), 40.0, "users"),
             ((lr, -1.0, Q_reg, ubr, ibr), 40.0, "users"), ((lr, np.inf, Q_reg, ubr, ibr), 40.0, "users"),
             ((lr, P_reg, 0.0, ubr, ibr), 40.0, "items"), ((lr, P_reg, np.inf, ubr, ibr), 40.0, "items"),
             ((lr, P_reg, np.nan, ubr, ibr), 40.0, "items"),
             (HYPER, -1.0, "users"), (HYPER, np.nan, "items"), (HYPER, np.inf, "users"), (HYPER, 40.0, 2), (HYPER, 40.0, -1)]
    for hyper, alpha, side in cases:
        assert ials(model, d, hyper, alpha, side)[0] == EINVAL, (hyper, alpha, side)
    # the regulariser of the other side, the bias regularisers and the learning rate are not looked at
    assert ials(cu.Model(tr.rows, tr.cols, 8, 0.0), d, (np.nan, P_reg, np.nan, np.nan, -1.0), 40.0, "users") == (0, 0)
    h = cu.Hyper(*HYPER)
    L = lib()
    assert L.cu2rec_model_als_implicit(None, d._h, C.byref(h), 40.0, 0, None) == EINVAL
    assert L.cu2rec_model_als_implicit(model._h, None, C.byref(h), 40.0, 0, None) == EINVAL
    assert L.cu2rec_model_als_implicit(model._h, d._h, None, 40.0, 0, None) == EINVAL
    for small in (cu.Model(tr.rows, tr.cols - 1, 8, 0.0), cu.Model(tr.rows - 1, tr.cols, 8, 0.0)):  # entries past the model's shape
        kept = small.download()
        for side in ("users", "items"):
            assert ials(small, d, HYPER, 40.0, side)[0] == EINVAL
        assert _same_state(small.download(), kept)
    wide = cu.Model(tr.rows, tr.cols, 253, tr.global_bias)
    wide_before = wide.download()
    assert ials(wide, d, HYPER, 40.0, "users")[0] == EUNSUPPORTED
    with pytest.raises(cu.Cu2recError):
        wide.implicit_objective(d, HYPER, 40.0)
    assert _same_state(wide.download(), wide_before)
    with pytest.raises(cu.Cu2recError):
        model.implicit_objective(d, HYPER, -1.0)
    cfg = api.default_config(total_iterations=2, n_factors=8, P_reg=0.0)
    with pytest.raises(cu.Cu2recError):
        cu.train(tr, None, cfg, mode="ials", verbose=False)
    assert _same_state(model.download(), before)
    assert ials(model, d, HYPER, 40.0, "users") == (0, 0)  # and the same objects still work
