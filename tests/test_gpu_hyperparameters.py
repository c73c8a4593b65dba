"""Every SGD mode with distinct, non-default hyper-parameters (-m gpu).

The rest of the suite trains with lr 0.01 and all four regularisers equal (0.02), so an exchange of two of the constants anywhere
between the configuration and a kernel -- P_reg with Q_reg, user_bias_reg with item_bias_reg, the block-solve decay tables of
a = 1 - lr Q_reg with those of c = 1 - lr item_bias_reg -- gives the same bits on both sides of those tests.  Here each mode runs
the sets of SETS (lr, P_reg, Q_reg, user_bias_reg, item_bias_reg) against the CPU oracle (TREE16 dot order, the kernels' own):
  * serial, ordered, ping-pong (both buffer pairs), Hogwild on a collision-free set and with the item side frozen, the resident
    Hogwild launch (one launch; partial residency) -- bit for bit;
  * block-solve within 2e-6 at the shapes of test_gpu_blocksolve.py (f = 1 / 100 / 252, every item hot, the loader's ring, the
    look-ahead form); where a set's lr * Q_reg or lr * item_bias_reg reaches 1 the mode runs the ordered walk: bit for bit;
  * successive block-solve calls on one schedule that change one constant at a time (the decay tables are cached per schedule);
  * train() in three modes, bin/mf (-m serial byte for byte, its default mode within 2e-6), bin/predict's partial fit.
Block-solve stayed within 2.7e-7 of the oracle in every case, the large learning rates (0.05 .. 0.1) included; had a case gone
above 2e-6, the float64 reference (tests/sgd_reference64.py) would have had to show which of the two float32 paths is farther.
Before block-solve fell back to the ordered walk for a <= 0 or c <= 0, all twelve a_zero / a_negative block-solve cases came back NaN
(the cross-tile terms lr (c^d + a^d ...) are evaluated as exp2(d log2 a): 0 * -inf at d = 0, NaN for a < 0)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib
from conftest import GOLDEN, ROOT
from oracle import oracle as orc
from test_gpu_resident import FORCE, _collision_free_set, resident_policy

pytestmark = pytest.mark.gpu

SETS = {
    "distinct": (0.01, 0.015, 0.03, 0.045, 0.08),      # a^64 ~ 0.981 against c^64 ~ 0.950
    "ref_train_cfg": (0.1, 0.2, 0.1, 0.1, 0.1),        # the reference's data/test/train.cfg
    "ref_test_sgd": (0.07, 0.1, 0.1, 0.1, 0.1),        # the reference's tests/test_sgd.cu
    "strong_decay": (0.05, 0.02, 0.4, 0.05, 1.0),      # c^126 ~ 0.0016: the bottom of the decay tables
    "no_reg": (0.01, 0.0, 0.0, 0.0, 0.0),              # a = c = 1, log2 = 0
    "lr_zero": (0.0, 0.02, 0.03, 0.04, 0.05),          # nothing moves
    "a_zero": (0.5, 0.02, 2.0, 0.02, 2.0),             # lr * Q_reg = lr * item_bias_reg = 1
    "a_negative": (0.5, 0.02, 3.0, 0.02, 0.5),         # a = -0.5
}
NAMES = list(SETS)
DISTINCT = SETS["distinct"]


def _iters(name, n=3):
    return 2 if name.startswith("a_") else n  # a <= 0: large steps, few iterations


def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


def _assert_equal(got, want, what=""):
    for name, g, w in zip(("P", "Q", "user_bias", "item_bias"), got, want):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


def _oracle(m, f, hyper, iter0, iters, update_items=True, state=None):
    state = state or orc.init_model(m.rows, m.cols, f)
    orc.sgd_iterations(_as_orc(m), *state, m.global_bias, hyper, 42, iter0, iters, dot_order=orc.DOT_TREE16, update_items=update_items)
    assert all(np.isfinite(a).all() for a in state), "the oracle itself is not finite"
    return state


def _check_lr_zero(name, got, m, f):
    if SETS[name][0] == 0.0:  # lr = 0: every parameter is bit for bit its initial value
        _assert_equal(got, orc.init_model(m.rows, m.cols, f), "lr = 0")


@pytest.fixture
def min_rate():
    prev = api.blocksolve_min_rate()
    yield api.blocksolve_min_rate
    api.blocksolve_min_rate(prev)


_SETS = {}


def _small():
    if "tr" not in _SETS:
        _SETS["tr"] = synth.make_ratings(400, 600, 4000, min_degree=3, seed=21)[0]  # 600 items: the ordered walk runs beside the 256 hot chains
    return _SETS["tr"]


# ------------------------------------------------------------------ exact modes

@pytest.mark.parametrize("name", NAMES)
def test_serial_ordered_and_pingpong_bit_exact(name):
    hyper, tr, f = SETS[name], _small(), 20
    iters = _iters(name)
    d = cu.DeviceCSR(tr)
    want = _oracle(tr, f, hyper, 5, iters)
    for mode in ("serial", "ordered"):
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(d, hyper, 42, 5, iters, mode=mode)
        _assert_equal(model.download(), want, mode)
        _check_lr_zero(name, model.download(), tr, f)
    for n in (iters, iters + 1):  # odd / even: the current item side in either buffer pair
        P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
        Qt, ibt = Q.copy(), ib.copy()
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(d, hyper, 42, 0, n, mode="pingpong")
        orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, hyper, 42, 0, n, dot_order=orc.DOT_TREE16)
        assert all(np.isfinite(a).all() for a in (P, Q, ub, ib))
        _assert_equal(model.download(), (P, Q, ub, ib), "pingpong %d" % n)
        _check_lr_zero(name, model.download(), tr, f)


@pytest.mark.parametrize("name", NAMES)
def test_hogwild_bit_exact_where_no_update_races(name):
    hyper, f = SETS[name], 20
    iters = _iters(name)
    n = 300
    rng = np.random.RandomState(3)  # every user rates only its own item
    m = cu.HostCSR(np.arange(n + 1), rng.permutation(n), rng.randint(1, 6, n).astype(np.float32), n, n, 3.0)
    prev = lib().cu2rec_hogwild_resident(0)  # streaming launches
    try:
        model = cu.Model(n, n, f, 3.0)
        model.sgd(cu.DeviceCSR(m), hyper, 42, 0, iters, mode="hogwild")
        _assert_equal(model.download(), _oracle(m, f, hyper, 0, iters), "hogwild")
        tr = _small()  # item side frozen: users share nothing
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(cu.DeviceCSR(tr), hyper, 42, 0, iters, mode="hogwild", update_items=False)
        _assert_equal(model.download(), _oracle(tr, f, hyper, 0, iters, update_items=False), "hogwild frozen items")
        _check_lr_zero(name, model.download(), tr, f)
    finally:
        lib().cu2rec_hogwild_resident(prev)


def _resident_run(m, f, hyper, iter0, chunks):
    model = cu.Model(m.rows, m.cols, f, m.global_bias)
    d = cu.DeviceCSR(m)
    with resident_policy(FORCE):
        it = iter0
        for n in chunks:
            model.sgd(d, hyper, 42, it, n, mode="hogwild")
            it += n
    return model.download()


@pytest.mark.parametrize("name", NAMES)
def test_resident_one_launch_bit_exact(name):
    """A grid smaller than the chip, every iteration of the call in one launch (the case of test_resident_every_row_width)."""
    hyper, f, users = SETS[name], 8, 700
    iters = _iters(name, 4)
    m = _collision_free_set(users, 2 * users + 64, 4, 7, iters, seed=f)
    with resident_policy(FORCE):
        assert lib().cu2rec_hogwild_resident_plan(users, f, iters, None, None) == 1
    _assert_equal(_resident_run(m, f, hyper, 7, [iters]), _oracle(m, f, hyper, 7, iters), "resident")


def test_resident_partial_residency_bit_exact_with_distinct_constants():
    """82,000 users at f = 256: three rows per group stream through the pipeline from and to memory."""
    f, users = 256, 82000
    assert lib().cu2rec_hogwild_resident_streamed_rows(users, f, 256) == 3
    m = _collision_free_set(users, 2 * users + 64, 3, 5, 4, seed=9, empty_every=53)
    _assert_equal(_resident_run(m, f, DISTINCT, 5, [2, 2]), _oracle(m, f, DISTINCT, 5, 4), "partial residency")


# ------------------------------------------------------------------ block-solve

# (users, items, nnz, f, iters, rate, look-ahead blocks): shapes of test_blocksolve_matches_sequential_oracle and of the look-ahead test;
# fewer iterations
BS_SHAPES = {
    "f1": (300, 120, 6000, 1, 3, 2.0, 0),
    "f100": (300, 120, 6000, 100, 3, 2.0, 0),
    "f252": (2000, 300, 40000, 252, 2, 4.0, 0),
    "all_hot": (500, 50, 5000, 8, 4, 0.01, 0),
    "ring": (9000, 6, 40000, 100, 2, 1.0, 0),
    "lookahead": (9000, 6, 40000, 100, 2, 1.0, 10),
}


def _blocksolve_run(shape, hyper, name):
    users, items, nnz, f, iters, rate, la = BS_SHAPES[shape]
    iters = _iters(name, iters)
    tr, _ = synth.make_ratings(users, items, nnz, min_degree=3, seed=users + f)
    prev_la = api.blocksolve_lookahead_blocks(la)
    try:
        api.blocksolve_min_rate(rate)
        d = cu.DeviceCSR(tr)  # (the schedule is created here: it reads both settings)
        assert d.blocksolve_items() > 0
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(d, hyper, 42, 0, iters, mode="blocksolve")
    finally:
        api.blocksolve_lookahead_blocks(prev_la)
    got = model.download()
    assert all(np.isfinite(a).all() for a in got), "block-solve result is not finite"
    return tr, f, iters, got


@pytest.mark.parametrize("shape", list(BS_SHAPES))
@pytest.mark.parametrize("name", NAMES)
def test_blocksolve_against_the_sequential_oracle(min_rate, name, shape):
    hyper = SETS[name]
    tr, f, iters, got = _blocksolve_run(shape, hyper, name)
    want = _oracle(tr, f, hyper, 0, iters)
    lr, _, q_reg, _, ib_reg = (float(np.float32(h)) for h in hyper)
    if 1.0 - lr * q_reg <= 0.0 or 1.0 - lr * ib_reg <= 0.0:  # no block form: the ordered walk
        _assert_equal(got, want, "a <= 0")
        return
    _check_lr_zero(name, got, tr, f)
    diffs = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want)]
    assert max(diffs) <= 2e-6, diffs  # float rounding of re-associated sums (measured: 2.7e-7 at most over these cases)


def test_blocksolve_decay_tables_follow_every_constant(min_rate):
    """One schedule, one model: successive calls whose constants differ in Q_reg only, then item_bias_reg only, then lr only, then
    P_reg and user_bias_reg; the oracle runs the same sequence.  A decay table kept from an earlier call is off by far more."""
    min_rate(1.0)
    tr, _ = synth.make_ratings(3000, 40, 30000, min_degree=3, seed=3040)
    f = 20
    d = cu.DeviceCSR(tr)
    assert d.blocksolve_items() > 0
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    state = orc.init_model(tr.rows, tr.cols, f)
    steps = [DISTINCT, (0.01, 0.015, 0.06, 0.045, 0.08), (0.01, 0.015, 0.06, 0.045, 0.16), (0.02, 0.015, 0.06, 0.045, 0.16),
             (0.02, 0.03, 0.06, 0.09, 0.16)]
    it = 0
    for k, hyper in enumerate(steps):
        model.sgd(d, hyper, 42, it, 2, mode="blocksolve")
        orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, hyper, 42, it, 2, dot_order=orc.DOT_TREE16)
        it += 2
        diffs = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)]
        assert max(diffs) <= 2e-6, (k, hyper, diffs)


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize("mode", ["serial", "ordered", "blocksolve"])
def test_train_with_distinct_constants_follows_the_oracle_schedule(min_rate, mode):
    """cu2rec_train with distinct regularisers and lr 0.05, which the patience schedule decays to 0.01 on this set (the shapes of
    test_train_schedule_matches_oracle and test_train_in_blocksolve_mode_follows_the_oracle_schedule)."""
    min_rate(1.0)
    if mode == "blocksolve":
        tr, te = synth.make_ratings(3000, 60, 40000, min_degree=3, seed=17)
        kw = dict(total_iterations=48, n_factors=20, check_error=8)
    else:
        tr, te = synth.make_ratings(300, 120, 6000, min_degree=3, seed=5)
        kw = dict(total_iterations=40, n_factors=10, check_error=8)
    kw.update(learning_rate=0.05, patience=1.0, P_reg=DISTINCT[1], Q_reg=DISTINCT[2], user_bias_reg=DISTINCT[3],
              item_bias_reg=DISTINCT[4])
    cfg, ocfg = cu.default_config(**kw), orc.default_config(**kw)
    f = kw["n_factors"]
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    log = orc.train(_as_orc(tr), _as_orc(te), ocfg, P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_TREE16, acc=orc.ACC_F64,
                    schedule=orc.SCHED_PATIENCE)
    gP, gQ, losses, gub, gib = cu.train(tr, te, cfg, mode=mode, verbose=False)
    assert log[0]["lr"] > log[-1]["lr"]  # the schedule decayed the rate
    assert cfg.learning_rate == ocfg.learning_rate and cfg.cur_iterations == ocfg.cur_iterations
    for e in log:
        if mode == "blocksolve":
            assert abs(float(losses[e["iteration"] - 1]) - e["test_rmse"]) <= 2e-6
        else:
            assert losses[e["iteration"] - 1] == e["test_rmse"]
    for g, w in ((gP, P), (gQ, Q), (gub, ub), (gib, ib)):
        if mode == "blocksolve":
            assert float(np.abs(g.astype(np.float64) - w).max()) <= 5e-6  # the bound of the blocksolve train test
        else:
            np.testing.assert_array_equal(g, w)


_LINE = re.compile(r"^(TRAIN|TEST): Iteration (\d+) GPU MAE: (\S+) RMSE: (\S+)$", re.M)


def _bin_mf(tmp_path, tr, te, cfg_line, f, mode=None, env=None):
    synth.write_csv(str(tmp_path / "train.csv"), tr)
    synth.write_csv(str(tmp_path / "test.csv"), te)
    (tmp_path / "c.cfg").write_text(cfg_line + "\n")
    cmd = [os.path.join(ROOT, "bin", "mf"), "-c", str(tmp_path / "c.cfg")] + (["-m", mode] if mode else [])
    out = subprocess.run(cmd + [str(tmp_path / "train.csv"), str(tmp_path / "test.csv")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})), timeout=300)
    assert out.returncode == 0, out.stderr
    assert "n_factors: %d" % f in out.stdout
    return out.stdout


def test_bin_mf_serial_with_distinct_constants_is_the_oracle_byte_for_byte(tmp_path):
    """bin/mf -m serial with a config file carrying distinct constants: its TRAIN / TEST lines and the five CSV files are the
    oracle's run of the same configuration, byte for byte."""
    tr, te = synth.make_ratings(300, 120, 6000, min_degree=3, seed=5)
    f, cfg_line = 8, "0 20 8 0.05 42 0.015 0.03 0.045 0.08"
    stdout = _bin_mf(tmp_path, tr, te, cfg_line, f, mode="serial")
    (tmp_path / "o.cfg").write_text(cfg_line + "\n")
    ocfg = orc.read_config(str(tmp_path / "o.cfg"))
    assert (ocfg.learning_rate, ocfg.P_reg, ocfg.Q_reg, ocfg.user_bias_reg, ocfg.item_bias_reg) == tuple(
        float(np.float32(v)) for v in (0.05, 0.015, 0.03, 0.045, 0.08))
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    log = orc.train(_as_orc(tr), _as_orc(te), ocfg, P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_TREE16, acc=orc.ACC_F64,
                    schedule=orc.SCHED_PATIENCE)
    want = []
    for e in log:
        want.append("TRAIN: Iteration %d GPU MAE: %f RMSE: %f" % (e["iteration"], e["train_mae"], e["train_rmse"]))
        want.append("TEST: Iteration %d GPU MAE: %f RMSE: %f" % (e["iteration"], e["test_mae"], e["test_rmse"]))
    assert [m.group(0) for m in _LINE.finditer(stdout)] == want
    for comp, arr in (("p", P), ("q", Q), ("user_bias", ub), ("item_bias", ib)):
        orc.write_csv(str(tmp_path / "want.csv"), arr)
        assert (tmp_path / ("train_f8_%s.csv" % comp)).read_text() == (tmp_path / "want.csv").read_text(), comp
    assert (tmp_path / "train_f8_global_bias.csv").read_text() == "%f\n" % tr.global_bias


def test_bin_mf_default_mode_with_distinct_constants_follows_the_oracle(tmp_path):
    """bin/mf without -m: block-solve at this width (CU2REC_BLOCKSOLVE_RATE makes items hot on this small set).  The written
    factors within 2e-6 of the oracle's, plus the 5e-7 of the files' six decimals."""
    tr, te = synth.make_ratings(3000, 60, 40000, min_degree=3, seed=31)
    f, cfg_line = 16, "0 10 16 0.01 42 0.015 0.03 0.045 0.08"
    _bin_mf(tmp_path, tr, te, cfg_line, f, env={"CU2REC_BLOCKSOLVE_RATE": "1.0"})
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(_as_orc(tr), P, Q, ub, ib, tr.global_bias, DISTINCT, 42, 0, 10, dot_order=orc.DOT_TREE16)
    for comp, want in (("p", P), ("q", Q), ("user_bias", ub), ("item_bias", ib)):
        got = np.loadtxt(str(tmp_path / ("train_f16_%s.csv" % comp)), delimiter=",", ndmin=2).reshape(want.shape)
        assert float(np.abs(got - want).max()) <= 2e-6 + 5e-7, comp


def test_bin_predict_partial_fit_with_distinct_user_constants(tmp_path):
    """bin/predict fits one new user with the item side frozen: P_reg and user_bias_reg distinct (test_bin_predict_partial_fit)."""
    mf, predict = os.path.join(ROOT, "bin", "mf"), os.path.join(ROOT, "bin", "predict")
    train = tmp_path / "ratings.csv"
    train.write_text(open(os.path.join(GOLDEN, "toy_ratings.csv")).read())
    (tmp_path / "train.cfg").write_text("0 50 4 0.05 42 0.02 0.02 0.02 0.02\n")
    subprocess.run([mf, "-c", str(tmp_path / "train.cfg"), "-m", "ordered", str(train), os.path.join(GOLDEN, "toy_ratings2.csv")],
                   stdout=subprocess.PIPE, check=True, timeout=300)
    hyper = (0.05, 0.03, 0.07, 0.3, 0.19)
    (tmp_path / "predict.cfg").write_text("0 200 4 %s 42 %s\n" % (hyper[0], " ".join(str(h) for h in hyper[1:])))
    out = subprocess.run([predict, "-c", str(tmp_path / "predict.cfg"), "-i", str(tmp_path / "ratings_f4_item_bias.csv"),
                          "-g", str(tmp_path / "ratings_f4_global_bias.csv"), "-q", str(tmp_path / "ratings_f4_q.csv"),
                          os.path.join(GOLDEN, "toy_user_spaces.csv")], stdout=subprocess.PIPE, text=True, check=True, timeout=300).stdout
    Q = cu.read_array(str(tmp_path / "ratings_f4_q.csv"))
    ib = cu.read_array(str(tmp_path / "ratings_f4_item_bias.csv")).ravel()
    gb = float(cu.read_array(str(tmp_path / "ratings_f4_global_bias.csv")).ravel()[0])
    u = cu.createSparseMatrix(os.path.join(GOLDEN, "toy_user_spaces.csv"))
    one = orc.CSR(np.array([0, u.nnz]), u.indices, u.data, 1, Q.shape[0])
    P, ub = orc.normal_fill(4, 4).reshape(1, 4), orc.normal_fill(1, 4)
    orc.sgd_iterations(one, P, Q.copy(), ub, ib.copy(), gb, hyper, 42, 0, 200, dot_order=orc.DOT_TREE16, update_items=False)
    pred = [orc.lib().orc_predict(4, P[0].ctypes.data_as(orc.C.POINTER(orc.C.c_float)), Q[i].ctypes.data_as(orc.C.POINTER(orc.C.c_float)),
                                  float(ub[0]), float(ib[i]), gb, orc.DOT_SEQ) for i in range(Q.shape[0])]
    want = sorted([(p, i) for i, p in enumerate(pred) if i not in set(u.indices.tolist())], key=lambda t: -t[0])
    lines = [l for l in out.split("\n") if l.startswith("Rank:")]
    assert len(lines) == len(want) == 2
    for rank, (line, (p, i)) in enumerate(zip(lines, want)):
        assert line == "Rank: %d\tItem: %d\tEstimated rating: %f" % (rank + 1, i, p)
