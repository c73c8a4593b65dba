"""CU2REC_SGD_BLOCKSOLVE (-m gpu): mf_sequential.cu:102-143's semantics with the long item chains solved block-wise
(cu2rec_amd/csrc/blocksolve.hip).  The mode re-associates sums (Gram matrix + forward substitution instead of 32
dependent row updates), so it is pinned at a TOLERANCE against the sequential oracle, stated in every test:
  * small sets, few iterations: every parameter within 2e-6 of the oracle (float rounding only);
  * the north-star bar at BASELINE.json configs[2]'s full shape (ML-20M shape, f=100): after 1,000 iterations
    |test RMSE - oracle| <= 1e-4 and every parameter within 1e-3.
Where no chain is long enough for a block solve the mode degenerates to the ordered walk and is bit-exact."""
import os

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HYPER = (0.01, 0.02, 0.02, 0.02, 0.02)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


@pytest.fixture
def min_rate():
    prev = api.blocksolve_min_rate()  # -1: automatic (scaled with the set)
    yield api.blocksolve_min_rate
    api.blocksolve_min_rate(prev)     # a negative value restores the automatic threshold, a positive one the explicit value


def _run_both(tr, f, iters, hyper=HYPER, seed=42, iter0=0, model=None, oracle_state=None):
    state = oracle_state or orc.init_model(tr.rows, tr.cols, f)
    model = model or cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(cu.DeviceCSR(tr), hyper, seed, iter0, iters, mode="blocksolve")
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, hyper, seed, iter0, iters, dot_order=orc.DOT_TREE16)
    return model, state


def _max_diffs(model, state):
    return [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)]


@pytest.mark.parametrize("users,items,nnz,f,iters,rate", [
    (300, 120, 6000, 1, 5, 2.0),      # f = 1: one float4 slot, three of the four column owners idle
    (300, 120, 6000, 10, 70, 2.0),    # crosses a 64-iteration schedule batch
    (300, 120, 6000, 100, 20, 2.0),
    (3000, 40, 30000, 100, 6, 1.0),   # 40 items: chains of ~75 links = three blocks, the last one partial
    (3000, 40, 30000, 50, 6, 1.0),
    (2000, 300, 40000, 64, 5, 0.5),
    (2000, 300, 40000, 128, 5, 0.5),
    (2000, 300, 40000, 200, 5, 0.5),  # 13 slots per column owner: the lane-per-column form of the transposed mat-vec
    (2000, 300, 40000, 252, 3, 4.0),
    (500, 50, 5000, 8, 10, 0.01),     # every item hot: nothing left for the walkers
    (9000, 6, 40000, 100, 3, 1.0),    # ~1,500 links per chain: the loader's ring (chains above six blocks)
])
def test_blocksolve_matches_sequential_oracle(min_rate, users, items, nnz, f, iters, rate):
    min_rate(rate)
    tr, _ = synth.make_ratings(users, items, nnz, min_degree=3, seed=users + f)
    model, state = _run_both(tr, f, iters)
    diffs = _max_diffs(model, state)
    assert max(diffs) <= 2e-6, diffs  # float rounding of re-associated sums; values are O(0.1 .. 1)


@pytest.mark.parametrize("users,items,nnz,f,iters,rate,la", [
    (300, 120, 6000, 10, 70, 2.0, 1),       # every chain of two blocks and more; crosses a schedule batch
    (3000, 40, 30000, 100, 6, 1.0, 1),      # three blocks a chain, the last one partial
    (9000, 6, 40000, 100, 3, 1.0, 10),      # ~24 blocks a chain: the rings go round many times
    (9000, 6, 40000, 116, 3, 1.0, 2),       # the widest row the form takes (29 slots)
    (2000, 300, 40000, 128, 5, 0.5, 1),     # wider: stays in the plain form
    (9000, 12, 60000, 40, 4, 1.0, 8),       # mixed: chains on both sides of the threshold
    (9000, 3, 30000, 1, 3, 1.0, 1),         # f = 1, ~47 blocks a chain
    (9000, 6, 40000, 64, 3, 1.0, 3),        # 16 slots: the narrow instantiation's last bucket
    (20000, 300, 90000, 16, 3, 8.0, 1),     # ~280 hot chains, most of them two or three blocks
])
def test_blocksolve_lookahead_form_matches_sequential_oracle(min_rate, users, items, nnz, f, iters, rate, la):
    """cu2rec_blocksolve_lookahead_blocks: the leading chains run phase 2 as e_i = M_i (pre_i - N_i e_(i-1)) on one wavefront,
    the item row one block behind (blocksolve_lookahead.hpp, chain_lookahead); the formulas: tests/test_blocksolve_algebra.py."""
    min_rate(rate)
    prev = cu.api.blocksolve_lookahead_blocks(la)
    try:
        tr, _ = synth.make_ratings(users, items, nnz, min_degree=3, seed=users + f)
        model, state = _run_both(tr, f, iters)  # (the schedule is created here: it reads the setting)
        assert max(_max_diffs(model, state)) <= 2e-6
    finally:
        cu.api.blocksolve_lookahead_blocks(prev)


def test_blocksolve_without_hot_items_is_the_ordered_walk_bit_for_bit(min_rate):
    min_rate(1e9)
    tr, _ = synth.make_ratings(3000, 40, 30000, min_degree=3, seed=11)
    model, state = _run_both(tr, 50, 6)
    for g, w in zip(model.download(), state):
        np.testing.assert_array_equal(g, w)


def test_blocksolve_resume_empty_users_frozen_items_and_lr_change(min_rate):
    min_rate(0.5)
    tr, _ = synth.make_ratings(1500, 60, 20000, min_degree=3, seed=5)
    indptr = tr.indptr.copy()  # users 100..139 lose their ratings: sentinel keys in the schedule
    lo, hi = indptr[100], indptr[140]
    indptr[100:141] = lo
    indptr[141:] -= hi - lo
    tr = cu.HostCSR(indptr, np.delete(tr.indices, np.s_[lo:hi]), np.delete(tr.data, np.s_[lo:hi]), tr.rows, tr.cols, tr.global_bias)
    f = 24
    model, state = _run_both(tr, f, 3)
    model, state = _run_both(tr, f, 70, iter0=3, model=model, oracle_state=state)          # resumed, crosses a batch
    decayed = (0.002, 0.02, 0.03, 0.04, 0.05)                                             # new decay tables
    model, state = _run_both(tr, f, 4, hyper=decayed, iter0=73, model=model, oracle_state=state)
    assert max(_max_diffs(model, state)) <= 5e-6
    model.sgd(cu.DeviceCSR(tr), HYPER, 42, 77, 5, mode="blocksolve", update_items=False)     # is_train == false
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, 42, 77, 5, dot_order=orc.DOT_TREE16, update_items=False)
    assert max(_max_diffs(model, state)) <= 5e-6


def test_blocksolve_calls_of_any_length_share_schedule_windows(min_rate):
    """One DeviceCSR, calls of 7 / 20 / 50 / 3 / 70 iterations that continue each other across the 64-iteration schedule windows
    (ordered.hip, Window: a call runs out of whichever window holds its iterations, at whatever offset; the plan of the blocks is the
    window's too), then a jump back into iterations already run, a jump ahead and another seed: after every call the oracle's state
    within the mode's rounding."""
    min_rate(2.0)
    tr, _ = synth.make_ratings(300, 120, 6000, min_degree=3, seed=310)
    f = 10
    d = cu.DeviceCSR(tr)
    assert d.blocksolve_items() > 0
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    state = orc.init_model(tr.rows, tr.cols, f)
    for k, (seed, it0, n) in enumerate([(42, 0, 7), (42, 7, 20), (42, 27, 50), (42, 77, 3), (42, 80, 70), (42, 5, 10), (42, 300, 9),
                                        (7, 309, 30), (7, 339, 100)]):
        model.sgd(d, HYPER, seed, it0, n, mode="blocksolve")
        orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, seed, it0, n, dot_order=orc.DOT_TREE16)
        assert max(_max_diffs(model, state)) <= 5e-6, (k, _max_diffs(model, state))


def test_blocksolve_raw_pointers_user_offset(min_rate):
    """cu2rec_sgd_update_blocksolve on a user shard: draws are keyed by the global user id."""
    from cu2rec_amd.engine import DeviceRatings, Engine
    min_rate(1.0)
    tr, _ = synth.make_ratings(3000, 40, 30000, min_degree=3, seed=8)
    f, u0, u1 = 20, 500, 2600
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    shard = tr.slice_users(u0, u1)
    eng = Engine(u1 - u0, tr.cols, f, tr.global_bias, P[u0:u1], Q, ub[u0:u1], ib)
    eng.sgd(DeviceRatings(shard, eng.device), HYPER, 42, 0, 12, mode="blocksolve", user_offset=u0)
    indptr = tr.indptr.copy()
    indptr[:u0 + 1] = tr.indptr[u0]
    indptr[u1:] = tr.indptr[u1]
    orc.sgd_iterations(orc.CSR(indptr, tr.indices, tr.data, tr.rows, tr.cols), P, Q, ub, ib, tr.global_bias, HYPER, 42, 0, 12,
                       dot_order=orc.DOT_TREE16)
    gP, gQ, gub, gib = eng.download()
    for g, w in ((gP, P[u0:u1]), (gQ, Q), (gub, ub[u0:u1]), (gib, ib)):
        assert float(np.abs(g.astype(np.float64) - w).max()) <= 2e-6


def test_blocksolve_train_loop_matches_ordered(min_rate):
    """cu2rec_train in block-solve mode: same schedule / LR decay / logged losses as the exact ordered mode, to 1e-5."""
    min_rate(1.0)
    tr, te = synth.make_ratings(3000, 60, 40000, min_degree=3, seed=6)
    outs = []
    for mode in ("ordered", "blocksolve"):
        cfg = cu.default_config(total_iterations=90, n_factors=12, check_error=30, learning_rate=0.02)
        outs.append(cu.train(tr, te, cfg, mode=mode, verbose=False) + (cfg.learning_rate,))
    for a, b in zip(outs[0][:5], outs[1][:5]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5, equal_nan=True)
    assert outs[0][5] == outs[1][5]


def test_blocksolve_full_shape_ml20m_1000_iterations_within_1e4_of_oracle():
    """The north-star tolerance at BASELINE.json configs[2]: ML-20M shape (138,493 x 26,744, 15.9 M train ratings), f=100,
    1,000 iterations of the block-solve mode against 1,000 iterations of the sequential CPU oracle on the same sample
    stream: |test RMSE - oracle| <= 1e-4, every one of the 16.7 M parameters within 1e-3.  Against BOTH arithmetic orders of the
    oracle: the kernels' own dot-product order (TREE16) and mf_sequential.cu's -- the sequential f-loop of util.cu:199-204
    (DOT_SEQ), the order the reference binary itself computes in and the one the north star's 1e-4 is stated against."""
    import bench
    tr, te = bench.load_dataset("ml-20m", 20240917, 0, lambda: None)
    f, iters = 100, 1000
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(cu.DeviceCSR(tr), HYPER, 42, 0, iters, mode="blocksolve")
    got = model.loss(cu.DeviceCSR(te))
    # (the two oracle runs -- 1.4e8 sequential updates each, ~45 s of one host core -- were started at collection time and ran beside
    # the GPU tests in front of this one: tests/conftest.py)
    import conftest
    states = {orc.DOT_TREE16: conftest.oracle_state("ml-20m", f, iters, "TREE16"), orc.DOT_SEQ: conftest.oracle_state("ml-20m", f, iters, "SEQ")}
    for order in (orc.DOT_TREE16, orc.DOT_SEQ):
        P, Q, ub, ib = states[order]
        want = orc.loss(_as_orc(te), P, Q, ub, ib, tr.global_bias, dot_order=order)
        assert abs(got["rmse"] - want["rmse"]) <= 1e-4, (order, got["rmse"], want["rmse"])
        assert abs(got["mae"] - want["mae"]) <= 1e-4, order
        diffs = _max_diffs(model, (P, Q, ub, ib))
        assert max(diffs) <= 1e-3, (order, diffs)


def test_blocksolve_lookahead_form_full_shape_ml20m_against_the_ordered_mode():
    """The opt-in look-ahead form at the ML-20M shape, f=100: items expected to collect 12 blocks and more per iteration (the
    chains that ARE phase 2's duration).  72 iterations (a schedule batch is crossed) against the ordered mode -- the sequential
    result bit for bit -- on the same sample stream: every parameter within 5e-6, and not the plain block-solve bits."""
    import bench
    tr, _ = bench.load_dataset("ml-20m", 20240917, 0, lambda: None)
    f, iters = 100, 72
    d_tr = cu.DeviceCSR(tr)
    exact = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    exact.sgd(d_tr, HYPER, 42, 0, iters, mode="ordered")
    plain = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    plain.sgd(d_tr, HYPER, 42, 0, iters, mode="blocksolve")
    prev = cu.api.blocksolve_lookahead_blocks(12)
    try:
        d_la = cu.DeviceCSR(tr)  # the setting is read when the schedule is created
        assert d_la.blocksolve_items() > 0
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(d_la, HYPER, 42, 0, iters, mode="blocksolve")
    finally:
        cu.api.blocksolve_lookahead_blocks(prev)
    want = exact.download()
    diffs = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), want)]
    assert max(diffs) <= 5e-6, diffs
    assert any(not np.array_equal(g, w) for g, w in zip(model.download(), plain.download())), "the look-ahead form did not run"


def test_blocksolve_full_shape_netflix_f128_against_the_cpu_oracle():
    """BASELINE.json configs[4]'s shape on one GPU: Netflix shape (480,189 x 17,770, 79 M train ratings), f=128 -- the automatic
    hot threshold of 880 expected updates, chains of ~70 blocks, the f=128 row bucket.  72 iterations (a 64-iteration schedule
    batch is crossed) of the block-solve mode against the sequential CPU oracle (mf_sequential.cu:102-143) on the same sample
    stream: every one of the 64 M parameters within 5e-6, test RMSE / MAE within 1e-5 -- and the block-solve kernels did run."""
    import bench
    tr, te = bench.load_dataset("netflix", 20240917, 0, lambda: None)
    f, iters = 128, 72
    d_tr = cu.DeviceCSR(tr)
    assert d_tr.blocksolve_items() > 0, "no item above the threshold: this would test the ordered walk"
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(d_tr, HYPER, 42, 0, iters, mode="blocksolve")
    import conftest
    P, Q, ub, ib = conftest.oracle_state("netflix", f, iters, "TREE16")  # (started at collection time: tests/conftest.py)
    diffs = _max_diffs(model, (P, Q, ub, ib))
    assert max(diffs) <= 5e-6, diffs
    got = model.loss(cu.DeviceCSR(te))
    want = orc.loss(_as_orc(te), P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_TREE16)
    assert abs(got["rmse"] - want["rmse"]) <= 1e-5 and abs(got["mae"] - want["mae"]) <= 1e-5, (got, want)


def test_blocksolve_full_shape_ml1m_f50_is_the_oracle_bit_for_bit():
    """BASELINE.json configs[1]'s shape: ML-1M shape (6,040 x 3,706), f=50.  No item collects enough updates per iteration for a
    block solve, so the mode IS the ordered walk there (whichever launch form runs it): 200 iterations equal the sequential CPU
    oracle bit for bit, all 0.5 M parameters."""
    import bench
    tr, te = bench.load_dataset("ml-1m", 20240917, 0, lambda: None)
    f, iters = 50, 200
    d_tr = cu.DeviceCSR(tr)
    assert d_tr.blocksolve_items() == 0
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(d_tr, HYPER, 42, 0, 72, mode="blocksolve")
    model.sgd(d_tr, HYPER, 42, 72, iters - 72, mode="blocksolve")  # resumed across a schedule batch
    state = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, 42, 0, iters, dot_order=orc.DOT_TREE16)
    for g, w in zip(model.download(), state):
        np.testing.assert_array_equal(g, w)


def test_bench_times_exactly_k_steps_and_dumps_the_model_they_leave(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on the ML-1M shape, where the timed mode IS the ordered walk: the line
    counts exactly K timed steps and W + K iterations, and DIR holds the model after the last of them -- the oracle's, bit for bit."""
    import json
    import subprocess
    import sys
    import bench
    warmup, steps, f = 2, 3, 50
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--workload", "ml-1m", "--factors", str(f), "--no-cpu-baseline", "--no-side-modes", "--dump-outputs", str(out)],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["timed_steps"] == steps and line["timed_regions"] == 1
    assert line["iterations_run"] == warmup + steps and line["ms_per_step"] > 0
    assert line["dumped_outputs"]["factor_rows"] == {"user_factors": "all", "item_factors": "all"}
    tr, _ = bench.load_dataset("ml-1m", 20240917, 0, lambda: None)
    state = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, 42, 0, warmup + steps, dot_order=orc.DOT_TREE16)
    for name, want in zip(("user_factors", "item_factors", "user_bias", "item_bias"), state):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32, name
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_bench_side_legs_run_with_full_only(tmp_path):
    """A plain `bench.py` run prints the headline without the side legs; `--full` adds them and the CPU baselines to the same line,
    with the same headline model (ML-1M shape, f=50: the timed mode IS the ordered walk, so its gap to the sequential result is 0;
    100 iterations, past the side legs' own warm-up of 64)."""
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    lines = {}
    for extra in ((), ("--full",)):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "50",
                              "--workload", "ml-1m", "--factors", "50", *extra], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        lines[extra] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = lines[()], lines[("--full",)]
    legs = ("rmse_gap_vs_sequential", "ordered_mode", "hogwild_streaming_mode", "tier2_converged", "loss_kernel", "cpu_baseline")
    assert not [k for k in legs if k in plain], plain.keys()
    assert all(k in full for k in legs), full.keys()
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "timed_steps", "iterations_run", "test_rmse"):
        assert plain[k] == full[k], k
    assert full["rmse_gap_vs_sequential"]["gap"] == 0.0 and full["rmse_gap_vs_sequential"]["iterations"] == 100
    assert full["ordered_mode"]["value"] > 0 and full["hogwild_streaming_mode"]["value"] > 0 and full["loss_kernel"]["ms"] > 0
    assert set(full["tier2_converged"]["modes"]) >= {"blocksolve", "hogwild-streaming"}
    assert full["cpu_baseline"]["value"] > 0


@pytest.mark.parametrize("policy,name", [(2, "resident"), (0, "streaming")])
def test_hogwild_mid_trajectory_gap_to_sequential_stays_bounded_at_full_shape(policy, name):
    """A regression bound on the racy modes while the model is still moving (popular items lose most of their updates to the
    race, sgd.cu:18-21), at BASELINE.json configs[2]'s shape against the exact ordered mode on the same data and sample stream:
    |test RMSE gap| <= 8e-4 after 500 iterations and <= 4e-3 after 1,000 (measured: resident 4e-4 / 2.8e-3, streaming 2e-4 /
    2.4e-3).  Whether Hogwild meets the north star's bar is decided at CONVERGENCE, by the Tier-2 test below."""
    import bench
    from cu2rec_amd._lib import lib
    tr, te = bench.load_dataset("ml-20m", 20240917, 0, lambda: None)
    d_tr, d_te = cu.DeviceCSR(tr), cu.DeviceCSR(te)
    f = 100
    seq, hog = cu.Model(tr.rows, tr.cols, f, tr.global_bias), cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    prev = lib().cu2rec_hogwild_resident(policy)
    try:
        assert lib().cu2rec_hogwild_resident_plan(tr.rows, f, 500, None, None) == (1 if policy else 0)
        gaps = []
        for it0 in (0, 500):
            seq.sgd(d_tr, HYPER, 42, it0, 500, mode="ordered")
            hog.sgd(d_tr, HYPER, 42, it0, 500, mode="hogwild")
            gaps.append(abs(hog.loss(d_te)["rmse"] - seq.loss(d_te)["rmse"]))
    finally:
        lib().cu2rec_hogwild_resident(prev)
    assert gaps[0] <= 8e-4 and gaps[1] <= 4e-3, (name, gaps)


def test_tier2_converged_runs_under_the_reference_schedule_pick_the_headline_mode():
    """SURVEY.md section 8c Tier 2 as written -- *converged* test RMSE against the sequential result within 1e-4 -- at BASELINE.json
    configs[2]'s shape (ML-20M shape, f=100): every mode runs the product's train() under the reference's schedule (loss check every
    500 iterations, patience 2, decay 0.2: training.cu:118,146-155) for 8,000 iterations, by which the learning rate has decayed five
    to six times (lr < 1e-5: the model has stopped moving).  The outcome, pinned EITHER way (profiles/r05_tier2_converged_*.json holds
    three sampler seeds per mode and the ML-1M shape):
      * block-solve (bench.py's `value`): converged gap <= 1e-4 (measured 1.0e-5 ... 1.3e-5);
      * Hogwild, resident and streaming launches (sgd.cu:18-21's racy semantics): converged gap ABOVE 1e-4 (measured 2.5e-3 ... 8.3e-3
        and 3.2e-3 ... 3.3e-3): the race delays the minimum of the test RMSE by a check, so the rate decays 500 iterations later and
        the run freezes somewhere else.  If this assertion ever fails, Hogwild meets the north star's bar and bench.py's headline
        should become the resident Hogwild form."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import tier2_converged as t2
    tr, te = bench.load_dataset("ml-20m", 20240917, 0, lambda: None)
    d_tr, d_te = cu.DeviceCSR(tr), cu.DeviceCSR(te)
    f, iters, seed = 100, 8000, 42
    seq, _ = t2.run_mode(cu, d_tr, d_te, f, seed, iters, "ordered")
    assert seq["converged"] and seq["n_decays"] >= 3 and seq["final_learning_rate"] < 1e-5, seq
    assert seq["min_test_rmse"] < seq["final_test_rmse"] < 0.83, seq  # the schedule froze the run a little past its minimum
    gaps = {}
    for label in ("blocksolve", "hogwild-resident", "hogwild-streaming"):
        rec, _ = t2.run_mode(cu, d_tr, d_te, f, seed, iters, label)
        assert rec["converged"], rec
        gaps[label] = abs(rec["final_test_rmse"] - seq["final_test_rmse"])
    assert gaps["blocksolve"] <= 1e-4, gaps
    assert 1e-4 < gaps["hogwild-resident"] <= 2e-2 and 1e-4 < gaps["hogwild-streaming"] <= 2e-2, gaps


def test_converged_ml20m_blocksolve_against_the_cpu_oracle_in_the_references_own_arithmetic():
    """The north-star sentence as written, on BASELINE.json configs[2] (ML-20M shape, f=100): "converged P/Q/bias outputs must match
    mf_sequential.cu on fixed seed within 1e-4 RMSE" -- the product's cu2rec_train in the headline mode (CU2REC_SGD_BLOCKSOLVE) against
    the CPU ORACLE's train() (orc_train = mf_sequential.cu:102-201 under training.cu:118,146-155's schedule: check every 500, patience
    2, decay 0.2, lr .01) in the reference's OWN arithmetic: the sequential dot of mf_sequential.cu:122-125 (DOT_SEQ), run once with
    the float loss accumulators of mf_sequential.cu:147-174 (ACC_F32: what the reference prints and takes its patience decisions on)
    and once with double ones (ACC_F64: loss.cu:185-190).  5,000 iterations = three decays (lr 8e-5 from 4,500 on): the model has
    stopped moving.  The oracle runs are 6.9e8 sequential updates each, started at collection time (tests/conftest.py).
      * the learning rate decays at the SAME iterations in all three runs -- no patience decision flips between the kernels' arithmetic
        (tree dot, block-wise re-associated sums, fp64 loss sums) and the reference's (sequential dot, float or double sums);
      * against the ACC_F64 oracle: every logged test RMSE (11 checks) and the final one within 1e-4; train RMSE likewise;
      * against the ACC_F32 oracle -- the reference's printed numbers: its float accumulators drop the small squared errors once the
        running sum is large, so what it PRINTS is 1.6e-3 (test) / 1.0e-2 (train) below the true RMSE of its own model (a property of
        mf_sequential.cu:147-174, pinned here as a finding); the model it converges to is the ACC_F64 run's bit for bit, and the
        reference's own loss routine (DOT_SEQ, ACC_F32) applied to the PRODUCT's converged P/Q/biases is within 1e-4 of what it
        prints for its own;
      * parameters: max |dP|, |dQ|, |d user_bias|, |d item_bias| reported (profiles/r06_converged_vs_cpu_oracle.json) and bounded."""
    import json
    import bench
    import conftest
    tr, te = bench.load_dataset("ml-20m", 20240917, 0, lambda: None)
    f, iters = 100, 5000
    d_tr, d_te = cu.DeviceCSR(tr), cu.DeviceCSR(te)
    cfg = api.default_config(total_iterations=iters, n_factors=f, learning_rate=0.01, seed=42, P_reg=0.02, Q_reg=0.02, user_bias_reg=0.02,
                             item_bias_reg=0.02)
    P, Q, losses, ub, ib, stats = api.train(d_tr, d_te, cfg, mode="blocksolve", verbose=False, return_stats=True)
    checks = [(i + 1, float(v)) for i, v in enumerate(losses) if np.isfinite(v)]
    rec64, state64 = conftest.oracle_converged_run("ml-20m", f, iters, "SEQ", "F64")
    rec32, state32 = conftest.oracle_converged_run("ml-20m", f, iters, "SEQ", "F32")
    # ---- the schedule: same checks, same decay iterations, same final rate
    lr, decays = np.float32(0.01), []
    last, patience = np.float32(np.finfo(np.float32).max), int(cfg.patience)
    for it, r in checks:  # (training.cu:129,146-155 replayed on the product's logged losses)
        if last < np.float32(r):
            patience -= 1
        if patience <= 0:
            patience, lr = int(cfg.patience), np.float32(lr * np.float32(cfg.learning_rate_decay))
            decays.append(it)
        last = np.float32(r)
    assert [c[0] for c in checks] == [e["iteration"] for e in rec64["checks"]] == [e["iteration"] for e in rec32["checks"]]
    assert decays == rec64["decay_iterations"] == rec32["decay_iterations"] and len(decays) >= 3, (decays, rec64["decay_iterations"], rec32["decay_iterations"])
    assert float(cfg.learning_rate) == rec64["final_learning_rate"] == rec32["final_learning_rate"] < 1e-4
    # ---- double accumulators: every logged test RMSE within 1e-4
    gaps = [abs(r - e["test_rmse"]) for (_, r), e in zip(checks, rec64["checks"])]
    assert max(gaps) <= 1e-4, list(zip([c[0] for c in checks], gaps))
    assert abs(checks[-1][1] - rec64["final_test_rmse"]) <= 1e-4
    assert abs(float(stats.last_train_rmse) - rec64["final_train_rmse"]) <= 1e-4
    # ---- float accumulators (what the reference binary prints): same model as the F64 run; its own loss routine on OUR factors
    for a, b in zip(state32, state64):
        np.testing.assert_array_equal(a, b)
    ref_on_ours = orc.loss(_as_orc(te), P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_SEQ, acc=orc.ACC_F32)
    assert abs(ref_on_ours["rmse"] - rec32["final_test_rmse"]) <= 1e-4, (ref_on_ours["rmse"], rec32["final_test_rmse"])
    printed_bias = rec64["final_test_rmse"] - rec32["final_test_rmse"]
    assert 5e-4 <= printed_bias <= 4e-3, printed_bias  # the finding: float sums under-report by ~1.6e-3 on 3.9 M test ratings
    # ---- parameters
    names = ("max_abs_dP", "max_abs_dQ", "max_abs_d_user_bias", "max_abs_d_item_bias")
    diffs = {n: float(np.abs(g.astype(np.float64) - w).max()) for n, g, w in zip(names, (P, Q, ub, ib), state64)}
    rms = {n.replace("max_abs", "rms"): float(np.sqrt(np.mean((g.astype(np.float64) - w) ** 2))) for n, g, w in zip(names, (P, Q, ub, ib), state64)}
    assert max(diffs.values()) <= 1e-3 and max(rms.values()) <= 1e-5, (diffs, rms)  # measured: 4.5e-5 (one Q entry), rms 2.3e-7
    out = {"what": "cu2rec_train(CU2REC_SGD_BLOCKSOLVE) on one MI355X against oracle/cu2rec_oracle.c orc_train (DOT_SEQ) on one host core; "
                   "ml-20m shape f=100, 5000 iterations, reference schedule, seed 42",
           "product": {"checks": checks, "decay_iterations": decays, "final_learning_rate": float(cfg.learning_rate),
                       "final_test_rmse": checks[-1][1], "final_train_rmse": float(stats.last_train_rmse), "seconds_sgd": float(stats.seconds_sgd)},
           "cpu_oracle_f64": {k: rec64[k] for k in ("checks", "decay_iterations", "final_learning_rate", "final_test_rmse", "final_train_rmse", "seconds_wall")},
           "cpu_oracle_f32": {k: rec32[k] for k in ("checks", "decay_iterations", "final_learning_rate", "final_test_rmse", "final_train_rmse", "seconds_wall")},
           "max_gap_logged_test_rmse_vs_f64": max(gaps), "gap_final_test_rmse_vs_f64": abs(checks[-1][1] - rec64["final_test_rmse"]),
           "reference_loss_routine_on_product_factors": ref_on_ours["rmse"],
           "gap_reference_loss_routine_on_product_factors_vs_its_own": abs(ref_on_ours["rmse"] - rec32["final_test_rmse"]),
           "float_accumulator_bias_of_the_printed_test_rmse": printed_bias, "same_decay_iterations": True, **diffs, **rms}
    os.makedirs(os.path.join(conftest.ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(conftest.ROOT, "gpurun_out", "converged_vs_cpu_oracle.json"), "w") as fh:
        json.dump(out, fh, indent=1)


def test_bin_mf_blocksolve_mode_against_the_oracle_run(tmp_path):
    """bin/mf -m blocksolve end to end (mf.cu:16-99): the printed TEST RMSE lines and the written factors against the
    oracle's sequential run of the same schedule (CU2REC_BLOCKSOLVE_RATE makes half of the items hot on this small set)."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    tr, te = synth.make_ratings(3000, 60, 40000, min_degree=3, seed=31)
    synth.write_csv(str(tmp_path / "train.csv"), tr)
    synth.write_csv(str(tmp_path / "test.csv"), te)
    (tmp_path / "c.cfg").write_text("0 40 16 0.01 42 0.02 0.02 0.02 0.02\n")
    env = dict(os.environ, CU2REC_BLOCKSOLVE_RATE="1.0")
    out = subprocess.run([os.path.join(ROOT, "bin", "mf"), "-c", str(tmp_path / "c.cfg"), "-m", "blocksolve", str(tmp_path / "train.csv"),
                          str(tmp_path / "test.csv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, 16)
    orc.sgd_iterations(_as_orc(tr), P, Q, ub, ib, tr.global_bias, HYPER, 42, 0, 40, dot_order=orc.DOT_TREE16)
    want_rmse = orc.loss(orc.CSR(te.indptr, te.indices, te.data, te.rows, te.cols, te.global_bias), P, Q, ub, ib, tr.global_bias,
                         dot_order=orc.DOT_TREE16)["rmse"]
    got_rmse = float(re.findall(r"TEST: Iteration 40 GPU MAE: \S+ RMSE: (\S+)", out.stdout)[-1])
    assert abs(got_rmse - want_rmse) <= 2e-6
    for comp, want in (("p", P), ("q", Q), ("user_bias", ub), ("item_bias", ib)):
        got = np.loadtxt(str(tmp_path / ("train_f16_%s.csv" % comp)), delimiter=",", ndmin=2).reshape(want.shape)
        assert float(np.abs(got - want).max()) <= 5e-6, comp  # %f files: six decimals


def test_train_in_blocksolve_mode_follows_the_oracle_schedule(min_rate):
    """cu2rec_train (training.cu:95-180) with CU2REC_SGD_BLOCKSOLVE: same checks, same patience / decay decisions and learning
    rate as the oracle's sequential run, logged test RMSE within float rounding of the re-associated sums."""
    min_rate(1.0)
    tr, te = synth.make_ratings(3000, 60, 40000, min_degree=3, seed=17)
    kw = dict(total_iterations=48, n_factors=20, check_error=8, learning_rate=0.05, patience=1.0)
    cfg, ocfg = cu.default_config(**kw), orc.default_config(**kw)
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, 20)
    log = orc.train(_as_orc(tr), orc.CSR(te.indptr, te.indices, te.data, te.rows, te.cols, te.global_bias), ocfg, P, Q, ub, ib,
                    tr.global_bias, dot_order=orc.DOT_TREE16, acc=orc.ACC_F64, schedule=orc.SCHED_PATIENCE)
    gP, gQ, losses, gub, gib, stats = cu.train(tr, te, cfg, mode="blocksolve", verbose=False, return_stats=True)
    assert [e["iteration"] - 1 for e in log] == [0, 7, 15, 23, 31, 39, 47]
    for e in log:
        assert abs(float(losses[e["iteration"] - 1]) - e["test_rmse"]) <= 2e-6
    assert cfg.learning_rate == ocfg.learning_rate and cfg.cur_iterations == 48 == ocfg.cur_iterations
    assert stats.n_checks == 7
    for g, w in ((gP, P), (gQ, Q), (gub, ub), (gib, ib)):
        assert float(np.abs(g.astype(np.float64) - w).max()) <= 5e-6


@pytest.mark.parametrize("case", range(10))
def test_blocksolve_random_shapes_long_chains(min_rate, case):
    """Long chains (hundreds to thousands of links per item and iteration: the ring of LDS slots, the loaders' register pipeline,
    the solvers' meeting points all cycle many times) at row widths from every compiled bucket, drawn from a fixed seed."""
    rng = np.random.RandomState(1000 + case)
    f = int(rng.choice([3, 8, 17, 33, 64, 100, 112, 128, 160, 200, 250]))
    items = int(rng.choice([3, 5, 9, 20]))
    users = int(rng.randint(4000, 16000))
    per_user = int(rng.randint(2, min(items, 6) + 1))
    min_rate(float(rng.choice([0.5, 50.0, 400.0])))
    tr, _ = synth.make_ratings(users, items, users * per_user, min_degree=min(2, per_user), seed=case)
    model, state = _run_both(tr, f, int(rng.randint(2, 5)))
    assert max(_max_diffs(model, state)) <= 3e-6, (f, items, users)


_FAULT_SCRIPT = r"""
import os
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import Cu2recError, check, lib
from oracle import oracle as orc
api.blocksolve_min_rate(1.0)
tr, _ = synth.make_ratings(3000, 40, 30000, min_degree=3, seed=3100)
f, iters, hyper = 100, 5, (0.01, 0.02, 0.02, 0.02, 0.02)
d_tr = cu.DeviceCSR(tr)
assert d_tr.blocksolve_items() > 0
model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
try:
    model.sgd(d_tr, hyper, 42, 0, iters, mode="blocksolve")
    check(lib().cu2rec_check_faults())
except Cu2recError as e:
    print("STATUS", e.status, "gave up" in str(e), "with events instead" in str(e), "CU2REC_BS_GATE" in str(e))
    if os.environ.get("CU2REC_BS_GATE"):  # forced: no healing, the device form stays
        print("TOPOLOGY", api.blocksolve_topology()[0])
        sys.exit(0)
    # self-healing: the process has switched to the event fork / join -- a fresh model, the same call, the oracle's result
    assert api.blocksolve_topology()[0] == "events", api.blocksolve_topology()
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(d_tr, hyper, 42, 0, iters, mode="blocksolve")
    check(lib().cu2rec_check_faults())
    state = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(orc.CSR(tr.indptr, tr.indices, tr.data, tr.rows, tr.cols, tr.global_bias), *state, tr.global_bias, hyper, 42, 0,
                       iters, dot_order=orc.DOT_TREE16)
    print("HEALED %%.3e" %% max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)))
    sys.exit(0)
assert api.blocksolve_topology()[0] == "device", api.blocksolve_topology()  # (the probe passed: nothing serialises the streams here)
state = orc.init_model(tr.rows, tr.cols, f)
orc.sgd_iterations(orc.CSR(tr.indptr, tr.indices, tr.data, tr.rows, tr.cols, tr.global_bias), *state, tr.global_bias, hyper, 42, 0,
                   iters, dot_order=orc.DOT_TREE16)
print("OK %%.3e" %% max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)))
"""


def _run_fault_script(dbg, **extra_env):
    import subprocess
    import sys
    # (the fault injection is compiled only into the test build of the library: make test-hooks -> build/test/libcu2rec_amd_hooks.so)
    hooks = os.path.join(ROOT, "build", "test", "libcu2rec_amd_hooks.so")
    assert os.path.exists(hooks), "build/test/libcu2rec_amd_hooks.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, CU2REC_BS_DBG=str(dbg), CU2REC_BS_WAIT_S="0.02", CU2REC_AMD_LIB=hooks)
    env.pop("CU2REC_BS_GATE", None)
    env.update(extra_env)
    res = subprocess.run([sys.executable, "-c", _FAULT_SCRIPT % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    return res.stdout.strip().splitlines()


def test_blocksolve_join_wait_that_is_never_satisfied_ends_in_ehip_and_the_process_heals():
    """The default launch topology's join: phase 3 carries one workgroup that waits for the number a signal kernel behind the side
    kernel stores.  With the signal never sent (CU2REC_BS_DBG=16) and the waits' bound cut to 20 ms (CU2REC_BS_WAIT_S; the join
    waits 15 x that) the launch ends by itself, the status word is set and the call reports CU2REC_EHIP -- nothing hangs -- and the
    error says that the process now forks and joins with events.  It does: the SAME call on a fresh model (the signal is still never
    sent: the event form does not need it) gives the oracle's result, and cu2rec_blocksolve_topology says "events".  In a process of
    its own: the settings are read once."""
    lines = _run_fault_script(16)
    assert lines[-2] == "STATUS -3 True True False", lines[-3:]
    assert lines[-1].startswith("HEALED ") and float(lines[-1].split()[1]) <= 2e-6, lines[-1]


def test_blocksolve_join_that_gives_up_under_a_forced_device_topology_names_the_force():
    """The same join give-up (CU2REC_BS_DBG=16) with the device form forced by CU2REC_BS_GATE=1: the call still reports CU2REC_EHIP,
    but nothing switches -- the error names CU2REC_BS_GATE as what keeps the device form instead of announcing events, and
    cu2rec_blocksolve_topology still says "device"."""
    lines = _run_fault_script(16, CU2REC_BS_GATE="1")
    assert lines[-2:] == ["STATUS -3 True False True", "TOPOLOGY device"], lines[-3:]


_SWEEP_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import check, lib
from oracle import oracle as orc
hyper = (0.01, 0.02, 0.02, 0.02, 0.02)
worst = 0.0
for users, items, nnz, f, iters, rate in ((3000, 400, 30000, 100, 5, 4.0), (20000, 3000, 90000, 16, 4, 8.0), (6000, 5000, 40000, 50, 70, 1e9),
                                          (9000, 6, 40000, 100, 3, 1.0), (9000, 6, 40000, 128, 3, 1.0), (2000, 300, 40000, 200, 5, 0.5)):
    api.blocksolve_min_rate(rate)
    api.blocksolve_lookahead_blocks(2 if f == 100 else 0)
    tr, _ = synth.make_ratings(users, items, nnz, min_degree=3, seed=users + f)
    d_tr = cu.DeviceCSR(tr)
    state = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(orc.CSR(tr.indptr, tr.indices, tr.data, tr.rows, tr.cols, tr.global_bias), *state, tr.global_bias, hyper, 42, 0,
                       iters, dot_order=orc.DOT_TREE16)
    exact = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    exact.sgd(d_tr, hyper, 42, 0, iters, mode="ordered")
    for g, w in zip(exact.download(), state):
        assert np.array_equal(g, w), "ordered mode with the walk swept by one workgroup differs from the oracle"
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(d_tr, hyper, 42, 0, iters, mode="blocksolve")
    check(lib().cu2rec_check_faults())
    worst = max(worst, max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)))
print("OK %%.3e" %% worst)
"""


def test_launch_bounds_too_small_are_swept_and_change_nothing():
    """The walk of an iteration covers only the TAIL of the sorted order, as long as the host expects it to be (OrderedSchedule::walk_bound:
    mean + 8 sigma of the positions behind the two-wave chains); what an iteration has in front of that is swept by one extra workgroup.
    The bound is about speed, never about results: in the test build CU2REC_BS_DBG=256 cuts it to 16 positions, so the sweeper does
    nearly the whole walk -- thousands of short chains -- and the ordered mode still equals the oracle bit for bit, the block-solve mode
    within its rounding, on sets with hundreds to thousands of walked items.  Likewise phase 3 of a block-solve iteration is launched
    with the EXPECTED number of blocks (BlockSolve's constructor, blocksolve.hip) and strides through the dense block table (phase 1
    keeps the full grid): with the launch cut to 3 workgroups (bit 512) every one of them does many blocks in turn -- same results."""
    import subprocess
    import sys
    hooks = os.path.join(ROOT, "build", "test", "libcu2rec_amd_hooks.so")
    assert os.path.exists(hooks), "build/test/libcu2rec_amd_hooks.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, CU2REC_BS_DBG="768", CU2REC_AMD_LIB=hooks)
    res = subprocess.run([sys.executable, "-c", _SWEEP_SCRIPT % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith("OK ") and float(last.split()[1]) <= 2e-6, last


def test_blocksolve_gate_that_never_opens_only_costs_time():
    """The side stream's gate kernel guards timing, not data: one that can never be satisfied (CU2REC_BS_DBG=32) gives up after the
    bound and the run goes on -- no error, and the result is the oracle's within the mode's usual rounding (a gate
    timeout must not declare the model state undefined)."""
    last = _run_fault_script(32)[-1]
    assert last.startswith("OK "), last
    assert float(last.split()[1]) <= 2e-6, last


_TOPOLOGY_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import check, lib
from oracle import oracle as orc
hyper = (0.01, 0.02, 0.02, 0.02, 0.02)
worst = 0.0
for users, items, nnz, f, iters, rate, la in ((300, 120, 6000, 10, 70, 2.0, 0), (3000, 40, 30000, 100, 6, 1.0, 2), (9000, 6, 40000, 100, 3, 1.0, 4),
                                              (9000, 6, 40000, 128, 3, 1.0, 0), (2000, 300, 40000, 200, 5, 0.5, 0), (20000, 300, 90000, 16, 3, 8.0, 2)):
    api.blocksolve_min_rate(rate)
    api.blocksolve_lookahead_blocks(la)
    tr, _ = synth.make_ratings(users, items, nnz, min_degree=3, seed=users + f)
    d_tr = cu.DeviceCSR(tr)
    assert d_tr.blocksolve_items() > 0
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(d_tr, hyper, 42, 0, iters, mode="blocksolve")
    check(lib().cu2rec_check_faults())
    state = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(orc.CSR(tr.indptr, tr.indices, tr.data, tr.rows, tr.cols, tr.global_bias), *state, tr.global_bias, hyper, 42, 0,
                       iters, dot_order=orc.DOT_TREE16)
    worst = max(worst, max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)))
print("TOPOLOGY %%s | %%s" %% api.blocksolve_topology())
print("OK %%.3e" %% worst)
"""


def test_blocksolve_heals_itself_when_the_streams_share_one_hardware_queue():
    """nothing but a profiler's environment variable used to take the library off the device-side fork / join, and
    anything else that keeps the two streams from running side by side ended in a 30 s give-up.  Now the first block-solve call probes
    the streams it will use (a wait kernel queued first on one, a signal kernel on the other, 10 ms bound, both directions).  Here:
    GPU_MAX_HW_QUEUES=1 in a child process -- every HIP stream of the process feeds ONE hardware queue -- and the whole small-shape
    matrix (plain and look-ahead chains, short and long, wide rows, more chains than CUs) against the sequential oracle: the oracle's
    results within the mode's rounding, no timeout, no error; the probe's verdict is printed, and if it says "events" the reason
    names the probe."""
    import subprocess
    import sys
    import time
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1")
    env.pop("CU2REC_BS_GATE", None)
    t0 = time.time()
    res = subprocess.run([sys.executable, "-c", _TOPOLOGY_SCRIPT % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith("OK ") and float(lines[-1].split()[1]) <= 2e-6, lines[-2:]
    assert lines[-2].startswith("TOPOLOGY "), lines[-2:]
    mode = lines[-2].split()[1]
    assert mode in ("events", "device"), lines[-2]
    assert mode == "device" or "handshake probe" in lines[-2], lines[-2]
    assert time.time() - t0 < 240, "the run took as long as a give-up would"
    print(lines[-2])


def test_blocksolve_event_fork_and_join_matches_sequential_oracle():
    """The launch topology a rocprofv3 counter pass gets (CU2REC_BS_GATE=0; the library takes it by itself when it sees
    ROCPROF_COUNTER_COLLECTION): the side stream forked by an event on phase 1's completion signal and joined by an event wait in front
    of the next phase 1, instead of the gate kernel and the device-side join of the default.  Same kernels, same results: plain and
    look-ahead chains, short and long, wide rows, more chains than CUs -- each against the sequential oracle.  In a process of its own:
    the setting is read once."""
    import subprocess
    import sys
    env = dict(os.environ, CU2REC_BS_GATE="0")
    res = subprocess.run([sys.executable, "-c", _TOPOLOGY_SCRIPT % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith("OK "), last
    assert float(last.split()[1]) <= 2e-6, last
