"""Softmax matrix factorization without a GPU: the float64 reference and the float32 restatement of tests/softmax_reference64.py on
the sets the GPU tests judge (tests/softmax_checks.py) -- the derived bounds are fair to a correct float32 evaluation and every
deliberate mistake breaks them -- the gradient against finite differences, the ML_SMALL experiment in float64, and what the C ABI,
the Python front end and bin/mf refuse before any device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import softmax_checks as chk
import softmax_reference64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gradient_is_the_objectives_by_central_differences():
    """7 users x 40 items at f = 8, every coordinate of P, Q and the item biases: (L(x + h) - L(x - h)) / 2h at h = 1e-5 is off by
    h^2 / 6 |L'''| -- the third derivatives here are sums of at most W_u <= 45 times third moments of factors of O(0.3), below 1e3, so
    below 2e-8 -- plus the differences' cancellation, 2^-53 |L| / h = 1e-16 x 2e3 / 1e-5 = 2e-8: 1e-6 leaves a factor of 25 (measured:
    5.8e-9)."""
    case = chk.cases()["empty-user"]
    state = tuple(np.asarray(a, np.float64) for a in case.state())
    h = 1e-5
    L = lambda st: ref.objective(case.csr, st, case.gb, case.hyper)
    gu, gub = ref.gradient(case.csr, state, case.gb, case.hyper, "users")
    gi, gib = ref.gradient(case.csr, state, case.gb, case.hyper, "items")
    worst = 0.0
    for which, grad, n in ((0, gu, case.csr.rows), (1, gi, case.csr.cols), (3, gib[:, None], case.csr.cols)):
        for r in range(n):
            for c in range(grad.shape[1]):
                hi, lo = [a.copy() for a in state], [a.copy() for a in state]
                hi[which].reshape(len(hi[which]), -1)[r, c] += h
                lo[which].reshape(len(lo[which]), -1)[r, c] -= h
                worst = max(worst, abs((L(hi) - L(lo)) / (2 * h) - grad[r, c]))
    print("worst distance from the central difference: %.3g" % worst)
    assert worst <= 1e-6
    assert not gub.any()
    # the objective does not see the user biases or the global bias: nothing of theirs is trained
    P, Q, ub, ib = state
    assert abs(L((P, Q, ub + 3.0, ib)) - L(state)) <= 1e-9 * abs(L(state))
    assert abs(ref.objective(case.csr, state, case.gb + 2.5, case.hyper) - L(state)) <= 1e-9 * abs(L(state))


def test_pi_sums_to_one_and_an_empty_user_only_shrinks():
    for name in ("empty-user", "dominated", "large-score-users", "f100-65x1000"):
        case = chk.cases()[name]
        assert np.abs(ref.mass(case.csr, case.state(), case.gb) - 1.0).max() <= 1e-12, name
    case = chk.cases()["empty-user"]
    P = case.state()[0]
    g, _ = ref.gradient(case.csr, case.state(), case.gb, case.hyper, "users")
    assert np.diff(case.csr.indptr)[1] == 0 and np.allclose(g[1], -case.hyper[1] * P[1].astype(np.float64), rtol=1e-14, atol=0)
    assert case.csr.indices.max() < case.csr.cols - 3  # cols larger than any stored item
    dom = chk.cases()["dominated"]
    S = chk.scores_of(tuple(a[:n] for a, n in zip(dom.state(), (dom.csr.rows, dom.csr.cols) * 2)), dom.gb)
    assert (np.exp(S[:, 5] - ref.lse(dom.csr, dom.state(), dom.gb)) > 1 - 1e-9).all()


def test_bounds_are_fair_and_every_mutation_breaks_them():
    """On every set the GPU tests judge: the float32 restatement in the kernels' order is within 0.5 of the bounds on lse, on
    sum_i pi and on every gradient value (worst measured: 0.076, 0.051 and 0.18, the last at a single partner), and each deliberate
    mistake is above 1 wherever softmax_checks.claimed() says it shows (least measured: 4.9, P_reg and Q_reg swapped; 6.8, the
    log-sum-exp over the model's three further items); every mistake is claimed on some set."""
    seen = dict.fromkeys(ref.MUTATIONS, 0)
    worst = {"lse": 0.0, "mass": 0.0, "gradient": 0.0}
    least = {}
    for name, case in chk.cases().items():
        state = case.state()
        fair = {"lse": chk.judge_lse(case, state, ref.lse_f32(case.csr, state, case.gb)),
                "mass": chk.judge_mass(case, state, ref.mass_f32(case.csr, state, case.gb)),
                "gradient": chk.judge(case, state, ref.gradient_f32(case.csr, state, case.gb, case.hyper, case.side))}
        print("%s: restatement at %s of the bounds" % (name, {k: round(v, 4) for k, v in fair.items()}))
        for k, v in fair.items():
            assert v <= 0.5, (name, k, v)
            worst[k] = max(worst[k], v)
        for mutation in ref.MUTATIONS:
            if not chk.claimed(case, mutation):
                continue
            seen[mutation] += 1
            r = chk.judge(case, state, ref.gradient(case.csr, state, case.gb, case.hyper, case.side, mutation=mutation))
            least[mutation] = min(least.get(mutation, np.inf), r)
            assert r > 1.0, (name, mutation, r)
    print("worst restatement: %s; least mutation: %s" % (worst, least))
    assert all(n > 0 for n in seen.values()), seen


def test_large_scores_overflow_a_raw_exponential():
    for side in ("users", "items"):
        case = chk.large_score_case(side)
        S = chk.scores_of(tuple(a[:n] for a, n in zip(case.state(), (case.csr.rows, case.csr.cols) * 2)), case.gb)
        assert S.max() > 150 and S.min() < -150, (S.min(), S.max())
        g = ref.gradient(case.csr, case.state(), case.gb, case.hyper, side)
        assert np.isfinite(g[0]).all() and np.isfinite(g[1]).all()
        assert np.isfinite(ref.lse_f32(case.csr, case.state(), case.gb)).all()


def test_objective_restatement_error():
    """The float32-lse objective against float64 on lmf_checks.OBJECTIVE_SETS; the GPU test allows svd_checks.MARGIN times the
    recorded figure."""
    worst = 0.0
    for name in chk.OBJECTIVE_SETS:
        case = chk.cases()[name]
        want = ref.objective(case.csr, case.state(), case.gb, case.hyper)
        got = ref.objective_f32(case.csr, case.state(), case.gb, case.hyper)
        rel = abs(got - want) / abs(want)
        print("%s: objective %.9g, float32 lse off by %.3g" % (name, want, rel))
        worst = max(worst, rel)
    assert worst <= chk.OBJECTIVE_RESTATEMENT_ERROR


def test_the_ml_small_experiment_in_float64_and_its_restatement():
    """f = 64, lr = 0.15, every regulariser 1, the stored values taken as 1, 6 sweeps from the library's seed-42 start, every user's
    last entry held out: float64 lists the held-out item in the top 10 for softmax_checks.ML_SMALL_HITS of 610 users (recorded).  The
    float32 restatement in the kernels' order stays within the recorded distances of the float64 run -- the objective at every
    half-step, the factors and the scores at the end -- which the GPU test scales by svd_checks.MARGIN, and the users whose hit such
    a run may decide differently are the recorded count."""
    tr, _ = chk.ml_small()
    s64, o64 = chk.ml_small_run64()
    hits = chk.hits_of(s64)
    print("float64: %d hits; objective %s" % (hits, ["%.1f" % o for o in o64]))
    assert hits == chk.ML_SMALL_HITS
    s32, o32 = ref.run(tr, chk.ml_small_start(), tr.global_bias, chk.ML_SMALL_HYPER, chk.ML_SMALL_SWEEPS, f32=True)
    objective_distance = max(abs(a - b) / abs(b) for a, b in zip(o32, o64))
    factor_distance = max(np.abs(np.asarray(a, np.float64) - b).max() for a, b in zip(s32, s64))
    S64 = chk.scores_of(s64, tr.global_bias)
    score_distance = np.abs(chk.scores_of(s32, tr.global_bias) - S64).max() / np.abs(S64).max()
    reach = chk.within_reach(chk.ML_SMALL_SCORE_DISTANCE)
    print("objective distance %.3g, factor distance %.3g, score distance %.3g, restatement hits %d, within reach %d (at the measured distance: %d)"
          % (objective_distance, factor_distance, score_distance, chk.hits_of(s32), reach, chk.within_reach(score_distance)))
    assert objective_distance <= chk.ML_SMALL_OBJECTIVE_DISTANCE
    assert factor_distance <= chk.ML_SMALL_FACTOR_DISTANCE
    assert score_distance <= chk.ML_SMALL_SCORE_DISTANCE
    assert reach == chk.ML_SMALL_WITHIN_REACH
    assert abs(chk.hits_of(s32) - hits) <= reach
    assert same_user_biases(s32, s64)


def same_user_biases(a, b):
    return np.array_equal(np.asarray(a[2], np.float64), np.asarray(b[2], np.float64))


def test_null_arguments_are_einval_without_a_device():
    L = cu.lib()
    assert L.cu2rec_model_softmax(None, None, None, 0, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_model_softmax_gradient(None, None, None, 0, None, None) == -1
    assert L.cu2rec_model_softmax_objective(None, None, None, None) == -1
    assert L.cu2rec_model_softmax_lse(None, None, None) == -1
    assert L.cu2rec_model_softmax_mass(None, None, None) == -1
    assert L.cu2rec_train_softmax(None, None, None, 0, None, None) == -1


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    for name in ("cu2rec_model_softmax", "cu2rec_model_softmax_gradient", "cu2rec_model_softmax_objective", "cu2rec_model_softmax_lse",
                 "cu2rec_model_softmax_mass", "cu2rec_train_softmax"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cu._lib.SIGNATURES


def test_python_front_end():
    assert "softmax" not in api.MODES  # the SGD mode table is unchanged: train() handles the string itself
    blank = object.__new__(cu.Model)  # no device object behind it: the side is refused before anything is called
    blank._h = None
    with pytest.raises(ValueError):
        cu.Model.softmax(blank, None, chk.HYPER, side="rows")
    with pytest.raises(ValueError):
        cu.Model.softmax_gradient(blank, None, chk.HYPER, "both")


def test_mf_usage_lists_softmax_and_refuses_what_it_does_not_take():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bsoftmax\b", usage[0]), res.stderr
    for flag in (["-a", "2"], ["-C", "3"], ["-g", "2"], ["-s", "4"], ["-w", "mean"], ["-W", "cosine"], ["-N", "5"], ["-L", "10"],
                 ["-l", "1"], ["-n", "3"]):
        res = subprocess.run([mf, "-m", "softmax"] + flag + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (flag, res.stderr)
