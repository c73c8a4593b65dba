"""Logistic matrix factorization without a GPU: the float64 reference and the float32 restatement of tests/lmf_reference64.py on the
sets the GPU tests judge (tests/lmf_checks.py) -- the bound is fair to a correct float32 evaluation and every deliberate mistake
breaks it -- the step and multi-sweep restatements, and what the C ABI, the Python front end and bin/mf refuse before any device is
touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import lmf_checks as chk
import lmf_reference64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_cases():
    out = dict(chk.cases())
    for side in ("users", "items"):
        case = chk.saturated_case(side)
        out[case.name] = case
    return out


def judge(case, got):
    state = case.state()
    g, gb = ref.gradient(case.csr, state, case.gb, case.hyper, case.alpha, case.side)
    b, bb = ref.bound(case.csr, state, case.gb, case.hyper, case.alpha, case.side)
    return max(ref.ratio(got[0], g, b), ref.ratio(got[1], gb, bb))


def test_bound_is_fair_and_every_mutation_breaks_it():
    """On every set the GPU tests judge: the float32 restatement in the kernels' order is within 0.5 of the bound on every row (worst
    measured: 0.18, at one partner), and each deliberate mistake is above 1 wherever lmf_checks.claimed() says it shows (least
    measured: 4.6, the last of 32 partners dropped against a single own row at f = 191); every mistake is claimed on some set."""
    seen = dict.fromkeys(ref.MUTATIONS, 0)
    for name, case in all_cases().items():
        state = case.state()
        fair = judge(case, ref.gradient_f32(case.csr, state, case.gb, case.hyper, case.alpha, case.side))
        print("%s: restatement %.4f of the bound" % (name, fair))
        assert fair <= 0.5, (name, fair)
        for mutation in ref.MUTATIONS:
            if not chk.claimed(case, mutation):
                continue
            seen[mutation] += 1
            r = judge(case, ref.gradient(case.csr, state, case.gb, case.hyper, case.alpha, case.side, mutation=mutation))
            assert r > 1.0, (name, mutation, r)
    assert all(n > 0 for n in seen.values()), seen


def test_saturated_sets_reach_scores_of_200_both_ways():
    for side in ("users", "items"):
        case = chk.saturated_case(side)
        _, _, _, X, xb, Y, yb, _, _ = ref.sides(case.csr, case.state(), case.hyper, case.side)
        S = case.gb + xb[:, None] + yb[None, :] + X.astype(np.float64) @ Y.astype(np.float64).T
        assert S.max() > 150 and S.min() < -150, (S.min(), S.max())


def test_grid_covers_what_the_issue_lists():
    cases = chk.cases()
    shapes = {(c.f, c.csr.rows, c.csr.cols) for c in cases.values() if c.side == "users"}
    assert {s[0] for s in shapes} == set(chk.WIDTHS)
    assert {s[1] for s in shapes} == set(chk.OWN_ROWS) and {s[2] for s in shapes} == set(chk.PARTNERS)
    lengths = set()
    for c in cases.values():
        if c.side == "users":
            lengths |= set(np.diff(c.csr.indptr).tolist())
            assert c.csr.nnz == 0 or c.csr.indices.max() < c.csr.cols
    assert {0, 1, 2, 300} <= lengths
    big = cases["f100-65x1000"].csr
    assert big.indices.max() < big.cols - 1 and (np.diff(big.indices[:300]) < 0).any()  # cols past every stored item; unsorted


def test_step_restatement_against_float64():
    """x' within 2^-22 max(|x'|, lr) and a' within 2^-23 relative of the float64 step: four correctly rounded operations (g g, the
    sum, the square root and the quotient's chain) each add at most 2^-24 relative; the final sum one more on |x'|."""
    rng = np.random.default_rng(3)
    lr = float(np.float32(0.2))  # the learning rate as the device holds it
    x = rng.normal(0, 1, 4000).astype(np.float32)
    g = (rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-6, 4, 4000)).astype(np.float32)
    a = np.where(rng.random(4000) < 0.3, 0, rng.random(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    g[:10] = 0.0
    a[:5] = 0.0  # a' = 0: the value stays
    x32, a32 = ref.step_f32(x, a, g, lr)
    x64, a64 = ref.step(x, a, g, lr)
    assert np.array_equal(x32[:5], x[:5])
    assert (np.abs(x32 - x64) <= 2.0 ** -22 * np.maximum(np.abs(x64), lr)).all()
    assert (np.abs(a32 - a64) <= 2.0 ** -23 * a64).all()


def test_objective_restatement_error():
    """The float32-score objective against float64 on lmf_checks.OBJECTIVE_SETS; the GPU test allows four times the worst."""
    worst = 0.0
    for name in chk.OBJECTIVE_SETS:
        case = chk.cases()[name]
        want = ref.objective(case.csr, case.state(), case.gb, case.hyper, case.alpha)
        got = ref.objective_f32(case.csr, case.state(), case.gb, case.hyper, case.alpha)
        rel = abs(got - want) / abs(want)
        print("%s: objective %.9g, float32 scores off by %.3g" % (name, want, rel))
        worst = max(worst, rel)
    assert worst <= chk.OBJECTIVE_RESTATEMENT_ERROR


def test_eight_sweeps_of_the_restatement_on_ml_small():
    """f = 32, alpha = 2, lr = 0.2, P_reg = Q_reg = 0.6, 8 sweeps from the library's seed-42 initial model: the float32 restatement in the kernels'
    order stays within 5.56e-8 (relative) of the float64 run's objective at every one of the 16 half-steps and ends within 6.90e-7
    of its factors and biases (measured; asserted against lmf_checks.FIXTURE_*, which the GPU test scales).  The float64 objective
    rises at every half-step."""
    tr, start = chk.fixture()
    s64, o64 = chk.fixture_run64()
    s32, o32 = ref.run(tr, start, tr.global_bias, chk.FIXTURE_HYPER, chk.FIXTURE_ALPHA, chk.FIXTURE_SWEEPS, f32=True)
    objective_distance = max(abs(a - b) / abs(b) for a, b in zip(o32, o64))
    factor_distance = max(np.abs(np.asarray(a, np.float64) - b).max() for a, b in zip(s32, s64))
    print("objective distance %.3g, factor distance %.3g" % (objective_distance, factor_distance))
    assert objective_distance <= chk.FIXTURE_OBJECTIVE_DISTANCE
    assert factor_distance <= chk.FIXTURE_FACTOR_DISTANCE
    assert all(b > a for a, b in zip(o64, o64[1:]))


def test_null_arguments_are_einval_without_a_device():
    L = cu.lib()
    assert L.cu2rec_model_lmf(None, None, None, 1.0, 0, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_model_lmf_gradient(None, None, None, 1.0, 0, None, None) == -1
    assert L.cu2rec_model_lmf_objective(None, None, None, 1.0, None) == -1
    assert L.cu2rec_model_lmf_state(None, None, None, None, None) == -1
    assert L.cu2rec_model_lmf_reset(None) == -1
    assert L.cu2rec_train_lmf(None, None, None, 1.0, 0, None, None) == -1


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    for name in ("cu2rec_model_lmf", "cu2rec_model_lmf_gradient", "cu2rec_model_lmf_objective", "cu2rec_model_lmf_state",
                 "cu2rec_model_lmf_reset", "cu2rec_train_lmf"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cu._lib.SIGNATURES


def test_python_front_end():
    assert "lmf" not in api.MODES  # the SGD mode table is unchanged: train() handles the string itself
    import inspect
    assert inspect.signature(cu.Model.lmf).parameters["alpha"].default == 1.0
    blank = object.__new__(cu.Model)  # no device object behind it: the side is refused before anything is called
    blank._h = None
    with pytest.raises(ValueError):
        cu.Model.lmf(blank, None, chk.HYPER, side="rows")
    with pytest.raises(ValueError):
        cu.Model.lmf_gradient(blank, None, chk.HYPER, 1.0, "both")


def test_mf_usage_lists_lmf_and_refuses_several_gpus_and_cg_steps():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bials\|lmf\b", usage[0]), res.stderr
    for args in (["-m", "lmf", "-g", "2"], ["-m", "lmf", "-C", "3"]):
        res = subprocess.run([mf] + args + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)
