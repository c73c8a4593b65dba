"""Bayesian Personalized Ranking without a GPU: the float64 reference and the float32 restatement of tests/bpr_reference64.py on the
sets the GPU tests judge (tests/bpr_checks.py) -- the bound is fair to a correct float32 evaluation and every deliberate mistake
breaks it -- the objective's and the multi-sweep restatements, whose measured distances the GPU suite scales, and what the C ABI,
the Python front end and bin/mf refuse before any device is touched."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import bpr_checks as chk
import bpr_reference64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_cases():
    out = dict(chk.cases())
    for side in ("users", "items"):
        case = chk.saturated_case(side)
        out[case.name] = case
    return out


def judge(case, got):
    state, neg = case.state(), case.negatives()
    g, gb = ref.gradient(case.csr, state, case.hyper, neg, case.side)
    b, bb = ref.bound(case.csr, state, case.hyper, neg, case.side)
    return max(ref.ratio(got[0], g, b), ref.ratio(got[1], gb, bb))  # a zero bound (the users' bias) admits only the exact value


def test_negatives_obey_the_definition():
    """Independently of how negatives() walks: every negative is outside its row, a -1 means that all eight draws are stored items, a
    row that stores every column has only -1, a row that lacks one column only that column or -1, cols == 1 gives -1 everywhere, and
    the draw of a row alone equals its draw among the others."""
    for name, csr in chk.negative_sets().items():
        for seed in chk.SEEDS:
            for sweep in chk.SWEEPS:
                neg = ref.negatives(csr, seed, sweep)
                for u in range(csr.rows):
                    lo, hi = csr.indptr[u], csr.indptr[u + 1]
                    stored = set(csr.indices[lo:hi].tolist())
                    assert all(j == -1 or (0 <= j < csr.cols and j not in stored) for j in neg[lo:hi].tolist()), (name, u)
                    for k in np.flatnonzero(neg[lo:hi] < 0)[:3]:
                        draws = [api.sampler_index(seed, u, ((sweep * 8 + a) << 32) | int(k), 0, csr.cols) for a in range(8)]
                        assert all(d in stored for d in draws)
    full = chk.negative_sets()["33x40"]
    neg = ref.negatives(full, 42, 0)
    assert (neg[:full.indptr[1]] == -1).all() and set(neg[full.indptr[1]:full.indptr[2]].tolist()) == {-1, 17}
    assert (ref.negatives(chk.negative_sets()["5x1"], 42, 1) == -1).all()
    big = chk.negative_sets()["65x1000"]
    one = big.slice_users(9, 10)
    alone = api.HostCSR(np.concatenate([np.zeros(10, np.int64), np.full(56, one.nnz)]), one.indices, one.data, 65, 1000, 0.0)
    assert np.array_equal(ref.negatives(alone, 42, 1), ref.negatives(big, 42, 1)[big.indptr[9]:big.indptr[10]])
    assert not np.array_equal(ref.negatives(big, 42, 0), ref.negatives(big, 42, 1))
    assert not np.array_equal(ref.negatives(big, 42, 0), ref.negatives(big, chk.SEEDS[1], 0))


def test_bound_is_fair_and_every_mutation_breaks_it():
    """On every set the GPU tests judge: the float32 restatement in the kernels' order is within bpr_checks.RESTATEMENT_WORST of the
    bound on every row, and each deliberate mistake is above 1 wherever bpr_checks.claimed() says it shows (least measured:
    bpr_checks.MUTATION_LEAST); every mistake is claimed on some set."""
    seen = dict.fromkeys(ref.MUTATIONS, 0)
    worst, least = 0.0, np.inf
    for name, case in all_cases().items():
        state, neg = case.state(), case.negatives()
        fair = judge(case, ref.gradient_f32(case.csr, state, case.hyper, neg, case.side))
        print("%s: restatement %.4f of the bound" % (name, fair))
        worst = max(worst, fair)
        for mutation in ref.MUTATIONS:
            if not chk.claimed(case, mutation):
                continue
            seen[mutation] += 1
            if mutation in ref.NEGATIVE_MUTATIONS:
                got = ref.gradient(case.csr, state, case.hyper, ref.negatives(case.csr, chk.GRADIENT_SEED, chk.GRADIENT_SWEEP, mutation), case.side)
            else:
                got = ref.gradient(case.csr, state, case.hyper, neg, case.side, mutation=mutation)
            r = judge(case, got)
            least = min(least, r)
            assert r > 1.0, (name, mutation, r)
    print("worst restatement %.4f, least mistake %.4g" % (worst, least))
    assert worst <= chk.RESTATEMENT_WORST <= 0.5 and least >= chk.MUTATION_LEAST > 1.0
    assert all(n > 0 for n in seen.values()), seen


def test_saturated_sets_reach_scores_of_200_both_ways():
    case = chk.saturated_case("users")
    neg = case.negatives()
    x = ref.scores(case.csr, case.state(), neg)[neg >= 0]
    assert x.max() > 150 and x.min() < -150, (x.min(), x.max())


def test_grid_covers_what_the_issue_lists():
    cases = chk.cases()
    assert {c.f for c in cases.values()} == set(chk.WIDTHS)
    assert all(name + "-items" in cases for name in cases if not name.endswith("-items"))
    big = cases["f100-65x1000"].csr
    assert set(np.diff(big.indptr).tolist()) == set(chk.ROW_LENGTHS) == {0, 1, 2, 3, 4, 5, 7, 40, 300}
    assert big.indices.max() < big.cols - 1 and (np.diff(big.indices[:300]) < 0).any()  # cols past every stored item; unsorted
    rows = np.repeat(np.arange(big.rows), np.diff(big.indptr))
    assert len(np.unique(rows * big.cols + big.indices)) < big.nnz  # repeated pairs
    neg = cases["f100-65x1000"].negatives()
    pos_items, neg_items = set(big.indices.tolist()), set(neg[neg >= 0].tolist())
    everything = set(range(big.cols))
    assert pos_items - neg_items and neg_items - pos_items and pos_items & neg_items and everything - pos_items - neg_items
    full = cases["f252-33x40"]
    assert (full.negatives() < 0).any() and (full.negatives() >= 0).any()  # entries without a triple among the judged gradients
    state = cases["f100-65x1000"].state()
    assert state[0].shape[0] > big.rows and state[1].shape[0] > big.cols and state[3].any()


def test_objective_restatement_error():
    """The objective added up in the device's order against numpy's float64 on bpr_checks.OBJECTIVE_SETS, and the counts' identity;
    the GPU test allows four times bpr_checks.OBJECTIVE_RESTATEMENT_ERROR."""
    worst = 0.0
    for name in chk.OBJECTIVE_SETS:
        case = chk.cases()[name]
        want, n, m = ref.objective(case.csr, case.state(), case.hyper, case.negatives())
        got = ref.objective_blocked(case.csr, case.state(), case.hyper, case.negatives())
        rel = abs(got - want) / abs(want)
        print("%s: objective %.15g over %d triples (%d ordered), the device's order off by %.3g" % (name, want, n, m, rel))
        assert n == (case.negatives() >= 0).sum() and 0 < m < n
        worst = max(worst, rel)
    assert worst <= chk.OBJECTIVE_RESTATEMENT_ERROR


def test_sweeps_of_the_restatement_on_ml_small():
    """The fixture run of bpr_checks (f = 32, every user's last entry held out): the float32 restatement in the kernels' order against
    the float64 run -- the objective's relative distance at every half-step, the worst factor distance at the end, the worst score
    distance on the last sweep's triples, and from that the triples and the held-out hits that a perturbation of eight times that
    size could flip: the margins of the GPU test's ranking figures.  The recorded reference values are this run's."""
    train, held, start = chk.fixture()
    s64, o64 = chk.fixture_run64()
    s32, o32 = ref.run(train, start, chk.FIXTURE_HYPER, chk.FIXTURE_SEED, chk.FIXTURE_SWEEPS, f32=True)
    R = chk.FIXTURE_REFERENCE
    objective_distance = max(abs(a[0] - b[0]) / abs(b[0]) for a, b in zip(o32, o64))
    factor_distance = max(np.abs(np.asarray(a, np.float64) - b).max() for a, b in zip(s32, s64))
    neg = ref.negatives(train, chk.FIXTURE_SEED, chk.FIXTURE_SWEEPS - 1)
    x64, x32 = ref.scores(train, s64, neg)[neg >= 0], ref.scores(train, s32, neg)[neg >= 0]
    score_distance = np.abs(x32 - x64).max()
    auc_flips = int((np.abs(x64) <= 8 * score_distance).sum())
    hit64, hit_flips = chk.hit_rate_at_10(train, held, s64, margin=16 * score_distance)
    hit32, _ = chk.hit_rate_at_10(train, held, s32)
    hit0, _ = chk.hit_rate_at_10(train, held, start)
    auc0 = ref.objective(train, start, chk.FIXTURE_HYPER, neg)
    print("objective distance %.3g, factor distance %.3g, score distance %.3g" % (objective_distance, factor_distance, score_distance))
    print("objectives %s" % [round(o[0], 6) for o in o64])
    print("triples %s ordered %s" % ([o[1] for o in o64], [o[2] for o in o64]))
    print("auc: float64 %.6f float32 %.6f untrained %.6f, triples within reach %d" % (o64[-1][2] / o64[-1][1], o32[-1][2] / o32[-1][1],
                                                                                     auc0[2] / auc0[1], auc_flips))
    print("hit rate @10: float64 %.6f float32 %.6f untrained %.6f, users within reach %d" % (hit64, hit32, hit0, hit_flips))
    assert objective_distance <= R["objective_distance"] and factor_distance <= R["factor_distance"] and score_distance <= R["score_distance"]
    assert np.allclose([o[0] for o in o64], R["objectives"], rtol=0, atol=1e-6)  # recorded to six decimals
    assert [o[1] for o in o64] == R["triples"] and [o[2] for o in o64] == R["ordered"]
    assert auc_flips == R["auc_flips"] and hit_flips == R["hit_flips"] and abs(hit64 - R["hit_rate"]) < 1e-12
    assert abs(o32[-1][2] - o64[-1][2]) <= auc_flips and abs(hit32 - hit64) * train.rows <= hit_flips + 1e-9
    # trained clearly above untrained, on both figures
    assert o64[-1][2] / o64[-1][1] > 0.85 > 0.55 > auc0[2] / auc0[1]
    assert hit64 * train.rows >= 8 and hit0 == 0.0


def test_null_arguments_are_einval_without_a_device():
    L = cu.lib()
    assert L.cu2rec_model_bpr(None, None, None, 42, 0, 0, None) == -1  # CU2REC_EINVAL, before any device is touched
    assert "null" in L.cu2rec_last_error().decode()
    assert L.cu2rec_model_bpr_gradient(None, None, None, 42, 0, 0, None, None) == -1
    assert L.cu2rec_model_bpr_objective(None, None, None, 42, 0, None, None, None) == -1
    assert L.cu2rec_csr_bpr_negatives(None, 42, 0, None) == -1
    assert L.cu2rec_train_bpr(None, None, None, 0, None, None) == -1


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    for name in ("cu2rec_model_bpr", "cu2rec_model_bpr_gradient", "cu2rec_model_bpr_objective", "cu2rec_csr_bpr_negatives", "cu2rec_train_bpr"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cu._lib.SIGNATURES


def test_python_front_end():
    assert "bpr" not in api.MODES  # the SGD mode table is unchanged: train() handles the string itself
    params = inspect.signature(cu.Model.bpr).parameters
    assert [params[k].default for k in ("seed", "sweep0", "side", "sweeps")] == [42, 0, "both", 1]
    blank = object.__new__(cu.Model)  # no device object behind it: the side is refused before anything is called
    blank._h = None
    with pytest.raises(ValueError):
        cu.Model.bpr(blank, None, chk.HYPER, side="rows")
    with pytest.raises(ValueError):
        cu.Model.bpr_gradient(blank, None, chk.HYPER, 42, 0, "both")


def test_mf_usage_lists_bpr_and_refuses_alpha_cg_steps_and_several_gpus():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\blmf\|bpr\b", usage[0]), res.stderr
    for args in (["-m", "bpr", "-a", "2"], ["-m", "bpr", "-C", "3"], ["-m", "bpr", "-g", "2"]):
        res = subprocess.run([mf] + args + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)
