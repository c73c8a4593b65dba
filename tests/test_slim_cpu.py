"""SLIM without a GPU: what the header, the C ABI, the Python front end and bin/mf declare and refuse before any device is touched; that
the float32 restatement of tests/slim_reference64.py in the device's order passes the judgements of tests/slim_checks.py on every table
and that every deliberate mistake fails them on some table; the restatement's measured distance from float64 per table; the EASE
limit; the stops the GPU test is held to; and the ML_SMALL experiment in float64."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api

import ease_reference64 as eref
import knn_reference64 as kref
import slim_checks as chk
import slim_reference64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def restated(name, sweeps):
    """W32 of a table after `sweeps` sweeps: the float32 restatement, once per process."""
    case = chk.cases()[name]
    W, _ = ref.blocked(eref.gram_f32(case.train, case.l2), case.l1, case.positive, sweeps, chk.block_items())
    W.setflags(write=False)
    return W


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "cu2rec_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint cu2rec_slim_create\(const cu2rec_csr \*train, float l1, float l2, int positive, int max_sweeps, float tol,", header)
    assert re.search(r"typedef struct \{ int sweeps; float last_delta; long long nonzeros; \} cu2rec_slim_report;", header)
    assert header.index("cu2rec_slim_create(const") > header.index("int cu2rec_ease_rank_metrics(")  # the SLIM section follows EASE's
    assert "cu2rec_slim_create" in cu._lib.SIGNATURES
    assert [n for n, _ in cu._lib.SlimReport._fields_] == ["sweeps", "last_delta", "nonzeros"]
    assert not [n for n in cu._lib.SIGNATURES if n.startswith("cu2rec_slim_") and n != "cu2rec_slim_create"]  # served by cu2rec_ease_*


def test_refusals_without_a_device():
    """Bad l1, l2, max_sweeps and tol are CU2REC_EINVAL from the arguments alone, before the handle is looked at."""
    L = cu.lib()
    h = api.C.c_void_p()

    def create(l1=5.0, l2=500.0, sweeps=3, tol=0.0, out=h):
        return L.cu2rec_slim_create(None, l1, l2, 1, sweeps, tol, None, api.C.byref(out) if out is not None else None)

    for kw, word in ([(dict(l1=v), "l1") for v in (-1.0, float("nan"), float("inf"))] +
                     [(dict(l2=v), "l2") for v in (0.0, -1.0, float("nan"), float("inf"))] +
                     [(dict(sweeps=v), "max_sweeps") for v in (0, -2)] + [(dict(tol=v), "tol") for v in (-1e-3, float("nan"))]):
        assert create(**kw) == -1 and h.value is None, kw
        assert word in L.cu2rec_last_error().decode(), kw
    assert create() == -1 and "null" in L.cu2rec_last_error().decode()
    assert create(out=None) == -1


def test_python_front_end():
    p = inspect.signature(cu.SLIM.__init__).parameters
    assert list(p)[1:] == ["train", "l1", "l2", "positive", "sweeps", "tol"]
    assert [p[n].default for n in list(p)[2:]] == [5.0, 500.0, True, 10, 1e-3]
    assert issubclass(cu.SLIM, cu.EASE) and cu.SLIM is api.SLIM
    for method in ("weights", "neighbors", "recommend", "rank_metrics", "close"):
        assert getattr(cu.SLIM, method) is getattr(cu.EASE, method)


def test_mf_usage_and_refusals_before_the_gpu():
    mf = os.path.join(ROOT, "bin", "mf")
    res = subprocess.run([mf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    usage = [line for line in res.stderr.splitlines() if line.startswith("usage: mf")]
    assert usage and re.search(r"-m [a-z|]*\bease\|slim\]", usage[0]) and "[-L l2]" in usage[0] and "[-l l1]" in usage[0] and "[-n sweeps]" in usage[0]
    s = ["-m", "slim", "-k", "5"]
    refused = (["-m", "slim"], ["-l", "5", "-k", "5"], ["-n", "3", "-k", "5"], ["-m", "ease", "-l", "5", "-k", "5"], ["-m", "ease", "-n", "3", "-k", "5"],
               ["-m", "knn", "-L", "500", "-k", "5"], ["-L", "500", "-k", "5"], s + ["-L", "0"], s + ["-L", "nan"], s + ["-l", "-1"], s + ["-l", "lots"],
               s + ["-l", "inf"], s + ["-n", "0"], s + ["-n", "two"], s + ["-c", "some.cfg"], s + ["-a", "2"], s + ["-C", "3"], s + ["-g", "2"],
               s + ["-s", "4"], s + ["-w", "mean"], s + ["-W", "cosine"], s + ["-N", "20"])
    for args in refused:
        res = subprocess.run([mf] + args + ["missing_train.csv", "missing_test.csv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert res.returncode != 0 and "usage: mf" in res.stderr and "Free memory" not in res.stdout, (args, res.stderr)


def test_the_tables():
    nb = chk.block_items()
    cases = chk.cases()
    assert sorted(c.train.cols for c in cases.values()) == sorted((1, 2, nb - 1, nb, nb + 1, 2 * nb + 1, 5 * nb + 3, 32 * nb + 1) * 2)
    assert set(chk.SLIM_DISTANCE) == set(cases)
    assert {c.l2 for c in cases.values()} == set(chk.echk.L2S) and {c.l1 for c in cases.values()} == set(chk.L1S)
    for kind in ("full", "sparse"):
        assert {c.positive for n, c in cases.items() if n.endswith(kind)} == {True, False}
    for name, case in cases.items():
        assert not kref.sorted_rows(case.train)[1]
        some = chk.some_but_not_all_zero(name)  # l1 leaves some but not all weights zero in float64
        assert some is True or (some is None and case.train.cols <= 2), name
    assert any(chk.unstored(c.train).any() for c in cases.values())


def test_the_two_float64_forms_agree():
    """Plainly as written, and through R = X W: the same W and the same largest |delta| per sweep."""
    for name, case in chk.cases().items():
        if case.train.cols > 2 * chk.block_items() + 1:
            continue
        A = chk.gram64(name)
        W, tops = ref.sweeps64(A, case.l1, case.positive, chk.SWEEPS)
        V, tops2, R = ref.sweeps64_rows(case.train, np.diag(A), case.l1, case.positive, chk.SWEEPS)
        assert np.abs(W - V).max(initial=0.0) <= 1e-13 and np.allclose(tops, tops2, rtol=1e-10, atol=1e-13), name
        assert np.abs(R - eref.dense(case.train) @ V).max(initial=0.0) <= 1e-12
        # and the blocked form in float64 is the same sequence
        Wb, tops3 = ref.blocked(A, case.l1, case.positive, chk.SWEEPS, chk.block_items(), np.float64)
        assert np.abs(W - Wb).max(initial=0.0) <= 1e-13 and np.allclose(tops, tops3, rtol=1e-10, atol=1e-13), name


def test_restatement_distance():
    """max |W - W64| / max |W64| of the restatement after SWEEPS sweeps per table: the figures slim_checks records."""
    for name in chk.cases():
        dist = chk.distance(restated(name, chk.SWEEPS), chk.weights64(name, chk.SWEEPS))
        print("%-12s distance %.3g (recorded %.3g)" % (name, dist, chk.SLIM_DISTANCE[name]))
        assert 0.5 * chk.SLIM_DISTANCE[name] <= dist <= chk.SLIM_DISTANCE[name], name


def test_restatement_passes_every_judgement():
    for name in chk.cases():
        for sweeps in chk.COUNTS:
            assert not chk.judge_weights(name, restated(name, sweeps), sweeps), (name, sweeps)


def test_every_deliberate_mistake_is_caught_on_some_table():
    """Each mistake in the blocked form in float64, judged like the device at 1, 2 and 3 sweeps; the first table and count that
    catches it.  A mistake in how C is updated can only show in a later read of C: two of them need a second sweep where the table
    is one tile."""
    nb = chk.block_items()
    tables = [c for c in chk.cases().values() if c.train.cols <= 5 * nb + 3]
    caught = dict.fromkeys(ref.MUTATIONS)
    first_sweep = {}
    for mutation in ref.MUTATIONS:
        for case in tables:
            A = chk.gram64(case.name)
            for sweeps in chk.COUNTS:
                W, _ = ref.blocked(A, case.l1, case.positive, sweeps, nb, np.float64, mutation, case.l2)
                if chk.judge_weights(case.name, W, sweeps):
                    caught[mutation] = caught[mutation] or (case.name, sweeps)
                    first_sweep.setdefault(mutation, {})[case.name] = sweeps
                    break
    print(caught)
    assert all(caught.values()), caught
    one_tile = [c.name for c in tables if 2 < c.train.cols <= nb]
    late = [m for m in ref.MUTATIONS if all(first_sweep[m].get(n, 9) >= 2 for n in one_tile)]
    assert set(late) >= {"own_rows_left_out", "tile_skipped"}, late
    for case in tables:  # and the unmutated blocked form passes in float64
        for sweeps in chk.COUNTS:
            W, _ = ref.blocked(chk.gram64(case.name), case.l1, case.positive, sweeps, nb, np.float64)
            assert not chk.judge_weights(case.name, W, sweeps)


def test_the_ease_limit():
    """l1 = 0 and free signs on the l2 = 500 tables: float64 coordinate descent reaches EASE's closed form within 1e-6 x max |B| in at
    most 50 sweeps on the tables of EASE_LIMIT (and on no other l2 = 500 table), after the recorded sweeps; the two float32 restatements
    are the recorded distance apart."""
    nb = chk.block_items()
    for name, case in chk.cases().items():
        if case.l2 != 500.0:
            continue
        A = chk.gram64(name)
        B = eref.weights(A)
        top = float(np.abs(B).max())
        _, tops, _ = ref.sweeps64_rows(case.train, np.diag(A), 0.0, False, chk.EASE_LIMIT_CAP,
                                       until=lambda W: np.abs(W - B).max() <= chk.EASE_LIMIT_TOL * top)
        if name not in chk.EASE_LIMIT:
            assert len(tops) == chk.EASE_LIMIT_CAP, name  # the cap is a condition: this table does not meet it
            continue
        sweeps, recorded = chk.EASE_LIMIT[name]
        assert len(tops) == sweeps, (name, len(tops))
        A32 = eref.gram_f32(case.train, case.l2)
        W32, _ = ref.blocked(A32, 0.0, False, sweeps, nb)
        dist = float(np.abs(W32.astype(np.float64) - eref.weights_f32(A32, nb)).max() / top)
        print("%-12s %2d sweeps, restatements %.3g apart (recorded %.3g)" % (name, sweeps, dist, recorded))
        assert 0.5 * recorded <= dist <= recorded, name
    assert len(chk.EASE_LIMIT) >= 3 and any(chk.cases()[n].train.cols > nb for n in chk.EASE_LIMIT)


def test_the_stops():
    """The float64 sequence of largest |delta| of every STOPS run stays a factor of 4 away from tol on both sides of the stopping
    sweep; the float32 restatement stops at the same sweep."""
    for name, (l1, l2, positive, tol, stop) in chk.STOPS.items():
        case = chk.cases()[name]
        diag = np.diag(eref.gram(case.train, l2))
        _, tops, _ = ref.sweeps64_rows(case.train, diag, l1, positive, stop)
        print(name, " ".join("%.3g" % t for t in tops), "tol %g" % tol)
        assert stop >= 3 and all(t >= 4 * tol for t in tops[:-1]) and 0 < tops[-1] <= tol / 4, name
        W32, tops32 = ref.blocked(eref.gram_f32(case.train, l2), l1, positive, chk.STOP_CAP, chk.block_items(), tol=tol)
        assert len(tops32) == stop and tops32[-1] <= tol, name
        assert tops[-1] >= 100 * 2.0 ** -24 * float(np.abs(W32).max())  # well above float32's resolution of the weights
    assert len({chk.cases()[n].train.cols for n in chk.STOPS}) >= 3 and {v[2] for v in chk.STOPS.values()} == {True, False}


def test_ml_small_experiment_in_float64():
    """Every user's last stored entry held out, l1 = 5, l2 = 500, non-negative, 3 sweeps: hits @10 of 610 users, the nonzero fraction
    and the users within reach of a float32 flip -- the records of slim_checks, which the GPU test is held to."""
    train, held = chk.ml_small()
    hits, W, _, _ = chk.ml_small_run()
    reach = chk.within_reach(chk.ml_distance())
    nonzero = float((W != 0).mean())
    print("SLIM l1 = %g, l2 = %g, %d sweeps: %d hits @%d of %d users; %.4f of W nonzero; users within reach: %d"
          % (chk.ML_SMALL_L1, chk.ML_SMALL_L2, chk.ML_SMALL_SWEEPS, hits, chk.ML_SMALL_K, train.rows, nonzero, reach))
    assert hits == chk.ML_SMALL_SLIM_HITS and reach == chk.ML_SMALL_SLIM_WITHIN_REACH
    assert abs(nonzero - chk.ML_SMALL_SLIM_NONZERO) <= 5e-5
    assert hits > chk.echk.ML_SMALL_EASE_HITS > chk.kchk.ML_SMALL_HITS["cosine"]
