"""The float64 sequential reference (tests/sgd_reference64.py) against the C oracle, with distinct hyper-parameters (CPU).

The oracle's float32 trajectory must lie inside the reference's running float32-rounding bound for every parameter, in both dot
orders, and the bound must be tight enough to matter: the reference run with two constants exchanged leaves it far behind."""
import numpy as np
import pytest

from cu2rec_amd import synth
from oracle import oracle as orc
from sgd_reference64 import State64, excess, sgd64

SETS = {
    "distinct": (0.01, 0.015, 0.03, 0.045, 0.08),
    "toy_golden": (0.05, 0.03, 0.07, 0.11, 0.19),
    "ref_train_cfg": (0.1, 0.2, 0.1, 0.1, 0.1),
    "strong_decay": (0.05, 0.02, 0.4, 0.05, 1.0),
    "a_zero": (0.5, 0.02, 2.0, 0.02, 2.0),
    "a_negative": (0.5, 0.02, 3.0, 0.02, 0.5),
}


def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("dot_order", [orc.DOT_SEQ, orc.DOT_TREE16])
def test_oracle_lies_inside_the_float64_references_rounding_bound(name, dot_order):
    hyper = SETS[name]
    iters = 2 if name.startswith("a_") else 4
    tr = synth.make_ratings(120, 40, 1500, min_degree=3, seed=5)[0]
    f = 20
    state = orc.init_model(tr.rows, tr.cols, f)
    st = State64(*state)
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, hyper, 42, 3, iters, dot_order=dot_order)
    sgd64(tr, st, tr.global_bias, hyper, 42, 3, iters)
    assert all(np.isfinite(a).all() for a in state)
    worst, dist = excess(state, st)
    assert worst <= 1.0, (name, worst, dist)  # measured: 0.05 .. 0.16 of the bound, at distances of 3e-8 .. 4e-7


def test_the_bound_separates_every_exchange_of_two_constants():
    """The oracle with the distinct set against the reference run with each pair of constants exchanged: outside the bound."""
    hyper = (0.05, 0.03, 0.07, 0.11, 0.19)
    tr = synth.make_ratings(120, 40, 1500, min_degree=3, seed=5)[0]
    f = 20
    state = orc.init_model(tr.rows, tr.cols, f)
    init = [a.copy() for a in state]
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, hyper, 42, 0, 4, dot_order=orc.DOT_TREE16)
    for i in range(1, 5):
        for j in range(i + 1, 5):
            swapped = list(hyper)
            swapped[i], swapped[j] = swapped[j], swapped[i]
            st = sgd64(tr, State64(*init), tr.global_bias, swapped, 42, 0, 4)
            worst, dist = excess(state, st)
            assert worst > 100.0, (i, j, worst, dist)
