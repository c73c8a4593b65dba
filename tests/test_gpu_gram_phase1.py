"""Phase 1 of the block-solve mode (-m gpu; cu2rec_amd/csrc/blocksolve_gram.hpp, bs_gram_kernel): the Gram contraction split over four
wavefronts (gram_split: wavefronts 0-2 the leading three quarters of the K range of one tile each, wavefront 3 the rest of all three,
the partial tiles added through LDS).

It re-associates nothing but float sums, so the bar is the mode's own (tests/test_gpu_blocksolve.py): every parameter within 2e-6 of
the sequential oracle."""
import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HYPER = (0.01, 0.02, 0.02, 0.02, 0.02)

# users, items, nnz, f, iters, rate, look-ahead blocks (0: the process default stays)
SHAPES = [
    (300, 120, 6000, 1, 5, 2.0, 0),       # one slot: wavefront 3's K range is empty, and so is lane half 1's
    (300, 120, 6000, 10, 70, 2.0, 0),     # three slots: wavefront 3 empty, lane half 1 one slot short; two schedule windows
    (3000, 40, 30000, 100, 6, 1.0, 0),    # three blocks a chain, the last partial; S0 = 13: the split 10 | 3 of the benchmark
    (2000, 300, 40000, 252, 3, 4.0, 0),   # 63 slots: S0 = 32, split 24 | 8
    (9000, 6, 40000, 116, 3, 1.0, 2),     # 29 slots (S0 = 15, split 12 | 3, both ranges end on an odd step), cross blocks
    (500, 50, 5000, 8, 10, 0.01, 0),      # every item hot, many one- and two-link blocks
]


@pytest.fixture
def settings():
    rate, la = api.blocksolve_min_rate(), api.blocksolve_lookahead_blocks()
    yield
    api.blocksolve_min_rate(rate)
    api.blocksolve_lookahead_blocks(la)


@pytest.mark.parametrize("users,items,nnz,f,iters,rate,la", SHAPES)
def test_phase1_matches_sequential_oracle(settings, users, items, nnz, f, iters, rate, la):
    api.blocksolve_min_rate(rate)
    if la:
        api.blocksolve_lookahead_blocks(la)
    tr, _ = synth.make_ratings(users, items, nnz, min_degree=3, seed=users + f)
    state = orc.init_model(tr.rows, tr.cols, f)
    orc.sgd_iterations(orc.CSR(tr.indptr, tr.indices, tr.data, tr.rows, tr.cols, tr.global_bias), *state, tr.global_bias, HYPER, 42, 0, iters,
                       dot_order=orc.DOT_TREE16)
    d_tr = cu.DeviceCSR(tr)  # (the schedule is created here: it reads the settings)
    assert d_tr.blocksolve_items() > 0
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    model.sgd(d_tr, HYPER, 42, 0, iters, mode="blocksolve")
    diffs = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)]
    print("max |model - oracle| per array:", diffs)
    assert max(diffs) <= 2e-6, diffs  # float rounding of re-associated sums; values are O(0.1 .. 1)
