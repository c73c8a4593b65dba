"""The views a cu2rec_csr keeps of itself (csrc/csr_views.hpp: item-major, row-sorted, row of every entry) are shared by ALS, iALS,
logistic MF, BPR and ItemKNN: whichever consumer asks first builds a view, and every other one then reads it.  Every consumer must
give the bits it gives on a fresh upload in every order of first use, a CSR with repeated columns must stay refused by ItemKNN and
accepted by BPR whoever sorted its rows, and the shared sort helpers are judged at the key widths and the empty shapes where they
take another path.  Every expected value is an existing float64 reference's (bpr_reference64, knn_reference64) or a fresh upload's."""
import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api

import bpr_checks
import bpr_reference64 as bpr_ref
import knn_checks
from als_checks import HYPER as ALS_HYPER, als, model_from, random_state, same_bits, same_state

pytestmark = pytest.mark.gpu

HYPER = (0.05, 0.6, 0.9, 0.25, 0.4)
SEED, SWEEP = bpr_checks.GRADIENT_SEED, bpr_checks.GRADIENT_SWEEP


# ---- 1: the order of first use -------------------------------------------------------------------------------------------------
def _consumers(csr):
    """name -> call(DeviceCSR) -> bytes, each from the same model state: the six consumers of the shared views."""
    state = random_state(csr.rows, csr.cols, 8, 31)

    def trained(step):
        def call(d):
            m = model_from(state, 3.0)
            extra = step(m, d)
            out = [a.tobytes() for a in m.download()] + [a.tobytes() for a in m.lmf_state()] + list(extra or [])
            m.close()
            return out
        return call

    def knn(d):
        model = cu.ItemKNN(d, "cosine", 10)
        out = [a.tobytes() for a in model.neighbors()] + [a.tobytes() for a in model.recommend(d, d, 5)]
        model.close()
        return out

    return {"als-items": trained(lambda m, d: m.als(d, HYPER, "items")),
            "ials": trained(lambda m, d: m.ials(d, HYPER, 2.0, "both")),
            "lmf-items": trained(lambda m, d: m.lmf(d, HYPER, 1.0, "items")),
            "bpr": trained(lambda m, d: [np.int64(m.bpr(d, HYPER, SEED, SWEEP, "both")).tobytes(), d.bpr_negatives(SEED, SWEEP + 1).tobytes()]),
            "knn-weights": lambda d: [d.knn_weights("bm25").tobytes()],
            "knn": knn}


def test_every_consumer_gives_its_fresh_bits_whichever_consumer_used_the_csr_first():
    """Six sequences on the 13 x 65 table of knn_checks, each from a fresh upload: one consumer first, then all the others.  BPR
    before ItemKNN builds the row-sorted view without positions and values and ItemKNN completes it; ItemKNN before BPR builds
    all of it; ALS plans a side whose view another consumer built, and the others read a view ALS built."""
    csr = knn_checks.cases()["65-full"].train
    consumers = _consumers(csr)
    fresh = {name: call(cu.DeviceCSR(csr)) for name, call in consumers.items()}
    for first in consumers:
        d = cu.DeviceCSR(csr)
        for name in [first] + [n for n in consumers if n != first]:
            assert consumers[name](d) == fresh[name], (first, name)
        d.close()


# ---- 2: repeated columns across the shared row-sorted view ---------------------------------------------------------------------
def _bpr_calls(d, csr):
    state = random_state(csr.rows, csr.cols, 8, 32)
    out = [d.bpr_negatives(SEED, SWEEP).tobytes()]
    for side in ("users", "items"):
        m = model_from(state, 0.0)
        out += [a.tobytes() for a in m.bpr_gradient(d, HYPER, SEED, SWEEP, side)]
        m.close()
    return out


def _knn_refusal(d):
    with pytest.raises(cu.Cu2recError) as err:
        cu.ItemKNN(d, "count", 5)
    assert err.value.status == -1 and "twice" in str(err.value)
    return str(err.value)


def test_a_csr_with_repeated_columns_is_refused_by_knn_and_served_by_bpr_in_either_order():
    """bpr_checks' 33 x 40 set: unsorted rows, one of which stores a quarter of its columns twice."""
    csr = bpr_checks.negative_sets()["33x40"]
    fresh_bpr, fresh_refusal = _bpr_calls(cu.DeviceCSR(csr), csr), _knn_refusal(cu.DeviceCSR(csr))
    d = cu.DeviceCSR(csr)  # BPR sorts the rows, ItemKNN reads what it sorted
    assert _bpr_calls(d, csr) == fresh_bpr
    assert _knn_refusal(d) == fresh_refusal
    d = cu.DeviceCSR(csr)  # ItemKNN sorts the rows and refuses, BPR reads what it sorted
    assert _knn_refusal(d) == fresh_refusal
    assert _bpr_calls(d, csr) == fresh_bpr
    d = cu.DeviceCSR(csr)  # both ALS plans first
    model_from(random_state(csr.rows, csr.cols, 8, 33), 0.0).als(d, HYPER, "both")
    assert _knn_refusal(d) == fresh_refusal
    assert _bpr_calls(d, csr) == fresh_bpr


# ---- 3: key widths and empty shapes of the shared sort helpers -------------------------------------------------------------------
def _edge_csr(per_row, cols):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in per_row])])
    idx = np.concatenate([np.asarray(r, np.int32) for r in per_row] + [np.zeros(0, np.int32)])
    data = (1 + (np.arange(len(idx)) * 7) % 10) / 2.0  # half stars
    return api.HostCSR(indptr, idx, data.astype(np.float32), len(per_row), cols, 0.0)


def _edge_sets():
    """A dozen entries in 3 to 6 unsorted rows.  cols 1 and 2: every column, with repeats.  cols 255, 256, 257 (the regrouping key
    `cols` needs a ninth bit exactly at 256; the columns' own keys at 257): columns 0 and cols - 1 stored, cols - 2 and most of
    the rest named by nobody.  One set ends in two empty rows.  The last one is larger: a row that stores all 256 columns, so that
    its entries go without a triple and the key `cols` itself, the one that needs the ninth bit, is sorted."""
    out = {"1": _edge_csr([[0, 0, 0], [0], [], [0, 0, 0, 0], [0, 0], [0, 0]], 1),
           "2": _edge_csr([[1, 0, 1, 0], [0], [1, 1, 0], [0, 1, 0, 1]], 2)}
    for cols in (255, 256, 257):
        top = cols - 1
        out[str(cols)] = _edge_csr([[top, 0, 128, 3], [], [127, top, 0], [0], [64, top, 129, 128]], cols)
    out["empty-tail"] = _edge_csr([[5, 0, 6], [6, 2, 0, 1, 5], [0, 6, 3, 1], [], []], 7)
    out["256-full-row"] = _edge_csr([[255, 0, 7], np.random.default_rng(5).permutation(256), [], [128, 255]], 256)
    return out


@pytest.mark.parametrize("name", ["1", "2", "255", "256", "257", "empty-tail", "256-full-row"])
def test_views_at_the_key_widths_and_with_empty_rows(name):
    """The negatives exactly (the row-sorted view and the row of every entry), the item gradient within its bound (the regrouping: an
    unnamed item is an empty group), the count and cosine weights as test_gpu_knn.py judges them (the item-major view and its
    positions)."""
    csr = _edge_sets()[name]
    assert 3 <= csr.rows <= 6
    if name in ("255", "256", "257"):
        assert csr.nnz == 12 and {0, csr.cols - 1} <= set(csr.indices.tolist()) and csr.cols - 2 not in csr.indices
    d = cu.DeviceCSR(csr)
    for seed in bpr_checks.SEEDS:
        for sweep in bpr_checks.SWEEPS:
            assert np.array_equal(d.bpr_negatives(seed, sweep), bpr_ref.negatives(csr, seed, sweep)), (seed, sweep)
    case = bpr_checks.Case(name, csr, "items", 5, 40)
    state, neg = case.state(), case.negatives()
    assert name != "256-full-row" or (neg[3:259] < 0).all()
    got = model_from(state, 0.0).bpr_gradient(d, case.hyper, SEED, SWEEP, "items")
    g, gb = bpr_ref.gradient(csr, state, case.hyper, neg, "items")
    b, bb = bpr_ref.bound(csr, state, case.hyper, neg, "items")
    assert got[0].shape == g.shape and got[1].shape == gb.shape
    ratio = max(bpr_ref.ratio(got[0], g, b), bpr_ref.ratio(got[1], gb, bb))
    print("%s: worst gradient value at %.3g of the bound, %d triples" % (name, ratio, (neg >= 0).sum()))
    assert ratio <= 1.0
    assert np.array_equal(d.knn_weights("count"), csr.data)
    ratio = knn_checks.weight_ratio(csr, "cosine", d.knn_weights("cosine"))
    print("%s: cosine weights at %.3f of 4 x %.3g" % (name, ratio, knn_checks.WEIGHT_DISTANCE))
    assert ratio <= 1.0


@pytest.mark.parametrize("cols", [0, 7])
def test_views_of_a_csr_without_entries(cols):
    """Every call returns; what it returns is what tests/test_gpu_bpr.py::test_problems_without_triples and
    tests/test_gpu_als_edges.py::test_no_ratings_changes_nothing expect of an empty problem: no negatives, the item gradient -reg x,
    no weights, and an ALS item half-step that solves nothing and leaves every bit of the model."""
    csr = api.HostCSR(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, cols, 0.0)
    d = cu.DeviceCSR(csr)
    assert d.bpr_negatives(SEED, SWEEP).shape == (0,)
    state = random_state(6, 8, 5, 41)
    model = model_from(state, 0.0)
    g, gb = model.bpr_gradient(d, HYPER, SEED, SWEEP, "items")
    assert g.shape == (cols, 5) and gb.shape == (cols,)
    assert same_bits(g, -(np.float32(HYPER[2]) * state[1][:cols])) and same_bits(gb, -(np.float32(HYPER[4]) * state[3][:cols]))
    for weighting in ("count", "cosine"):
        assert d.knn_weights(weighting).shape == (0,)
    for _ in range(2):
        assert als(model, d, ALS_HYPER, "items") == (0, 0)
    assert same_state(model.download(), state)
