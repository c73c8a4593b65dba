"""Block-solve at every row width x pinned chain lengths, in both phase-2 forms (-m gpu).

tests/blocksolve_checks.py holds the cases: the 63 widths nslots = 1 .. 63 (f = 4 nslots - nslots mod 4: all seven phase-2
instantiations, all five look-ahead ones, one to four phase-3 wavefronts), on 19 items whose chains have EXACTLY 1, 2, 31, 32, 33, 63,
64, 65, 127, 128, 129, 255, 256, 257, 320, 511, 512, 513 and 769 links in every iteration -- both halves of a block, full blocks and
one link more or fewer, the 4 / 5-block long_chain threshold, n_intervals of 8 and of 12, 13 blocks -- from a starting model of O(0.5)
entries on which a lost float4 slot or a lost link moves the result by at least 2.5e-3 (tests/test_blocksolve_checks_cpu.py).  Every
parameter is held to tol = max(2e-6, 4 d_orc) of the float64 walk (tests/sgd_reference64.py), d_orc being the float32 oracle's own
distance from it (tol <= 4.2e-6 here, capped at 1e-5); a failure names the chain length and the array.
  * the plain form at every width, P's and Q's padding floats still zero behind it (phase 3 computes the columns f .. 4 nslots);
  * the look-ahead form at every width it is compiled for (nslots <= 29), and not the plain form's bits;
  * above 29 slots the look-ahead setting changes nothing, bit for bit;
  * a call with the item side frozen, then a resumed call (iter0 = 2) on the same DeviceCSR and model, one width per phase-2 bucket;
  * hot chains whose length changes from iteration to iteration: empty in some, one block in some and two in others.
Every case prints its distances (kernel, oracle, bound); -s shows them."""
import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import check, lib

import blocksolve_checks as bc
from test_gpu_row_widths import _check_padding

pytestmark = pytest.mark.gpu

PLAIN, LOOKAHEAD = 0, 1  # cu2rec_blocksolve_lookahead_blocks: 0 = off; 1 = every rank expected to fill one block


@pytest.fixture
def settings():
    """Both settings are read when a DeviceCSR's schedule is created; whatever a test sets is taken back."""
    rate, la = api.blocksolve_min_rate(), api.blocksolve_lookahead_blocks()
    yield
    api.blocksolve_min_rate(rate)
    api.blocksolve_lookahead_blocks(la)


def lookahead_items(csr, la_min, min_rate):
    """blocksolve.hip, BlockSolve::BlockSolve, and blocksolve_device.hpp, chain_is_lookahead: the leading ranks (rate descending) with
    rate >= 64 la_min are look-ahead ranks; such a chain runs the look-ahead form in an iteration in which it has at least two blocks
    and its blocks -- the first of the block table, in rank order -- end within la_cap.  -> (the ranks' items, la_cap)"""
    rate = api.item_update_rates(csr)
    order = np.argsort(-rate, kind="stable")
    n_hot = int((rate >= min_rate).sum())
    n_active = int((np.diff(csr.indptr) > 0).sum())
    max_blocks = n_active // 64 + n_hot + 1
    ranks = [int(j) for j in order[:n_hot] if rate[j] >= 64.0 * la_min]
    la_blocks = sum(np.ceil(rate[j] / 64.0) + 1.0 for j in ranks)
    return ranks, min(max_blocks, int(la_blocks * 1.25) + 4 * len(ranks) + 8)


def _run(csr, f, start, la, calls=bc.LENGTH_CALLS, rate=0.5, hot=len(bc.LENGTHS)):
    """The calls on one DeviceCSR and one model from `start` -> (the model, its downloaded state after every call)."""
    api.blocksolve_min_rate(rate)
    api.blocksolve_lookahead_blocks(la)
    d = cu.DeviceCSR(csr)
    assert d.blocksolve_items() == hot
    model = bc.model_from(csr, f, start)
    out = []
    for iter0, n, update_items in calls:
        model.sgd(d, bc.HYPER, bc.SEED, iter0, n, mode="blocksolve", update_items=update_items)
        check(lib().cu2rec_check_faults())
        out.append(model.download())
    return model, out


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _report(form, nslots, worst, ref):
    print("grid %-9s nslots %2d f %3d SW %2d: kernel %.3e oracle %.3e bound %.3e" % (form, nslots, bc.width(nslots), bc.sw_bucket(nslots),
                                                                                  worst, ref.d_orc, ref.tol))


@pytest.mark.parametrize("nslots", bc.NSLOTS)
def test_plain_form_every_width_every_length(settings, nslots):
    tr, f = bc.length_set(), bc.width(nslots)
    start, (ref,) = bc.references("lengths", tr, f)
    model, (got,) = _run(tr, f, start, PLAIN)
    _report("plain", nslots, bc.assert_within(got, ref, tr, "plain form, f=%d (SW %d)" % (f, bc.sw_bucket(nslots))), ref)
    assert not _same_bits(got, ref.oracle), "block-solve equals the sequential oracle bit for bit: its kernels did not run"
    _check_padding(model, f)


@pytest.mark.parametrize("nslots", [n for n in bc.NSLOTS if n <= bc.LA_MAX_SLOTS])
def test_lookahead_form_every_width_every_length(settings, nslots):
    tr, f = bc.length_set(), bc.width(nslots)
    # the rule: every item with rate >= 64 is a look-ahead rank, and those of 65 links and more -- two blocks -- take the form
    ranks, la_cap = lookahead_items(tr, LOOKAHEAD, 0.5)
    assert sorted(bc.LENGTHS[j] for j in ranks) == [n for n in bc.LENGTHS if n >= 64]
    assert sum(-(-bc.LENGTHS[j] // 64) for j in ranks) <= la_cap
    assert sum(1 for j in ranks if bc.LENGTHS[j] > 64) == 12
    start, (ref,) = bc.references("lengths", tr, f)
    model, (got,) = _run(tr, f, start, LOOKAHEAD)
    _report("lookahead", nslots, bc.assert_within(got, ref, tr, "look-ahead form, f=%d (NSM %d)" % (f, bc.nsm_bucket(nslots))), ref)
    _check_padding(model, f)
    _, (plain,) = _run(tr, f, start, PLAIN)
    assert not _same_bits(got, plain), "the look-ahead form did not run: the plain form's bits"


@pytest.mark.parametrize("nslots", [30, 32, 33, 63])
def test_lookahead_setting_is_ignored_above_29_slots(settings, nslots):
    """la_supported (blocksolve_lookahead.hpp; read in BlockSolve::begin) takes rows of at most 29 slots, and bs_solve_kernel compiles
    the form for SW <= 8 only."""
    assert nslots > bc.LA_MAX_SLOTS and {bc.sw_bucket(n) for n in (30, 32, 33, 63)} == {8, 12, 16}
    tr, f = bc.length_set(), bc.width(nslots)
    start, (ref,) = bc.references("lengths", tr, f)
    _, (plain,) = _run(tr, f, start, PLAIN)
    model, (got,) = _run(tr, f, start, LOOKAHEAD)
    assert _same_bits(got, plain)
    bc.assert_within(got, ref, tr, "look-ahead setting at f=%d" % f)
    _check_padding(model, f)


@pytest.mark.parametrize("nslots", bc.ONE_PER_BUCKET)
def test_frozen_items_and_resumed_call(settings, nslots):
    """update_items = False for two iterations (no two updates share a written row), then two more
    iterations from iter0 = 2 with the item side moving, on the same DeviceCSR and model -- the schedule's window is entered at an
    offset.  The float64 walk and the oracle continue the same way; the resumed call's bound comes from the oracle's distance THERE."""
    tr, f = bc.length_set(), bc.width(nslots)
    start, refs = bc.references("lengths", tr, f, calls=bc.FROZEN_THEN_RESUMED)
    for la in (PLAIN, LOOKAHEAD) if nslots <= bc.LA_MAX_SLOTS else (PLAIN,):
        what = "%s form, f=%d" % ("look-ahead" if la else "plain", f)
        model, (frozen, resumed) = _run(tr, f, start, la, calls=bc.FROZEN_THEN_RESUMED)
        assert _same_bits(frozen[1::2], start[1::2]), "the frozen item side moved (%s)" % what
        bc.assert_within(frozen, refs[0], tr, what + ", item side frozen")
        worst = bc.assert_within(resumed, refs[1], tr, what + ", resumed at iteration 2")
        _report("resumed" + ("/la" if la else ""), nslots, worst, refs[1])
        _check_padding(model, f)


@pytest.mark.parametrize("la", [PLAIN, LOOKAHEAD], ids=["plain", "lookahead"])
@pytest.mark.parametrize("nslots", [1, 17, 33])
def test_hot_chain_that_some_iterations_leave_empty(settings, nslots, la):
    """The length set plus items rated only by users of two ratings (bc.varying_set): hot by their rate, their chains Binomial.  Over the
    six iterations one of them is empty in some, and the one of 132 raters -- a look-ahead rank -- has one block in some iterations
    and two in others, so the form it runs changes from iteration to iteration.  The raters' partner items (rate 0.5 each, below
    the threshold of 1.0 used here) are walked on the side stream beside the chains."""
    va, hot = bc.varying_set()
    f = bc.width(nslots)
    chains = np.array([bc.realised_chains(va, bc.SEED, it) for it in range(bc.VARYING_ITERS)])
    assert (chains[:, hot] == 0).any() and any(chains[:, j].min() <= 64 < chains[:, j].max() for j in hot), chains[:, hot]
    ranks, la_cap = lookahead_items(va, LOOKAHEAD, bc.VARYING_MIN_RATE)
    assert hot[-1] in ranks and int((-(-chains[:, ranks].max(axis=0) // 64)).sum()) <= la_cap
    calls = ((0, bc.VARYING_ITERS, True),)
    start, (ref,) = bc.references("varying", va, f, calls=calls)
    model, (got,) = _run(va, f, start, la, calls=calls, rate=bc.VARYING_MIN_RATE, hot=len(bc.LENGTHS) + len(hot))
    worst = bc.assert_within(got, ref, va, "%s form, f=%d, varying chains" % ("look-ahead" if la else "plain", f))
    _report("varying" + ("/la" if la else ""), nslots, worst, ref)
    _check_padding(model, f)
