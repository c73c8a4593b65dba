"""The raw-pointer ABI at caller-chosen row strides and base offsets (-m gpu).

include/cu2rec_amd.h: a factor matrix may have any row stride that is a multiple of 4 floats and at least n_factors, on any 16-byte
aligned base.  Everything else in the suite runs at ld = round4(f), ldq = round32(f) from the start of an allocation; here every mode
runs at the four layouts of tests/layout_checks.py (dense: no padding, Q rows sharing lines; crossed: ldp > ldq, ldq no multiple of
32; wide: a large stride; offset16: a base aligned to 16 bytes only) over lc.WIDTHS -- each f % 4, f % 32 == 0 and not, both sides of
the 252-factor block-solve limit, J = 1, 2, 3, 4, 5 and 8 float4 slots per lane -- on the set of tests/test_gpu_row_widths.py:
  * serial, ordered, ping-pong (cu2rec_sgd_update_pingpong, the current side ending in either pair), streaming Hogwild on a
    collision-free set and with the item side frozen, the resident Hogwild launch with and without the sample array (the eleven
    widths up to 256), one partial residency case (crossed only): the oracle's result bit for bit (TREE16 dot order, the kernels' own);
  * the loss pass on the initial and on a trained model: MAE, RMSE and every residual, bit for bit;
  * block-solve up to 252 factors within 2e-6 of the oracle AND bit for bit the default layout's result (its arithmetic depends on
    the number of float4 slots, not on the stride; two default-layout runs are compared first) and NOT the oracle's bits (the
    schedule the engines use does solve chains block-wise), in both phase-2 settings up to 116 factors; refused above 252 with
    nothing written;
  * one cu2rec_schedule used at ldq = 104, 260, 100 in turn (BlockSolve::begin re-allocates its item-row workspace);
  * a stride or a base the header forbids is CU2REC_EINVAL with the header's words, and nothing is written.
After every call the guards around P, Q and Q_target are still the sentinel and the padding columns still zero (lc.verify)."""
import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib
from oracle import oracle as orc

import blocksolve_checks as bc
import layout_checks as lc
from test_gpu_resident import FORCE, _collision_free_set, resident_policy
from test_gpu_row_widths import HYPER, ITERS, _as_orc, _own_item_set, _set

pytestmark = pytest.mark.gpu

WIDTHS = lc.WIDTHS
LAYOUT_IDS = [lay.name for lay in lc.LAYOUTS]
NAMES = ("P", "Q", "user_bias", "item_bias")
PLAIN, LOOKAHEAD = 0, 1  # cu2rec_blocksolve_lookahead_blocks, as tests/test_gpu_blocksolve_grid.py sets the two forms
BS_BOUND = 2e-6          # the bound of tests/test_gpu_row_widths.py for block-solve on this set
SEED = 42

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ratings(name, host):
    """One DeviceRatings (and so one schedule) per rating set for the whole module: engines of every stride share it."""
    from cu2rec_amd.engine import DeviceRatings
    return _cached(("ratings", name), lambda: DeviceRatings(host, "cuda"))


def _init(m, f):
    """The starting model (the library's own initialisation); shared, never written to."""
    return _cached(("init", m.rows, m.cols, f), lambda: orc.init_model(m.rows, m.cols, f))


def _engine(layout, m, f, targets=False):
    P, Q, ub, ib = _init(m, f)
    return lc.strided_engine(layout, m.rows, m.cols, f, m.global_bias, P, Q, ub, ib, targets=targets)


def _trained(name, m, f, iter0=0, iters=ITERS, update_items=True):
    def make():
        state = [a.copy() for a in _init(m, f)]
        orc.sgd_iterations(_as_orc(m), *state, m.global_bias, HYPER, SEED, iter0, iters, dot_order=orc.DOT_TREE16, update_items=update_items)
        return state
    return _cached(("trained", name, f, iter0, iters, update_items), make)


def _loss(name, m, state, f):
    return _cached(("loss", name, f), lambda: orc.loss(_as_orc(m), *state, m.global_bias, dot_order=orc.DOT_TREE16, want_errors=True))


def _assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, w, err_msg="%s: %s" % (what, name))


def _assert_loss(eng, d, want, what):
    got = eng.loss(d, want_errors=True)
    assert got["mae"] == want["mae"] and got["rmse"] == want["rmse"], (what, got["mae"], want["mae"], got["rmse"], want["rmse"])
    np.testing.assert_array_equal(got["errors"], want["errors"], err_msg=what + ": residuals")


layouts = pytest.mark.parametrize("layout", lc.LAYOUTS, ids=LAYOUT_IDS)
widths = pytest.mark.parametrize("f", WIDTHS)


# ------------------------------------------------------------------ the exact modes
@layouts
@widths
def test_serial_ordered_and_loss_bit_exact(f, layout):
    tr = _set()
    d = _ratings("tr", tr)
    want = _trained("tr", tr, f)
    eng = _engine(layout, tr, f)
    _assert_loss(eng, d, _loss("tr-init", tr, _init(tr, f), f), "initial model")
    _assert_equal(lc.verify(eng), _init(tr, f), "the loss pass wrote to the model")
    for mode in ("serial", "ordered"):
        eng = _engine(layout, tr, f)
        eng.sgd(d, HYPER, SEED, 0, ITERS, mode=mode)
        _assert_equal(lc.verify(eng), want, mode)
        _assert_loss(eng, d, _loss("tr-trained", tr, want, f), mode + ", trained model")
        lc.verify(eng)


@layouts
@widths
def test_pingpong_bit_exact_in_both_buffer_pairs(f, layout):
    tr = _set()
    d = _ratings("tr", tr)
    for iters in (ITERS, ITERS + 1):  # odd: the current item side ends in the target pair; even: in the first

        def make():
            P, Q, ub, ib = (a.copy() for a in _init(tr, f))
            Qt, ibt = Q.copy(), ib.copy()
            orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, HYPER, SEED, 0, iters, dot_order=orc.DOT_TREE16)
            return (P, Q, ub, ib), (Qt, ibt)
        want, want_other = _cached(("pingpong", f, iters), make)
        eng = _engine(layout, tr, f, targets=True)
        swapped = lc.pingpong(eng, d, HYPER, SEED, 0, iters)
        assert swapped == iters % 2
        P, Q, ub, ib = lc.verify(eng)
        Qt, ibt = eng.target
        current, other = ((P, Qt, ub, ibt), (Q, ib)) if swapped else ((P, Q, ub, ib), (Qt, ibt))
        _assert_equal(current, want, "ping-pong, %d iterations" % iters)
        # the other pair: the item side of one iteration earlier (the oracle's target buffers after its swap)
        np.testing.assert_array_equal(other[0], want_other[0], err_msg="ping-pong, %d iterations: the other Q" % iters)
        np.testing.assert_array_equal(other[1], want_other[1], err_msg="ping-pong, %d iterations: the other item_bias" % iters)


@layouts
@widths
def test_streaming_hogwild_bit_exact_where_no_update_races(f, layout):
    own, tr = _own_item_set(f), _set()
    with resident_policy(0):  # streaming launches only
        eng = _engine(layout, own, f)
        eng.sgd(_ratings(("own", f), own), HYPER, SEED, 0, ITERS, mode="hogwild")
        _assert_equal(lc.verify(eng), _trained(("own", f), own, f), "hogwild")
        eng = _engine(layout, tr, f)
        eng.sgd(_ratings("tr", tr), HYPER, SEED, 0, ITERS, mode="hogwild", update_items=False)
        _assert_equal(lc.verify(eng), _trained("tr", tr, f, update_items=False), "hogwild, item side frozen")


@pytest.mark.parametrize("with_pairs", [True, False], ids=["pairs", "csr"])
@layouts
@pytest.mark.parametrize("f", [f for f in WIDTHS if f <= 256])
def test_resident_hogwild_bit_exact(f, layout, with_pairs):
    own = _own_item_set(f)
    d = _ratings(("own", f), own)
    eng = _engine(layout, own, f)
    with resident_policy(FORCE):
        assert lib().cu2rec_hogwild_resident_plan(own.rows, f, ITERS, None, None) == 1
        if with_pairs:
            eng.sgd(d, HYPER, SEED, 0, ITERS, mode="hogwild")  # (the engine passes the sample array to a resident launch)
            assert d._pairs is not None
        else:
            from cu2rec_amd.engine import _stream_ptr
            api.sgd_update(d.indptr.data_ptr(), d.indices.data_ptr(), d.data.data_ptr(), own.rows, own.cols, eng.P.data_ptr(), eng.ld,
                           eng.Q.data_ptr(), eng.ldq, eng.user_bias.data_ptr(), eng.item_bias.data_ptr(), eng.global_bias, f, HYPER,
                           SEED, 0, ITERS, api.SGD_HOGWILD, True, 0, _stream_ptr(), None)
    _assert_equal(lc.verify(eng), _trained(("own", f), own, f), "resident hogwild")


def test_partial_residency_at_crossed_strides():
    """The shape of test_resident_partial_residency_bit_exact_with_distinct_constants: 82,000 users at f = 256, three rows of every
    group streamed from and to memory at stride ldp = 288 while the item rows sit at ldq = 260."""
    f, users, layout = 256, 82000, lc.BY_NAME["crossed"]
    assert lib().cu2rec_hogwild_resident_streamed_rows(users, f, 256) == 3
    assert (layout.ldp(f), layout.ldq(f)) == (288, 260)
    m = _collision_free_set(users, 2 * users + 64, 3, 5, 4, seed=9, empty_every=53)
    from cu2rec_amd.engine import DeviceRatings
    eng = _engine(layout, m, f)
    d = DeviceRatings(m, eng.device)
    with resident_policy(FORCE):
        assert lib().cu2rec_hogwild_resident_plan(users, f, 2, None, None) == 1
        eng.sgd(d, HYPER, SEED, 5, 2, mode="hogwild")
        eng.sgd(d, HYPER, SEED, 7, 2, mode="hogwild")
    _assert_equal(lc.verify(eng), _trained("partial", m, f, iter0=5, iters=4), "partial residency")


# ------------------------------------------------------------------ block-solve
@pytest.fixture
def settings():
    """Both settings are read when a schedule is created; whatever a test sets is taken back."""
    rate, la = api.blocksolve_min_rate(), api.blocksolve_lookahead_blocks()
    yield
    api.blocksolve_min_rate(rate)
    api.blocksolve_lookahead_blocks(la)


def _bs_ratings(la):
    """The set with a schedule created under min_rate 1.0 and the given look-ahead setting (call with the `settings` fixture)."""
    tr = _set()
    api.blocksolve_min_rate(1.0)
    api.blocksolve_lookahead_blocks(la)
    d = _ratings(("tr-blocksolve", la), tr)
    d.schedule()
    if ("hot", la) not in _CACHE:
        _CACHE[("hot", la)] = cu.DeviceCSR(tr).blocksolve_items()  # the same rule on the same set under the same settings
    assert _CACHE[("hot", la)] > 0
    return tr, d


def _bs_run(layout, tr, d, f):
    eng = _engine(layout, tr, f)
    eng.sgd(d, HYPER, SEED, 0, ITERS, mode="blocksolve")
    return lc.verify(eng)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _bs_default(tr, d, f, la):
    """The default layout's result of the case, run twice in this process: the two runs must agree bit for bit for the comparison of
    another layout with them to mean anything."""
    def make():
        first, second = _bs_run(lc.DEFAULT, tr, d, f), _bs_run(lc.DEFAULT, tr, d, f)
        assert _same_bits(first, second), "two default-layout block-solve runs differ (f=%d, look-ahead %d)" % (f, la)
        return first
    return _cached(("bs-default", f, la), make)


def _assert_within(got, want, what):
    diffs = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want)]
    print("%s: distance from the oracle %s" % (what, ", ".join("%s %.2e" % nd for nd in zip(NAMES, diffs))))
    assert all(np.isfinite(g).all() for g in got) and max(diffs) <= BS_BOUND, (what, diffs)


@layouts
@widths
def test_blocksolve_within_2e6_and_the_default_layouts_bits_or_refused(settings, f, layout):
    if f > 252:
        tr, d = _bs_ratings(PLAIN)
        eng = _engine(layout, tr, f)
        before = lc.snapshot(eng)
        with pytest.raises(cu.Cu2recError) as e:
            eng.sgd(d, HYPER, SEED, 0, ITERS, mode="blocksolve")
        assert e.value.status == -6  # CU2REC_EUNSUPPORTED
        lc.assert_unchanged(eng, before)
        lc.verify(eng)
        return
    want = _trained("tr", _set(), f)
    for la in (PLAIN, LOOKAHEAD) if f <= 116 else (PLAIN,):
        tr, d = _bs_ratings(la)
        what = "block-solve f=%d %s look-ahead %d" % (f, layout.name, la)
        base = _bs_default(tr, d, f, la)
        _assert_within(base, want, what + " (default layout)")
        # the schedule these engines run on has hot chains: the ordered walk alone would be the oracle bit for bit
        assert not _same_bits(base, want), what + ": the sequential oracle's bits, the block-solve kernels did not run"
        got = _bs_run(layout, tr, d, f)
        _assert_within(got, want, what)
        assert _same_bits(got, base), what + ": not the default layout's bits"


@pytest.mark.parametrize("la", [PLAIN, LOOKAHEAD], ids=["plain", "lookahead"])
def test_one_schedule_at_three_item_strides(settings, la):
    """crossed, wide, dense on ONE api.Schedule: ldq = 104, 260, 100, so BlockSolve::begin re-allocates qstart before the second and
    the third call.  Same starting model, same iterations: the same bits, within the bound."""
    f = 100
    tr, d = _bs_ratings(la)
    want = _trained("tr", tr, f)
    base = _bs_default(tr, d, f, la)
    strides, results = [], []
    for name in ("crossed", "wide", "dense"):
        layout = lc.BY_NAME[name]
        strides.append(layout.ldq(f))
        results.append(_bs_run(layout, tr, d, f))
    assert strides == [104, 260, 100]
    for name, got in zip(("crossed", "wide", "dense"), results):
        _assert_within(got, want, "one schedule, %s" % name)
        assert _same_bits(got, results[0]) and _same_bits(got, base), name


def _lengths_run(layout, f, la):
    """Block-solve on the length set from bc's starting model, on the one DeviceRatings whose schedule was created under `la`."""
    from cu2rec_amd.engine import DeviceRatings
    tr = bc.length_set()
    start, _ = bc.references("lengths", tr, f)

    def make():
        api.blocksolve_min_rate(0.5)
        api.blocksolve_lookahead_blocks(la)
        d = DeviceRatings(tr, "cuda")
        d.schedule()
        return d
    d = _cached(("lengths", la), make)
    eng = lc.strided_engine(layout, tr.rows, tr.cols, f, tr.global_bias, *start)
    eng.sgd(d, bc.HYPER, bc.SEED, 0, bc.ITERS, mode="blocksolve")
    return lc.verify(eng)


def _lengths_default(f, la):
    def make():
        first, second = _lengths_run(lc.DEFAULT, f, la), _lengths_run(lc.DEFAULT, f, la)
        assert _same_bits(first, second), "two default-layout runs differ"
        return first
    return _cached(("lengths-default", f, la), make)


@pytest.mark.parametrize("la", [PLAIN, LOOKAHEAD], ids=["plain", "lookahead"])
@layouts
@pytest.mark.parametrize("f", [5, 36, 100])
def test_blocksolve_long_chains_at_every_layout(settings, f, layout, la):
    """On the set above no chain reaches two blocks, so the look-ahead setting selects nothing there.  The length set of
    tests/blocksolve_checks.py has chains of exactly 1 .. 769 links (thirteen blocks): on it the look-ahead form runs, and the plain
    form's long_chain path.  Held to that helper's bound against the float64 walk, and to the default layout's bits."""
    tr = bc.length_set()
    _, (ref,) = bc.references("lengths", tr, f)
    base = _lengths_default(f, la)
    got = _lengths_run(layout, f, la)
    bc.assert_within(got, ref, tr, "length set, f=%d, %s, look-ahead %d" % (f, layout.name, la))
    assert not _same_bits(got, ref.oracle), "block-solve equals the sequential oracle bit for bit: its kernels did not run"
    assert _same_bits(got, base), "not the default layout's bits"
    if la == LOOKAHEAD:
        assert not _same_bits(got, _lengths_default(f, PLAIN)), "the look-ahead form did not run: the plain form's bits"


# ------------------------------------------------------------------ refusals
BAD_STRIDE = "row stride must be a multiple of 4 floats and >= n_factors"
BAD_BASE = "factor matrix must be 16-byte aligned"


def _calls(eng, d, sched, **over):
    """The four entry points on the engine's buffers, with some arguments replaced -> {name: thunk}."""
    from cu2rec_amd.engine import _stream_ptr
    a = dict(P=eng.P.data_ptr(), ldp=eng.ld, Q=eng.Q.data_ptr(), ldq=eng.ldq, Q_target=eng.Q_target.data_ptr())
    a.update(over)
    csr = (d.indptr.data_ptr(), d.indices.data_ptr(), d.data.data_ptr())
    ub, ib, gb, f = eng.user_bias.data_ptr(), eng.item_bias.data_ptr(), eng.global_bias, eng.f
    return {
        "cu2rec_sgd_update": lambda: api.sgd_update(*csr, d.rows, eng.cols, a["P"], a["ldp"], a["Q"], a["ldq"], ub, ib, gb, f, HYPER, SEED, 0,
                                                    ITERS, api.SGD_HOGWILD, True, 0, _stream_ptr(), None),
        "cu2rec_sgd_update_pingpong": lambda: lc.pingpong(eng, d, HYPER, SEED, 0, ITERS, **a),
        "cu2rec_sgd_update_ordered": lambda: api.sgd_update_ordered(sched, *csr, d.rows, eng.cols, a["P"], a["ldp"], a["Q"], a["ldq"], ub, ib,
                                                                    gb, f, HYPER, SEED, 0, ITERS, True, 0, _stream_ptr()),
        "cu2rec_loss": lambda: api.loss_raw(*csr, d.rows, d.nnz, a["P"], a["ldp"], a["Q"], a["ldq"], ub, ib, gb, f,
                                            eng.workspace.data_ptr(), None, _stream_ptr()),
    }


@pytest.mark.parametrize("f", [1, 5, 8, 36, 100, 252, 512])
def test_forbidden_strides_and_bases_are_refused_and_nothing_is_written(f):
    """Real buffers at the wide layout's strides (more than twice any stride passed below) inside their guards: even a call that
    were wrongly accepted would stay in memory the test owns."""
    tr = _set()
    d = _ratings("tr", tr)
    eng = _engine(lc.BY_NAME["wide"], tr, f, targets=True)
    before = lc.snapshot(eng)
    cases = [("P stride", dict(ldp=lc.round4(f) + 2), "P: " + BAD_STRIDE, None),
             ("P base", dict(P=eng.P.data_ptr() + 4), "P: " + BAD_BASE, None),
             ("Q base", dict(Q=eng.Q.data_ptr() + 4), "Q: " + BAD_BASE, None),
             ("Q_target base", dict(Q_target=eng.Q_target.data_ptr() + 4), "Q_target: " + BAD_BASE, "cu2rec_sgd_update_pingpong")]
    if f >= 8:
        cases.append(("Q stride", dict(ldq=f - 4), "Q: " + BAD_STRIDE, None))
    for what, over, message, only in cases:
        for name, call in _calls(eng, d, d.schedule(), **over).items():
            if only is not None and name != only:
                continue
            with pytest.raises(cu.Cu2recError) as e:
                call()
            assert e.value.status == -1 and message in str(e.value), (name, what, str(e.value))  # CU2REC_EINVAL
            lc.assert_unchanged(eng, before)
    for name, call in _calls(eng, d, d.schedule()).items():  # and the same calls with nothing replaced are accepted
        call()
    lc.verify(eng)
