"""The raw-pointer ABI on the caller's own streams (-m gpu).

`stream` is the caller's hipStream_t and calls are asynchronous on it (include/cu2rec_amd.h); cu2rec_amd/engine.py passes torch's
current stream, which everywhere else in the suite is the null stream -- where the library's guards BETWEEN streams are no-ops.
Here every call is made on torch.cuda.Stream()s, which are non-blocking:
  * every mode (ping-pong through its raw entry point), then the loss, on one such stream with no host synchronisation in between:
    the oracle's model and loss;
  * the CSR arrays and the model copied in from pinned memory on the stream just ahead of the call, over valid stale contents
    (same indptr, permuted indices and ratings, another model): the schedule stream, which reads the CSR arrays, waits for
    "whatever the caller queued on `stream` so far" (ordered.hip, ev_consumed[1]) -- a missing wait computes a wrong model from
    in-range data, never reads out of range.  In block-solve mode a warm-up call on the same schedule at the same ldq comes first:
    BlockSolve::begin synchronises the caller's stream on a schedule's first call (and when ldq changes), which would drain the
    copies on the host before any guard is armed.  Behind the warm-up the ev_consumed[1] wait is covered in this mode too; the side
    stream's own wait (blocksolve.hip, ev_call) is EXECUTED here, not covered: everything on the side stream is also gated behind
    phase 1 of its iteration on `stream` (bs_gate_kernel / ev_gram), so taking ev_call alone away would not change a result;
  * one cu2rec_schedule, two models, two streams, no ordering by the caller: a call on another stream than the schedule's last one
    starts behind that call (ordered.hip, last_stream != stream), in ordered and in block-solve mode;
  * resident Hogwild launches from two streams back to back: "never two at once" (resident.hip);
  * cu2rec_sgd_update_pingpong with swap_last = 0, then cu2rec_loss, on one stream: the loss before the swap.
The buffers are the default layout (ld = round4(f), ldq = round32(f)) inside the guards of tests/layout_checks.py."""
import numpy as np
import pytest
import torch

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib
from cu2rec_amd.engine import DeviceRatings, _stream_ptr
from oracle import oracle as orc

import layout_checks as lc
from test_gpu_layouts import _assert_equal, _assert_within, _same_bits
from test_gpu_resident import FORCE, resident_policy
from test_gpu_row_widths import HYPER, ITERS, _as_orc, _own_item_set, _set

pytestmark = pytest.mark.gpu

WIDTHS = [5, 100, 252]
SEED = 42
widths = pytest.mark.parametrize("f", WIDTHS)


@pytest.fixture
def min_rate():
    prev = api.blocksolve_min_rate()
    api.blocksolve_min_rate(1.0)  # read when a schedule is created: every DeviceRatings below has hot chains
    yield
    api.blocksolve_min_rate(prev)


def _model(m, f, seed=None):
    """seed None: the library's own initialisation; otherwise another model of the same scale."""
    if seed is None:
        return orc.init_model(m.rows, m.cols, f)
    rng = np.random.RandomState(seed)
    return tuple((rng.randn(*shape) / f).astype(np.float32) for shape in ((m.rows, f), (m.cols, f), (m.rows,), (m.cols,)))


def _engine(m, f, state, targets=False):
    return lc.strided_engine(lc.DEFAULT, m.rows, m.cols, f, m.global_bias, *state, targets=targets)


def _oracle(m, state, iter0, iters, update_items=True):
    out = [a.copy() for a in state]
    orc.sgd_iterations(_as_orc(m), *out, m.global_bias, HYPER, SEED, iter0, iters, dot_order=orc.DOT_TREE16, update_items=update_items)
    return out


def _oracle_loss(m, state):
    return orc.loss(_as_orc(m), *state, m.global_bias, dot_order=orc.DOT_TREE16)


def _ratings(m):
    d = DeviceRatings(m, "cuda")
    d.schedule()
    d.sample_pairs()
    torch.cuda.synchronize()
    return d


def _loss_on_current_pair(eng, d, swapped):
    """cu2rec_loss on torch's current stream, reading the item side from the pair *swapped names."""
    Q, ib = (eng.Q_target, eng.item_bias_target) if swapped else (eng.Q, eng.item_bias)
    return api.loss_raw(d.indptr.data_ptr(), d.indices.data_ptr(), d.data.data_ptr(), d.rows, d.nnz, eng.P.data_ptr(), eng.ld, Q.data_ptr(),
                        eng.ldq, eng.user_bias.data_ptr(), ib.data_ptr(), eng.global_bias, eng.f, eng.workspace.data_ptr(), None, _stream_ptr())


# ------------------------------------------------------------------ every mode on a stream of the caller's
@widths
def test_every_mode_then_the_loss_on_one_stream(min_rate, f):
    tr, own = _set(), _own_item_set(f)
    d_tr, d_own = _ratings(tr), _ratings(own)
    assert cu.DeviceCSR(tr).blocksolve_items() > 0
    init_tr, init_own = _model(tr, f), _model(own, f)
    want_tr, want_own = _oracle(tr, init_tr, 0, ITERS), _oracle(own, init_own, 0, ITERS)
    s1 = torch.cuda.Stream()
    null_bs = _engine(tr, f, init_tr)  # block-solve on the null stream, for the bits
    null_bs.sgd(d_tr, HYPER, SEED, 0, ITERS, mode="blocksolve")
    null_bs = lc.verify(null_bs)
    for mode, m, d, init, want, policy in (("serial", tr, d_tr, init_tr, want_tr, 1), ("ordered", tr, d_tr, init_tr, want_tr, 1),
                                           ("blocksolve", tr, d_tr, init_tr, want_tr, 1), ("hogwild", own, d_own, init_own, want_own, 0),
                                           ("resident", own, d_own, init_own, want_own, FORCE)):
        eng = _engine(m, f, init)
        with resident_policy(policy):
            if mode == "resident":
                assert lib().cu2rec_hogwild_resident_plan(m.rows, f, ITERS, None, None) == 1
            with torch.cuda.stream(s1):
                eng.sgd(d, HYPER, SEED, 0, ITERS, mode="hogwild" if mode == "resident" else mode)
                loss = eng.loss(d)  # no host synchronisation since the SGD call
        got = lc.verify(eng)
        if mode == "blocksolve":
            _assert_within(got, want, "block-solve on a stream, f=%d" % f)
            assert _same_bits(got, null_bs), "block-solve on a stream: not the null stream's bits"
            want_loss = _oracle_loss(m, got)
        else:
            _assert_equal(got, want, mode + " on a stream")
            want_loss = _oracle_loss(m, want)
        assert loss["mae"] == want_loss["mae"] and loss["rmse"] == want_loss["rmse"], (mode, loss, want_loss)
    # ping-pong: the raw entry point on the stream
    for iters in (ITERS, ITERS + 1):
        P, Q, ub, ib = (a.copy() for a in init_tr)
        Qt, ibt = Q.copy(), ib.copy()
        orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, HYPER, SEED, 0, iters, dot_order=orc.DOT_TREE16)
        eng = _engine(tr, f, init_tr, targets=True)
        with torch.cuda.stream(s1):
            swapped = lc.pingpong(eng, d_tr, HYPER, SEED, 0, iters)
            assert swapped == iters % 2
            loss = _loss_on_current_pair(eng, d_tr, swapped)  # no host synchronisation since the SGD call
        gP, gQ, gub, gib = lc.verify(eng)
        gQt, gibt = eng.target
        _assert_equal((gP, gQt, gub, gibt) if swapped else (gP, gQ, gub, gib), (P, Q, ub, ib), "ping-pong on a stream, %d iterations" % iters)
        want_loss = _oracle_loss(tr, (P, Q, ub, ib))
        assert loss["mae"] == want_loss["mae"] and loss["rmse"] == want_loss["rmse"], ("ping-pong", iters, loss, want_loss)


@widths
def test_pingpong_without_the_last_swap_then_the_loss_on_one_stream(f):
    """swap_last = 0: the loss right behind the call sees this iteration's P and the item side the iteration READ
    (training.cu:121 runs before the swap at :164), as tests/test_gpu_pingpong.py checks through cu2rec_train on the null stream."""
    tr = _set()
    d = _ratings(tr)
    init = _model(tr, f)
    iters = ITERS + 1  # three swaps: the side the loss must read is in the target pair
    P, Q, ub, ib = (a.copy() for a in init)
    Qt, ibt = Q.copy(), ib.copy()
    orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, HYPER, SEED, 0, iters, dot_order=orc.DOT_TREE16,
                                swap_last=False)
    want = _oracle_loss(tr, (P, Q, ub, ib))
    eng = _engine(tr, f, init, targets=True)
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        swapped = lc.pingpong(eng, d, HYPER, SEED, 0, iters, swap_last=False)
        assert swapped == 1
        loss = _loss_on_current_pair(eng, d, swapped)
    assert loss["mae"] == want["mae"] and loss["rmse"] == want["rmse"], (loss, want)
    gP, _, gub, _ = lc.verify(eng)
    gQt, gibt = eng.target
    _assert_equal((gP, gQt, gub, gibt), (P, Q, ub, ib), "ping-pong without the last swap")


# ------------------------------------------------------------------ inputs queued just ahead of the call
def _pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


@pytest.mark.parametrize("mode", ["ordered", "blocksolve"])
@widths
def test_inputs_copied_in_on_the_stream_just_ahead_of_the_call(min_rate, f, mode):
    tr = _set()
    d = _ratings(tr)  # (the schedule's popularity ranks are read from the real arrays, at creation)
    init, stale = _model(tr, f), _model(tr, f, seed=77)
    want = _oracle(tr, init, 0, ITERS)
    rng = np.random.RandomState(5)
    perm = rng.permutation(tr.nnz)
    if mode == "blocksolve":
        # warm-up on the null stream, same schedule, same ldq: the side stream exists, qstart has this ldq and the device's fork / join
        # form is decided, so BlockSolve::begin does not synchronise the stream of the call below
        warm = _engine(tr, f, init)
        warm.sgd(d, HYPER, SEED, 0, 1, mode=mode)
        lc.verify(warm)
    eng = _engine(tr, f, stale)
    assert mode != "blocksolve" or eng.ldq == warm.ldq
    real_img = {name: _pinned(lc.make_image(a, m.ld, m.front, m.back)) for (name, m), a in zip(eng.mats.items(), init[:2])}
    real = [(d.indptr, _pinned(tr.indptr)), (d.indices, _pinned(tr.indices)), (d.data, _pinned(tr.data)),
            (eng.mats["P"].flat, real_img["P"]), (eng.mats["Q"].flat, real_img["Q"]),
            (eng.user_bias, _pinned(init[2])), (eng.item_bias, _pinned(init[3]))]
    # valid stale contents first: the same indptr, in-range indices and ratings in another order, another model (already in eng)
    d.indices.copy_(torch.from_numpy(tr.indices[perm]))
    d.data.copy_(torch.from_numpy(tr.data[perm]))
    filler = torch.ones(16 << 20, dtype=torch.float32, device="cuda")  # 64 MB
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        filler.mul_(1.5)
        for dst, src in real:
            dst.copy_(src, non_blocking=True)
        eng.sgd(d, HYPER, SEED, 0, ITERS, mode=mode)
    got = lc.verify(eng)
    if mode == "ordered":
        _assert_equal(got, want, "ordered behind its inputs' copies")
    else:
        _assert_within(got, want, "block-solve behind its inputs' copies, f=%d" % f)
    assert not any(np.array_equal(g, s) for g, s in zip(got, stale))


# ------------------------------------------------------------------ one schedule, two models, two streams
@pytest.mark.parametrize("mode", ["ordered", "blocksolve"])
@widths
def test_one_schedule_two_models_two_streams(min_rate, f, mode):
    tr = _set()
    d = _ratings(tr)  # one DeviceRatings, so one api.Schedule
    init_a, init_b = _model(tr, f), _model(tr, f, seed=11)
    a, b = _engine(tr, f, init_a), _engine(tr, f, init_b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a.sgd(d, HYPER, SEED, 0, ITERS, mode=mode)
    with torch.cuda.stream(s2):
        b.sgd(d, HYPER, SEED, 0, ITERS, mode=mode)  # no ordering by the caller: the schedule's workspace is the library's
    s2.wait_stream(s1)  # A's buffers are the caller's: its second call is ordered behind its first by the caller
    with torch.cuda.stream(s2):
        a.sgd(d, HYPER, SEED, ITERS, ITERS, mode=mode)
    got_a, got_b = lc.verify(a), lc.verify(b)
    want_a, want_b = _oracle(tr, init_a, 0, 2 * ITERS), _oracle(tr, init_b, 0, ITERS)
    if mode == "ordered":
        _assert_equal(got_a, want_a, "model A, two streams")
        _assert_equal(got_b, want_b, "model B, the other stream")
    else:
        _assert_within(got_a, want_a, "model A, two streams, f=%d" % f)
        _assert_within(got_b, want_b, "model B, the other stream, f=%d" % f)
        # and the null stream's bits: the same three calls one after the other
        na, nb = _engine(tr, f, init_a), _engine(tr, f, init_b)
        na.sgd(d, HYPER, SEED, 0, ITERS, mode=mode)
        nb.sgd(d, HYPER, SEED, 0, ITERS, mode=mode)
        na.sgd(d, HYPER, SEED, ITERS, ITERS, mode=mode)
        assert _same_bits(got_a, lc.verify(na)) and _same_bits(got_b, lc.verify(nb)), "not the null stream's bits"
    assert lib().cu2rec_check_faults() == 0


# ------------------------------------------------------------------ resident launches from two streams
@widths
def test_resident_launches_from_two_streams_back_to_back(f):
    own = _own_item_set(f)
    d = _ratings(own)
    init_a, init_b = _model(own, f), _model(own, f, seed=23)
    a, b = _engine(own, f, init_a), _engine(own, f, init_b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    refusals = lib().cu2rec_hogwild_resident_refusals()
    with resident_policy(FORCE):
        assert lib().cu2rec_hogwild_resident_plan(own.rows, f, ITERS, None, None) == 1
        with torch.cuda.stream(s1):
            a.sgd(d, HYPER, SEED, 0, ITERS, mode="hogwild")
        with torch.cuda.stream(s2):
            b.sgd(d, HYPER, SEED, 0, ITERS, mode="hogwild")
    _assert_equal(lc.verify(a), _oracle(own, init_a, 0, ITERS), "resident launch on the first stream")
    _assert_equal(lc.verify(b), _oracle(own, init_b, 0, ITERS), "resident launch on the second stream")
    assert lib().cu2rec_check_faults() == 0  # CU2REC_OK
    assert lib().cu2rec_hogwild_resident_refusals() == refusals
