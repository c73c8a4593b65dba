"""Every compiled row width (-m gpu).  The SGD kernels and the loss pass are templates over J = ceil(ceil(f / 4) / 16) float4
slots per lane (kernels.hip launch_sgd / launch_loss / launch_sgd_pingpong, ordered.hip); the library accepts f up to 512, so
J runs from 1 to 8.  FACTORS holds both sides of every J boundary, every f % 4, and both sides of the block-solve mode's limit
(252 factors = 63 slots).  At each width, on one small set:
  * serial, ordered, ping-pong, Hogwild on a collision-free set and Hogwild with the item side frozen are the oracle's
    result bit for bit (TREE16 dot order, the kernels' own);
  * the loss pass is the oracle's bit for bit, on the initial model and on a trained one;
  * block-solve is within 2e-6 of the oracle up to 252 factors and refused with CU2REC_EUNSUPPORTED above, where train()'s
    default mode is the ordered walk;
  * the padding floats of P (stride ld) and Q (stride ldq), read back padded straight from device memory, are still zero
    after every mode, in both buffer pairs of ping-pong."""
import ctypes as C

import numpy as np
import pytest

import cu2rec_amd as cu
from cu2rec_amd import api, synth
from cu2rec_amd._lib import lib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HYPER = (0.01, 0.02, 0.02, 0.02, 0.02)
FACTORS = [1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 252, 253, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512]
ITERS = 3


def _as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


_SETS = {}


def _set():
    if "tr" not in _SETS:
        _SETS["tr"] = synth.make_ratings(300, 120, 3000, min_degree=3, seed=21)[0]
    return _SETS["tr"]


def _hip():
    # the HIP runtime the library is linked against (already loaded by lib(): dlopen by soname returns that copy)
    if "hip" not in _SETS:
        lib()
        h = C.CDLL("libamdhip64.so.7")
        h.hipMemcpy.restype = C.c_int
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _SETS["hip"] = h
    return _SETS["hip"]


def _raw(ptr, rows, stride):
    """rows x stride floats from device address ptr, padding included (hipMemcpyDeviceToHost = 2)."""
    out = np.empty((rows, stride), np.float32)
    assert _hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def _item_stride(model):
    return lib().cu2rec_model_item_stride(model._h)


def _check_padding(model, f, q_ptrs=()):
    """P[:, f:ld] and Q[:, f:ldq] are exactly zero, for the model's current Q and any other item buffers named in q_ptrs."""
    P, Q, _, _ = model.device_ptrs()
    ld, ldq = model.ld, _item_stride(model)
    assert ld % 4 == 0 and ld >= f and ldq % 32 == 0 and ldq >= f
    hP = _raw(P, model.rows, ld)
    assert not hP[:, f:].any(), "P padding written (f=%d, ld=%d)" % (f, ld)
    for q in {Q, *q_ptrs}:
        hQ = _raw(q, model.cols, ldq)
        assert not hQ[:, f:].any(), "Q padding written (f=%d, ldq=%d)" % (f, ldq)
    return hP, ld, ldq


def _assert_equal(model, state):
    for name, g, w in zip(("P", "Q", "user_bias", "item_bias"), model.download(), state):
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("f", FACTORS)
def test_serial_and_ordered_bit_exact_and_loss(f):
    tr = _set()
    d = cu.DeviceCSR(tr)
    state = orc.init_model(tr.rows, tr.cols, f)
    fresh = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    _check_padding(fresh, f)
    want = orc.loss(_as_orc(tr), *state, tr.global_bias, dot_order=orc.DOT_TREE16)
    got = fresh.loss(d)
    assert got["rmse"] == want["rmse"] and got["mae"] == want["mae"], (got, want)
    orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, 42, 0, ITERS, dot_order=orc.DOT_TREE16)
    want = orc.loss(_as_orc(tr), *state, tr.global_bias, dot_order=orc.DOT_TREE16)
    for mode in ("serial", "ordered"):
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(d, HYPER, 42, 0, ITERS, mode=mode)
        _assert_equal(model, state)
        _check_padding(model, f)
        got = model.loss(d)
        assert got["rmse"] == want["rmse"] and got["mae"] == want["mae"], (mode, got, want)


@pytest.mark.parametrize("f", FACTORS)
def test_pingpong_bit_exact_in_both_buffer_pairs(f):
    tr = _set()
    d = cu.DeviceCSR(tr)
    for iters in (ITERS, ITERS + 1):  # odd: the current item side is the second pair; even: the first
        P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
        Qt, ibt = Q.copy(), ib.copy()
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        q_before = model.device_ptrs()[1]
        model.sgd(d, HYPER, 42, 0, iters, mode="pingpong")
        q_after = model.device_ptrs()[1]
        assert (q_after != q_before) == (iters % 2 == 1)
        orc.sgd_pingpong_iterations(_as_orc(tr), P, Q, Qt, ub, ib, ibt, tr.global_bias, HYPER, 42, 0, iters,
                                    dot_order=orc.DOT_TREE16)
        _assert_equal(model, (P, Q, ub, ib))
        _check_padding(model, f, q_ptrs=(q_before,))
        # the other pair holds the item side of one iteration earlier (the oracle's target buffers after its swap)
        ldq = _item_stride(model)
        other = q_before if q_after != q_before else None
        if other is not None:
            np.testing.assert_array_equal(_raw(other, tr.cols, ldq)[:, :f], Qt)


def _own_item_set(f, n=300):
    # every user rates only its own item: no two updates of an iteration touch the same row, so the streaming Hogwild launch
    # has the sequential result bit for bit (the construction of test_sgd_hogwild_exact_when_no_item_is_shared)
    rng = np.random.RandomState(f)
    return cu.HostCSR(np.arange(n + 1), rng.permutation(n), rng.randint(1, 6, n).astype(np.float32), n, n, 3.0)


@pytest.mark.parametrize("f", FACTORS)
def test_hogwild_bit_exact_where_no_update_races(f):
    n = 300
    m = _own_item_set(f, n)
    prev = lib().cu2rec_hogwild_resident(0)  # streaming launches only
    try:
        state = orc.init_model(n, n, f)
        model = cu.Model(n, n, f, 3.0)
        model.sgd(cu.DeviceCSR(m), HYPER, 42, 0, ITERS, mode="hogwild")
        orc.sgd_iterations(_as_orc(m), *state, 3.0, HYPER, 42, 0, ITERS, dot_order=orc.DOT_TREE16)
        _assert_equal(model, state)
        _check_padding(model, f)
        # item side frozen: users never share anything, any rating set is exact
        tr = _set()
        state = orc.init_model(tr.rows, tr.cols, f)
        model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        model.sgd(cu.DeviceCSR(tr), HYPER, 42, 0, ITERS, mode="hogwild", update_items=False)
        orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, 42, 0, ITERS, dot_order=orc.DOT_TREE16,
                           update_items=False)
        _assert_equal(model, state)
        _check_padding(model, f)
    finally:
        lib().cu2rec_hogwild_resident(prev)


@pytest.fixture
def min_rate():
    prev = api.blocksolve_min_rate()
    yield api.blocksolve_min_rate
    api.blocksolve_min_rate(prev)


@pytest.mark.parametrize("f", FACTORS)
def test_blocksolve_within_2e6_or_refused_above_252(min_rate, f):
    tr = _set()
    min_rate(1.0)  # read when the schedule is created: the DeviceCSR below has hot chains
    d = cu.DeviceCSR(tr)
    model = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
    if f <= 252:
        assert d.blocksolve_items() > 0
        state = orc.init_model(tr.rows, tr.cols, f)
        model.sgd(d, HYPER, 42, 0, ITERS, mode="blocksolve")
        orc.sgd_iterations(_as_orc(tr), *state, tr.global_bias, HYPER, 42, 0, ITERS, dot_order=orc.DOT_TREE16)
        diffs = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(model.download(), state)]
        assert max(diffs) <= 2e-6, diffs  # float rounding of re-associated sums
        _check_padding(model, f)
        return
    before = model.download()
    with pytest.raises(cu.Cu2recError) as e:
        model.sgd(d, HYPER, 42, 0, ITERS, mode="blocksolve")
    assert e.value.status == -6  # CU2REC_EUNSUPPORTED
    indptr, indices, data = d.device_ptrs()
    P, Q, ub, ib = model.device_ptrs()
    sched = api.Schedule(indptr, indices, tr.rows, tr.cols, tr.nnz)
    try:
        with pytest.raises(cu.Cu2recError) as e:
            api.sgd_update_blocksolve(sched, indptr, indices, data, tr.rows, tr.cols, P, model.ld, Q, _item_stride(model), ub, ib,
                                      tr.global_bias, f, HYPER, 42, 0, ITERS)
        assert e.value.status == -6
    finally:
        sched.close()
    for g, w in zip(model.download(), before):  # a refused call changes nothing
        np.testing.assert_array_equal(g, w)
    _check_padding(model, f)


@pytest.mark.parametrize("f", [252, 253])
def test_train_default_mode_either_side_of_252(min_rate, f):
    """train() without a mode: block-solve up to 252 factors, the ordered walk (the oracle's result bit for bit) above."""
    tr = _set()
    te = synth.make_ratings(300, 120, 3000, min_degree=3, seed=22)[0]
    min_rate(1.0)
    assert api.default_mode(f) == (api.SGD_BLOCKSOLVE if f <= 252 else api.SGD_ORDERED)
    cfg = cu.default_config(total_iterations=4, n_factors=f, check_error=2, learning_rate=0.02, patience=1.0)
    ocfg = orc.default_config(total_iterations=4, n_factors=f, check_error=2, learning_rate=0.02, patience=1.0)
    P, Q, ub, ib = orc.init_model(tr.rows, tr.cols, f)
    orc.train(_as_orc(tr), _as_orc(te), ocfg, P, Q, ub, ib, tr.global_bias, dot_order=orc.DOT_TREE16, acc=orc.ACC_F64)
    gP, gQ, _, gub, gib = cu.train(tr, te, cfg, verbose=False)
    for g, w in zip((gP, gQ, gub, gib), (P, Q, ub, ib)):
        if f <= 252:  # block-solve: float rounding of re-associated sums (the bound of test_blocksolve_train_loop_matches_ordered)
            assert float(np.abs(g.astype(np.float64) - w).max()) <= 1e-5
        else:
            np.testing.assert_array_equal(g, w)
