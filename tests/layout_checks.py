"""TEST INFRASTRUCTURE shared by tests/test_gpu_layouts.py, tests/test_gpu_streams.py and tests/test_layout_checks_cpu.py: factor
matrices at caller-chosen row strides and base offsets, inside guarded allocations.

include/cu2rec_amd.h lets the caller of the raw-pointer entry points choose any row stride that is a multiple of 4 floats and at
least n_factors, and any 16-byte aligned base.  cu2rec_amd/engine.py and cu2rec_model always choose ld = round4(f) for P,
ldq = round32(f) for Q and the start of a fresh allocation; LAYOUTS holds four other choices, each isolating one assumption a kernel
could make (the table below).

Each of P, Q and Q_target lives in ONE flat float32 tensor [front guard | rows x ld | back guard].  Both guards are at least ld + 64
floats of one NaN bit pattern (SENTINEL), the columns f .. ld of every row are zero as the header requires, and the row region's
address goes to the library.  A kernel that takes ldp where it means ldq, reads a Q row in whole 32-float tiles or steps one row
too far then reads or writes memory the test owns: it produces a wrong number or a touched guard (check_image names the region, the
row and the column), not a fault.

Nothing here needs a GPU to be imported; torch and the engine are imported where a device is first needed."""
import collections
import ctypes as C

import numpy as np

from cu2rec_amd._lib import Hyper, check, lib

# the widths of tests/test_gpu_layouts.py: each f % 4, f % 32 == 0 and not, both sides of the 252-factor block-solve limit, and
# J = ceil(ceil(f / 4) / 16) = 1, 2, 3, 4, 5 and 8 float4 slots per lane (6 and 7 are left to tests/test_gpu_row_widths.py)
WIDTHS = [1, 4, 5, 36, 63, 64, 100, 129, 252, 253, 256, 300, 512]
SENTINEL = 0x7FA5A5A5  # a NaN: any arithmetic that takes a guard word in shows in the result


def round4(f):
    return (f + 3) & ~3


def round32(f):
    return (f + 31) & ~31


def _crossed_ldq(f):
    # round4(f) + 4, and four more where that is a multiple of 32 (f = 25 .. 28 mod 32: 252 + 4 = 256): this stride is never one
    ldq = round4(f) + 4
    return ldq + 4 if ldq % 32 == 0 else ldq


# name, ldp(f), ldq(f), floats by which the row region is moved off its 256-byte aligned place
Layout = collections.namedtuple("Layout", "name ldp ldq offset")
LAYOUTS = [
    # no padding when f % 4 == 0 and Q rows that share 128-byte lines: the reference's own layout
    Layout("dense", round4, round4, 0),
    # ldp > ldq and an ldq that is never a multiple of 32: ldp taken for ldq (or the reverse) reads other rows
    Layout("crossed", lambda f: round32(f) + 32, _crossed_ldq, 0),
    # a large stride: 32-bit offset arithmetic, "row + 1 is next to row"
    Layout("wide", lambda f: 2 * round32(f) + 4, lambda f: 2 * round32(f) + 4, 0),
    # the project's default strides on a base that is 16-byte aligned and nothing more
    Layout("offset16", round4, round32, 4),
]
DEFAULT = Layout("default", round4, round32, 0)  # what engine.py and cu2rec_model choose, here with guards around it
BY_NAME = {lay.name: lay for lay in LAYOUTS + [DEFAULT]}


def guard_sizes(ld, offset):
    """(front, back) guard lengths in floats: both >= ld + 64; the front one a multiple of 64 floats (256 bytes) plus `offset`."""
    return ((ld + 64 + 63) & ~63) + offset, ld + 64


def make_image(dense, ld, front, back):
    """The flat float32 array [front guard | rows x ld | back guard] holding `dense` (rows x f) at row stride ld."""
    rows, f = dense.shape
    assert ld >= f and dense.dtype == np.float32
    bits = np.full(front + rows * ld + back, SENTINEL, np.uint32)
    body = bits[front:front + rows * ld].reshape(rows, ld)
    body[:] = 0
    body[:, :f] = dense.view(np.uint32)
    return bits.view(np.float32)


def dense_block(host_flat, rows, f, ld, guard_front):
    """rows x f from a flat image, unchecked."""
    return host_flat[guard_front:guard_front + rows * ld].reshape(rows, ld)[:, :f].copy()


def check_image(host_flat, rows, f, ld, guard_front, guard_back, what="image"):
    """The guards are bit for bit the sentinel and the padding columns f .. ld are zero -> the dense rows x f block.  A failure
    names the region and the first offending word's row and column, counted from the row region's start at stride ld (row -1 is in
    the front guard, row `rows` the first of the back guard)."""
    bits = np.ascontiguousarray(host_flat).view(np.uint32).reshape(-1)
    n = rows * ld
    assert bits.size == guard_front + n + guard_back, "%s: %d floats, expected %d" % (what, bits.size, guard_front + n + guard_back)
    for region, lo, hi in (("front guard", 0, guard_front), ("back guard", guard_front + n, bits.size)):
        bad = np.flatnonzero(bits[lo:hi] != SENTINEL)
        if bad.size:
            at = lo + int(bad[0]) - guard_front
            raise AssertionError("%s: %s touched, %d words; the first at row %d, column %d (stride %d, f %d): 0x%08X"
                                 % (what, region, bad.size, at // ld, at % ld, ld, f, bits[lo + int(bad[0])]))
    body = bits[guard_front:guard_front + n].reshape(rows, ld).view(np.float32)
    bad = np.argwhere(body[:, f:] != 0)  # (NaN != 0 holds: a guard word copied into the padding counts)
    if bad.size:
        r, c = int(bad[0][0]), f + int(bad[0][1])
        raise AssertionError("%s: padding not zero in %d places; the first at row %d, column %d (stride %d, f %d): %r"
                             % (what, len(bad), r, c, ld, f, float(body[r, c])))
    return body[:, :f].copy()


# ---- on the device -----------------------------------------------------------------------------------------------------------
class Guarded:
    """One factor matrix in its guarded flat tensor; `view` is the rows x ld strided view whose data_ptr() the library gets."""

    def __init__(self, name, dense, ld, offset, device):
        import torch
        dense = np.ascontiguousarray(dense, np.float32)
        self.name, (self.rows, self.f), self.ld = name, dense.shape, ld
        self.front, self.back = guard_sizes(ld, offset)
        self.flat = torch.from_numpy(make_image(dense, ld, self.front, self.back)).to(device)
        self.view = self.flat[self.front:self.front + self.rows * ld].view(self.rows, ld)
        ptr = self.view.data_ptr()
        assert ptr % 256 == 4 * offset, "the allocation's start is not 256-byte aligned"

    def host(self):
        return self.flat.cpu().numpy()

    def dense(self):
        return check_image(self.host(), self.rows, self.f, self.ld, self.front, self.back, self.name)


def strided_engine(layout, rows, cols, f, global_bias, P, Q, user_bias, item_bias, targets=False, device=None):
    """A cu2rec_amd.engine.Engine on the given dense host arrays whose P and Q are guarded views at the layout's strides.
    targets: also Q_target / item_bias_target (copies of Q / item_bias, as cu2rec_sgd_update_pingpong wants them) and claim."""
    import torch
    from cu2rec_amd.engine import Engine

    eng = Engine(rows, cols, f, global_bias, P, Q, user_bias, item_bias, device=device)
    eng.layout = layout
    eng.ld, eng.ldq = layout.ldp(f), layout.ldq(f)
    eng.mats = {"P": Guarded("P", P, eng.ld, layout.offset, eng.device), "Q": Guarded("Q", Q, eng.ldq, layout.offset, eng.device)}
    eng.P, eng.Q = eng.mats["P"].view, eng.mats["Q"].view
    eng.Q_target = eng.item_bias_target = eng.claim = None
    if targets:
        eng.mats["Q_target"] = Guarded("Q_target", Q, eng.ldq, layout.offset, eng.device)
        eng.Q_target = eng.mats["Q_target"].view
        eng.item_bias_target = eng.item_bias.clone()
        eng.claim = torch.empty(max(cols, 1), dtype=torch.int64, device=eng.device)
    torch.cuda.synchronize(eng.device)
    return eng


def pingpong(eng, ratings, hyper, seed, iter0, n_iters, swap_last=True, update_items=True, P=None, ldp=None, Q=None, ldq=None,
             Q_target=None):
    """cu2rec_sgd_update_pingpong on the engine's two buffer pairs and torch's current stream -> *swapped.  P, ldp, Q, ldq, Q_target:
    addresses / strides passed in place of the engine's own (the refusal tests)."""
    from cu2rec_amd.engine import _stream_ptr
    swapped, h = C.c_int(-1), Hyper(*[float(x) for x in hyper])
    check(lib().cu2rec_sgd_update_pingpong(
        ratings.indptr.data_ptr(), ratings.indices.data_ptr(), ratings.data.data_ptr(), ratings.rows, eng.cols,
        eng.P.data_ptr() if P is None else P, eng.ld if ldp is None else ldp, eng.Q.data_ptr() if Q is None else Q,
        eng.Q_target.data_ptr() if Q_target is None else Q_target, eng.ldq if ldq is None else ldq, eng.user_bias.data_ptr(),
        eng.item_bias.data_ptr(),
        eng.item_bias_target.data_ptr(), eng.claim.data_ptr(), eng.global_bias, eng.f, C.byref(h), int(seed), int(iter0), int(n_iters),
        1 if update_items else 0, 0, 1 if swap_last else 0, C.byref(swapped), _stream_ptr()))
    return swapped.value


def verify(eng):
    """After the device is idle: every guard untouched and every padding float zero in P, Q and (where present) Q_target
    -> (P, Q, user_bias, item_bias) dense; the checked Q_target and item_bias_target are left in eng.target."""
    import torch
    torch.cuda.synchronize(eng.device)
    dense = {name: m.dense() for name, m in eng.mats.items()}
    eng.target = (dense["Q_target"], eng.item_bias_target.cpu().numpy()) if "Q_target" in dense else None
    return dense["P"], dense["Q"], eng.user_bias.cpu().numpy(), eng.item_bias.cpu().numpy()


def snapshot(eng):
    """Every word the engine owns, guards included."""
    import torch
    torch.cuda.synchronize(eng.device)
    out = {name: m.host().view(np.uint32) for name, m in eng.mats.items()}
    for name in ("user_bias", "item_bias", "item_bias_target"):
        if getattr(eng, name, None) is not None:
            out[name] = getattr(eng, name).cpu().numpy().view(np.uint32)
    return out


def assert_unchanged(eng, before):
    after = snapshot(eng)
    assert after.keys() == before.keys()
    for name in before:
        np.testing.assert_array_equal(after[name], before[name], err_msg="%s changed" % name)
