"""TEST INFRASTRUCTURE shared by tests/test_gpu_ials.py and tests/test_ials_cpu.py: the entry sets of the GPU half-step tests (the
CPU suite solves every judged row of every one of them with the float32 restatement, to show that they are fair, and with four
deliberate mistakes in float64, to show that they can tell), and the judgement of one GPU half-step against the float64
reference (tests/ials_reference64.py).  Nothing here needs a GPU to be imported."""
import ctypes as C

import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api
from cu2rec_amd._lib import lib

import als_checks as chk
import ials_reference64 as ref
from als_checks import model_from, q_padding, random_state, same_bits

# (learning rate, P_reg, Q_reg, user_bias_reg, item_bias_reg): only the two factor regularisers are read.  They are of O(1) on the
# large sets: there G0's diagonal is 0.09 x the partner count (370 at 4,137 partners, 5,900 at 65,617), and a regulariser of 0.05
# multiplied by a row's length, the explicit objective's form, would move no row by the bar -- a mistake the tests must see.
HYPER = (0.01, 0.8, 1.2, 0.02, 0.03)
SMALL_HYPER = (0.01, 0.05, 0.04, 0.02, 0.03)  # the small-partner sets: G0 has rank 40 < f, reg alone bounds the other 60 directions
WIDTHS = [1, 8, 30, 31, 100, 126, 252]
EXTRA_LONG = (31, 252)  # widths whose width x length set also holds the row of 64 x 1,024 + 1 entries
# The sets cu2rec_model_implicit_objective is compared on, and the relative error of its float32 restatement
# (ials_reference64.objective_f32: float32 Grams summed in the kernels' order) on them, measured by tests/test_ials_cpu.py:
# 3.69e-9, 2.25e-9, 2.04e-9, 7.9e-11.  The GPU test allows four times the worst, for the freedom in accumulation order.
OBJECTIVE_SETS = ("lengths-f100-users", "lengths-f252-users", "small-partners-f100-users", "batches-f30-40x17")
OBJECTIVE_RESTATEMENT_ERROR = 3.7e-9
_CACHE = {}


class Case:
    """One half-step: `csr` is what the model is trained on (user-major), `side` the side solved; every row of that side with
    entries is judged."""

    def __init__(self, name, csr, side, f, alpha, hyper, seed):
        self.name, self.csr, self.side, self.f, self.alpha, self.hyper, self.seed = name, csr, side, f, alpha, hyper, seed

    def state(self):
        """float32 (P, Q, user_bias, item_bias) of O(0.3) / O(0.1), with model rows past the CSR on both sides."""
        return random_state(self.csr.rows + 3, self.csr.cols + 5, self.f, self.seed)

    def system(self):
        """(indptr, indices, data, X, reg): the side's entries as it reads them, its partner rows [0, n) and its regulariser."""
        P, Q, _, _ = self.state()
        indptr, indices, data, n = ref.own_major(self.csr, self.side)
        return indptr, indices, data, (Q if self.side == "users" else P)[:n], self.hyper[1 if self.side == "users" else 2]

    def judged(self):
        indptr = ref.own_major(self.csr, self.side)[0]
        return np.flatnonzero(np.diff(indptr) > 0)


def small_partner_set():
    """70 rows over 40 partners: rows of 1 .. 40 distinct partners, then 30 rows of 41 .. 64 entries drawn with repeats; entries of
    half stars 0.5 .. 5 and a few exact zeros."""
    if "small" not in _CACHE:
        rng = np.random.default_rng(1234)
        per_row = [np.sort(rng.choice(40, n, replace=False)) for n in range(1, 41)]
        per_row += [np.sort(rng.integers(0, 40, 41 + (i % 24))) for i in range(30)]
        csr = chk.csr_from_rows(per_row, 40, rng)
        csr.data[::17] = 0.0
        _CACHE["small"] = csr
    return _CACHE["small"]


def messy_set():
    """150 users x 60 items: unsorted items, repeated (user, item) pairs with different values, entries of exactly 0, users and
    items without entries (the last three items among them)."""
    if "messy" not in _CACHE:
        rng = np.random.default_rng(17)
        rows, cols = 150, 60
        counts = rng.multinomial(3000, np.ones(rows) / rows)
        counts[[0, rows // 2, rows - 1]] = 0
        items = rng.integers(0, cols - 3, counts.sum())
        items[rng.random(len(items)) < 0.2] = 1
        indptr = np.zeros(rows + 1, np.int64)
        indptr[1:] = np.cumsum(counts)
        values = rng.integers(0, 11, len(items)).astype(np.float32) / 2
        _CACHE["messy"] = api.HostCSR(indptr, items, values, rows, cols, 0.0)
    return _CACHE["messy"]


def tile_edge_set(partners):
    """Five rows (1, 5, 40, 1,024 and all partners) over exactly `partners` partner rows: G0's last tile full, of one row, of one
    row after two full ones."""
    if ("tiles", partners) not in _CACHE:
        rng = np.random.default_rng(partners)
        per_row = [np.sort(rng.choice(partners, n, replace=False)) for n in (1, 5, 40, 1024, partners)]
        _CACHE[("tiles", partners)] = chk.csr_from_rows(per_row, partners, rng)
    return _CACHE[("tiles", partners)]


def cases():
    """name -> Case, every set the GPU half-step tests judge."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = {}

    def add(name, *args):
        out[name] = Case(name, *args)

    for f in WIDTHS:
        rows_major = chk.width_length_set(extra_long=f in EXTRA_LONG)
        alpha = 40.0 if f in (8, 31, 100, 252) else 1.0
        add("lengths-f%d-users" % f, rows_major, "users", f, alpha, HYPER, 5000 + f)
        add("lengths-f%d-items" % f, rows_major.transpose(), "items", f, alpha, HYPER, 5500 + f)
    # long item rows over one and two workspace batches (455 partial Grams fit at f = 252: 36 tile pairs)
    add("batches-f252-40x17", chk.batch_set(40, 17).transpose(), "items", 252, 40.0, HYPER, 6001)
    add("batches-f252-9x64", chk.batch_set(9, 64).transpose(), "items", 252, 1.0, HYPER, 6002)
    add("batches-f30-40x17", chk.batch_set(40, 17).transpose(), "items", 30, 40.0, HYPER, 6003)
    add("small-partners-f100-users", small_partner_set(), "users", 100, 1.0, SMALL_HYPER, 6101)
    add("small-partners-f100-items", small_partner_set().transpose(), "items", 100, 1.0, SMALL_HYPER, 6102)
    for partners in (1024, 1025, 2049):  # the G0 tile edges
        for f in (8, 31):
            add("tiles-%d-f%d-users" % (partners, f), tile_edge_set(partners), "users", f, 1.0, HYPER, 6300 + f)
    add("tiles-1025-f8-items", tile_edge_set(1025).transpose(), "items", 8, 1.0, HYPER, 6400)  # G0 over X = P
    # entries of 0, repeated pairs, rows without entries; alpha = 0 is the system G0 + reg I against sum q
    for alpha in (40.0, 0.0):
        for f in (8, 30):
            for side in ("users", "items"):
                add("messy-alpha%d-f%d-%s" % (alpha, f, side), messy_set(), side, f, alpha, HYPER, 6200 + f)
    _CACHE["cases"] = out
    return out


def bar_ratio(x, xs):
    """max over rows of |x - x*|_inf / (1e-3 max(1, |x*|_inf)): at most 1 when every row meets the project's forward bar."""
    x, xs = np.asarray(x, np.float64), np.asarray(xs, np.float64)
    if len(xs) == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        ratio = np.abs(x - xs).max(axis=1) / (1e-3 * np.maximum(1.0, np.abs(xs).max(axis=1)))
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def ials(model, d_csr, hyper, alpha, side):
    n = C.c_int(-1)
    h = cu.Hyper(*[float(x) for x in hyper])
    s = api.SIDES[side] if isinstance(side, str) else side
    rc = lib().cu2rec_model_als_implicit(model._h, d_csr._h, C.byref(h), float(alpha), s, C.byref(n))
    return rc, n.value


def check_half_step(model, d_csr, csr, side, hyper, alpha, report=None):
    """One GPU half-step against the float64 reference from the same float32 state; returns the state after it.
    The other side, the model rows past the CSR (factors and biases) and Q's padding keep their bits; inside the CSR the solved
    side's biases are exactly 0 and rows without entries exactly zero; unsolved == 0; every row with entries is within
    1e-3 max(1, |x*|_inf) of the float64 optimum x*."""
    f = model.n_factors
    before = model.download()
    pad_before = q_padding(model, f)
    rc, unsolved = ials(model, d_csr, hyper, alpha, side)
    assert rc == 0, (rc, lib().cu2rec_last_error())
    got = model.download()
    own, other = ((0, 2), (1, 3)) if side == "users" else ((1, 3), (0, 2))
    n_own = csr.rows if side == "users" else csr.cols
    for k in other:
        assert same_bits(got[k], before[k]), "the other side moved (%s half-step, f=%d)" % (side, f)
    for k in own:
        assert same_bits(got[k][n_own:], before[k][n_own:]), "model rows past the CSR moved (%s, f=%d)" % (side, f)
    pad = q_padding(model, f)
    assert not pad[:csr.cols].any() and same_bits(pad[csr.cols:], pad_before[csr.cols:])
    if side == "users":
        assert same_bits(pad, pad_before)
    assert unsolved == 0, (side, f, unsolved)
    assert same_bits(got[own[1]][:n_own], np.zeros(n_own, np.float32)), "a solved bias is not +0.0"
    indptr, indices, data, n_part = ref.own_major(csr, side)
    empty = np.flatnonzero(np.diff(indptr) == 0)
    assert same_bits(got[own[0]][empty], np.zeros((len(empty), f), np.float32)), "a row without entries is not the zero row"
    rated = np.flatnonzero(np.diff(indptr) > 0)
    want = ref.solve_rows(indptr, indices, data, before[other[0]][:n_part], hyper[1 if side == "users" else 2], alpha, rows=rated)
    worst = bar_ratio(got[own[0]][rated], want)
    if report is not None:
        report[(side, f)] = worst
    assert worst <= 1.0, ("rows off the float64 optimum, in units of the bar", side, f, worst)
    return got
