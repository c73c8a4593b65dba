"""TEST INFRASTRUCTURE shared by tests/test_gpu_ials.py, tests/test_gpu_ials_edges.py and tests/test_ials_cpu.py: the entry sets of
the GPU half-step tests (the CPU suite solves every judged row of every one of them with the float32 restatement, to show that
they are fair, and with five deliberate mistakes in float64, to show that they can tell), and the judgement of one GPU half-step
against the float64 reference (tests/ials_reference64.py).  Nothing here needs a GPU to be imported."""
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
# 32 NT - 1 (the last staged tile exactly full: f columns and the right-hand side's weight) and 32 NT (one more tile for that weight
# alone), NT = ials_tiles(f) = 1 .. 8 -- with the 31 and 252 above, both edges of every compiled tile count
EDGE_WIDTHS = [32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224]
EXTRA_LONG = (31, 252, 95)  # widths whose width x length set also holds the row of 64 x 1,024 + 1 entries
# The sets cu2rec_model_implicit_objective is compared on, and the relative error of its float32 restatement
# (ials_reference64.objective_f32: float32 Grams summed in the kernels' order) on them, measured by tests/test_ials_cpu.py:
# 3.69e-9, 2.25e-9, 2.04e-9, 7.9e-11 on the first four; 4.42e-8, 3.58e-9, 1.99e-8, 1.03e-8, 9.73e-9, 4.68e-8 on the edge widths
# 32, 63, 96, 160, 191, 224 (at the even ones alpha is 1: the entries term is smaller and the float32 Grams' share of the
# objective larger); 3.6e-11 and 8.9e-10 on the two sets of objective_loop_cases().  The GPU tests allow four times the worst,
# for the freedom in accumulation order.
OBJECTIVE_SETS = ("lengths-f100-users", "lengths-f252-users", "small-partners-f100-users", "batches-f30-40x17",
                  "lengths-f32-users", "lengths-f63-users", "lengths-f96-users", "lengths-f160-users", "lengths-f191-users",
                  "lengths-f224-users")
OBJECTIVE_LOOP_SETS = ("objective-loop-entries", "objective-loop-rows")
OBJECTIVE_RESTATEMENT_ERROR = 4.7e-8
OBJECTIVE_LOOP = 4096 * 16 * 8  # entries / rows one trip of ials_objective_kernel's grid-stride loops covers (als.hip)
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
        return self.system_of(self.state())

    def system_of(self, state):
        P, Q, _, _ = state
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

    for f in WIDTHS + EDGE_WIDTHS:
        rows_major = chk.width_length_set(extra_long=f in EXTRA_LONG)
        alpha = 40.0 if f in (8, 31, 100, 252) or (f in EDGE_WIDTHS and f % 2) else 1.0
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


def check_half_step(model, d_csr, csr, side, hyper, alpha, report=None, may_fail=None):
    """One GPU half-step against the float64 reference from the same float32 state; returns the state after it.
    The other side, the model rows past the CSR (factors and biases) and Q's padding keep their bits; inside the CSR the solved
    side's biases are exactly 0 and rows without entries exactly zero; every solved row with entries is within
    1e-3 max(1, |x*|_inf) of the float64 optimum x*.
    may_fail: None -- `unsolved` must be 0 and every row with entries is judged, one that kept its bits included.  Otherwise the
        rows (ids of this side) that are allowed to be left unsolved, by the rules of als_checks.check_half_step(singular=...):
        `unsolved` must equal the number of rows with entries that kept their bits (factors and bias), each of them must be
        listed here, and every other row with entries is judged.
    report: a dict that receives the worst ratio under (side, f) and, with may_fail, the count under "unsolved" and the kept
        rows under "kept"."""
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
    indptr, indices, data, n_part = ref.own_major(csr, side)
    rated = np.flatnonzero(np.diff(indptr) > 0)
    if may_fail is None:
        assert unsolved == 0, (side, f, unsolved)
        kept = np.zeros(0, np.int64)
    else:
        x_all = np.concatenate([got[own[0]], got[own[1]][:, None]], axis=1)[rated]
        x0_all = np.concatenate([before[own[0]], before[own[1]][:, None]], axis=1)[rated]
        kept = rated[(np.ascontiguousarray(x_all).view(np.uint32) == np.ascontiguousarray(x0_all).view(np.uint32)).all(axis=1)]
        assert unsolved == len(kept), (side, f, unsolved, kept[:8].tolist())
        stray = np.setdiff1d(kept, np.asarray(list(may_fail), np.int64))
        assert len(stray) == 0, ("rows left unsolved that should have been solved", side, f, stray[:8].tolist())
    done = np.setdiff1d(np.arange(n_own), kept)
    assert same_bits(got[own[1]][done], np.zeros(len(done), np.float32)), "a solved bias is not +0.0"
    empty = np.flatnonzero(np.diff(indptr) == 0)
    assert same_bits(got[own[0]][empty], np.zeros((len(empty), f), np.float32)), "a row without entries is not the zero row"
    judged = np.setdiff1d(rated, kept)
    want = ref.solve_rows(indptr, indices, data, before[other[0]][:n_part], hyper[1 if side == "users" else 2], alpha, rows=judged)
    worst = bar_ratio(got[own[0]][judged], want)
    if report is not None:
        report[(side, f)] = worst
        if may_fail is not None:
            report["unsolved"], report["kept"] = unsolved, kept
    assert worst <= 1.0, ("rows off the float64 optimum, in units of the bar", side, f, worst)
    return got


# ---- rows that cannot be solved (tests/test_gpu_ials_edges.py; tests/test_ials_cpu.py shows that the float32 restatement fails
# exactly the same rows and meets the bar on every other) ---------------------------------------------------------------------
UNSOLVED_WIDTHS = (8, 100)
OVERFLOW_ALPHA = 3e38  # finite in float32; times an entry of 2.0 it is not


def _with_data(csr, data):
    return api.HostCSR(csr.indptr, csr.indices, data, csr.rows, csr.cols, csr.global_bias)


def _entries_apart(csr, n, seed):
    """n entry positions of distinct users and distinct items, none of item 1 (the messy set's hot item)."""
    rng = np.random.default_rng(seed)
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    picked = []
    for k in rng.permutation(csr.nnz):
        if csr.indices[k] != 1 and all(users[k] != users[j] and csr.indices[k] != csr.indices[j] for j in picked):
            picked.append(int(k))
            if len(picked) == n:
                return picked
    raise AssertionError("the set has no %d entries of distinct users and items" % n)


def rows_of_entries(csr, side, entries):
    """The rows of `side` (users or items) that hold the entry positions `entries` of the user-major CSR."""
    users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
    return np.unique((users if side == "users" else csr.indices)[np.asarray(entries, np.int64)])


def poison_entry_set():
    """(csr, entries): the messy set with one entry value NaN and one +inf, of different users and items."""
    if "poison-entry" not in _CACHE:
        csr = messy_set()
        entries = _entries_apart(csr, 2, 71)
        data = csr.data.copy()
        data[entries] = (np.nan, np.inf)
        _CACHE["poison-entry"] = (_with_data(csr, data), entries)
    return _CACHE["poison-entry"]


def overflow_set():
    """(csr, entries): the messy set's pattern with every value 0 but one of 2.0: at OVERFLOW_ALPHA every weight is exactly 0 (the
    system G0 + reg I against sum q, solved and judged) except that one, which is alpha r = +inf in float32."""
    if "overflow" not in _CACHE:
        csr = messy_set()
        entries = _entries_apart(csr, 1, 72)
        data = np.zeros_like(csr.data)
        data[entries] = 2.0
        _CACHE["overflow"] = (_with_data(csr, data), entries)
    return _CACHE["overflow"]


NEGATIVE_ALPHA, MILD, STRONG = 40.0, -0.002, -100.0


def negative_set():
    """(csr, entries): the messy set with every entry of ten users MILD (w = -0.08: with the partner's own q q^T in G0 the
    system stays above reg I, repeated pairs included) and three entries, of different users and items, STRONG (w = -4,000: an
    eigenvalue far below -10 reg, whatever else the row holds).  The rows that hold a STRONG entry cannot be factorised; every
    other row, on either side, is solved and judged."""
    if "negative" not in _CACHE:
        csr = messy_set()
        entries = _entries_apart(csr, 3, 73)
        users = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
        data = csr.data.copy()
        mild = np.setdiff1d(np.flatnonzero(np.diff(csr.indptr) > 0), users[entries])[3::14][:10]
        assert len(mild) == 10
        data[np.isin(users, mild)] = MILD
        data[entries] = STRONG
        _CACHE["negative"] = (_with_data(csr, data), entries)
    return _CACHE["negative"]


def unsolved_cases():
    """name -> (Case, rows of the case's side that cannot be solved): poison-entry, overflow and negative at f = 8 and 100 on
    both sides, from a state with model rows past the CSR."""
    if "unsolved" not in _CACHE:
        out = {}
        for kind, (csr, entries), alpha in (("poison-entry", poison_entry_set(), 40.0), ("overflow", overflow_set(), OVERFLOW_ALPHA),
                                            ("negative", negative_set(), NEGATIVE_ALPHA)):
            for f in UNSOLVED_WIDTHS:
                for side in ("users", "items"):
                    name = "%s-f%d-%s" % (kind, f, side)
                    out[name] = (Case(name, csr, side, f, alpha, HYPER, 6500 + f), rows_of_entries(csr, side, entries))
        _CACHE["unsolved"] = out
    return _CACHE["unsolved"]


def poisoned_partner(case, where):
    """(row, column) of the partner matrix of `case`: "inside" -- a partner row inside the CSR that no entry names (it still enters
    G0); "outside" -- a model row past the CSR's range (it does not)."""
    indices, n_part = ref.own_major(case.csr, case.side)[1::2]
    if where == "outside":
        return n_part + 1, 2
    unnamed = np.setdiff1d(np.arange(n_part), indices)
    assert len(unnamed) > 0
    return int(unnamed[len(unnamed) // 2]), 2


# ---- G0 over two workspace batches ----------------------------------------------------------------------------------------------
BIG_F, BIG_PARTNERS = 252, 455 * 1024 + 1  # 64 MiB / (36 tile pairs x 4 KiB) = 455 tiles of 1,024 partner rows fit one batch


def big_partner_case():
    """Five rows of 1, 5, 40, 1,024 and 2,049 entries drawn from all of 455 x 1,024 + 1 partners at f = 252: the second G0 batch
    is one tile of one row.  NT = 8 is the only tile count at which a second batch exists below 2^21 partner rows."""
    if "big" not in _CACHE:
        rng = np.random.default_rng(8)
        per_row = [np.sort(rng.choice(BIG_PARTNERS, n, replace=False)) for n in (1, 5, 40, 1024, 2049)]
        per_row[2][-1] = BIG_PARTNERS - 1  # the one row of the second batch is named as well
        _CACHE["big"] = Case("g0-two-batches-f252-users", chk.csr_from_rows(per_row, BIG_PARTNERS, rng), "users", BIG_F, 1.0, HYPER, 6600)
    return _CACHE["big"]


def big_partner_state():
    """The case's float32 state (0.5 GB of item factors), made once per process.  The partners some entry names are of O(0.3) as
    everywhere else, the other 460,000 of O(0.02): with all of them at 0.3, G0's diagonal (42,000) would dwarf every row's own
    sums and the regulariser, the optimum would be of O(1e-3) -- the size of the bar itself -- and no mistake outside G0 could
    show.  So G0 (about 470 on the diagonal, 280 of it from the named rows), the longest row's own Gram (about 500) and n reg
    (1,600) are of one order."""
    if "big-state" not in _CACHE:
        case = big_partner_case()
        P, Q, ub, ib = random_state(case.csr.rows + 3, case.csr.cols + 5, case.f, case.seed)
        named = np.zeros(len(Q), bool)
        named[case.csr.indices] = True
        named[BIG_PARTNERS - 1] = False  # the one row of the second batch is small like its neighbours
        Q[~named] *= np.float32(1 / 16)
        _CACHE["big-state"] = (P, Q, ub, ib)
    return _CACHE["big-state"]


# ---- the objective's grid-stride loops ---------------------------------------------------------------------------------------
def objective_loop_cases():
    """name -> Case at f = 8: OBJECTIVE_LOOP + 129 entries over 2,000 rows and 60 items (the entries loop takes a second trip), and
    OBJECTIVE_LOOP + 129 rows of one entry each over 50 items (the entries and the users loop do)."""
    if "loops" not in _CACHE:
        n = OBJECTIVE_LOOP + 129
        rng = np.random.default_rng(99)
        counts = rng.multinomial(n, np.ones(2000) / 2000)
        counts[[0, 1000, 1999]] = 0
        counts[5] += n - counts.sum()
        indptr = np.zeros(2001, np.int64)
        indptr[1:] = np.cumsum(counts)
        many_entries = api.HostCSR(indptr, rng.integers(0, 60, n), rng.integers(0, 11, n).astype(np.float32) / 2, 2000, 60, 0.0)
        many_rows = api.HostCSR(np.arange(n + 1), rng.integers(0, 50, n), rng.integers(0, 11, n).astype(np.float32) / 2, n, 50, 0.0)
        _CACHE["loops"] = {"objective-loop-entries": Case("objective-loop-entries", many_entries, "users", 8, 40.0, HYPER, 6701),
                           "objective-loop-rows": Case("objective-loop-rows", many_rows, "users", 8, 40.0, HYPER, 6702)}
    return _CACHE["loops"]
