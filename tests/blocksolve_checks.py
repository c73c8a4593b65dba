"""TEST INFRASTRUCTURE shared by tests/test_gpu_blocksolve_grid.py and tests/test_blocksolve_checks_cpu.py: the cases of the block-solve
grid (every row width x pinned chain lengths), their rating sets and starting models, the two CPU references and the bound a GPU
result is held to.  Nothing here needs a GPU to be imported.

What decides the mode's code path, restated below from cu2rec_amd/csrc/blocksolve.hip and its phase headers (blocksolve_*.hpp):
  * the row width nslots = ceil(f / 4) float4 slots: launch_solve's seven phase-2 instantiations SW (sw_bucket), bs_solve_kernel's
    five look-ahead instantiations NSM (nsm_bucket, rows of at most kLaMaxSlots = 29 slots), launch_update's one to four phase-3
    wavefronts, the odd LDS row stride nslots | 1;
  * the chain length: blocks of kB = 64 links in two halves of 32; solve_chain's (blocksolve_solve.hpp) long_chain path above
    kDepth = 4 blocks with n_intervals rounded up to a multiple of 4; chain_lookahead (blocksolve_lookahead.hpp) from two blocks on
    (chain_is_lookahead), rings of 3 / 2 / 2.
Chain lengths are made EXACT instead of sampled: a user with one rating samples it in every iteration, so an item rated by L such users
has a chain of exactly L links (users ascending) in every iteration, and its expected update rate is exactly L.

The starting model is not the library's initialisation, whose entries shrink with f (max |Q| = 0.0175 at f = 252: a float4 slot
dropped from a dot product moves most parameters by less than any bound worth stating) but uniform values of +-min(0.5, 2 / sqrt(f)),
biases +-0.3; tests/test_blocksolve_checks_cpu.py shows that a slot or a link lost on these values moves the float64 result by at
least ten times the largest bound used here.

The bound of a case: tol = max(2e-6, 4 d_orc), d_orc being the float32 oracle's own largest distance from the float64 walk
(tests/sgd_reference64.py) on that case -- measured from the two references, never from a kernel; 2e-6 is the suite's bound for the
mode everywhere else, the factor 4 allows for its re-associated sums, and tol may not exceed TOL_CAP = 1e-5 (asserted: a loose
reference must not hide a failure).  Measured on the length set: d_orc = 1.9e-7 .. 1.06e-6 over the 63 widths
(the largest at f = 54), so tol is 2e-6 .. 4.2e-6."""
import numpy as np

import cu2rec_amd as cu
from cu2rec_amd import api
from oracle import oracle as orc

from sgd_reference64 import State64, sgd64

LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 511, 512, 513, 769]
HYPER = (0.05, 0.02, 0.03, 0.04, 0.05)  # lr, P_reg, Q_reg, user_bias_reg, item_bias_reg: all distinct
SEED = 42
ITERS = 2
TOL_FLOOR, TOL_CAP = 2e-6, 1e-5
NAMES = ("P", "Q", "user_bias", "item_bias")

NSLOTS = list(range(1, 64))
LA_MAX_SLOTS = 29  # blocksolve_lookahead.hpp, kLaMaxSlots / la_supported


def width(nslots):
    """The f of a row of nslots float4 slots: every f mod 4 in turn (3, 2, 1, 0, 3, ...), and ceil(f / 4) = nslots."""
    return 4 * nslots - (nslots % 4)


def sw_bucket(nslots):
    """blocksolve.hip, launch_solve: sw = ceil(nslots / 4) slots per quarter-owner picks bs_solve_kernel<SW>, the first SW >= sw."""
    if not 1 <= nslots <= 63:  # (BlockSolve::begin, kBsMaxSlots)
        raise ValueError("block-solve mode is compiled for n_factors <= 252")
    sw = (nslots + 3) // 4
    return next(SW for SW in (1, 2, 4, 7, 8, 12, 16) if sw <= SW)


def nsm_bucket(nslots):
    """blocksolve.hip, bs_solve_kernel: chain_lookahead<min(4 SW, kLaMaxSlots)>, taken only for SW <= 8 and (la_supported,
    blocksolve_lookahead.hpp, read in BlockSolve::begin) nslots <= kLaMaxSlots."""
    assert 1 <= nslots <= LA_MAX_SLOTS
    return min(4 * sw_bucket(nslots), LA_MAX_SLOTS)


def update_waves(nslots):
    """blocksolve.hip, launch_update: wavefronts of a phase-3 workgroup, one per 64 columns of the 4 nslots."""
    return (4 * nslots + 63) // 64


SW_VALUES = (1, 2, 4, 7, 8, 12, 16)
# the first and the last width of every SW bucket: at the first, 4 SW exceeds nslots by the most (three quarter-owners partly idle)
BUCKET_EDGES = sorted({min(n for n in NSLOTS if sw_bucket(n) == SW) for SW in SW_VALUES} |
                      {max(n for n in NSLOTS if sw_bucket(n) == SW) for SW in SW_VALUES})
ONE_PER_BUCKET = [2, 6, 12, 23, 31, 41, 57]  # one width inside each SW bucket, every f mod 4 among them

assert all((width(n) + 3) // 4 == n for n in NSLOTS) and {width(n) % 4 for n in NSLOTS} == {0, 1, 2, 3}
assert {sw_bucket(n) for n in NSLOTS} == set(SW_VALUES)
assert {nsm_bucket(n) for n in NSLOTS if n <= LA_MAX_SLOTS} == {4, 8, 16, 28, 29}
assert {update_waves(n) for n in NSLOTS} == {1, 2, 3, 4}
assert BUCKET_EDGES == [1, 4, 5, 8, 9, 16, 17, 28, 29, 32, 33, 48, 49, 63]
assert [sw_bucket(n) for n in ONE_PER_BUCKET] == list(SW_VALUES) and {width(n) % 4 for n in ONE_PER_BUCKET} == {0, 1, 2, 3}

_CACHE = {}


# ---- rating sets -----------------------------------------------------------------------------------------------------------
def _half_stars(rng, n):
    return rng.integers(1, 11, n).astype(np.float32) / 2  # 0.5 .. 5.0


def length_set():
    """19 items, item j rated by LENGTHS[j] users of one rating each (4,068 users), users dealt to items by a seeded permutation so
    that a chain's rows are scattered over P.  19 is no power of two: ordered.hip's rank clamp does not bind."""
    if "lengths" not in _CACHE:
        rng = np.random.default_rng(1964)
        n = sum(LENGTHS)
        item_of_user = np.repeat(np.arange(len(LENGTHS)), LENGTHS)[rng.permutation(n)]
        data = _half_stars(rng, n)
        _CACHE["lengths"] = api.HostCSR(np.arange(n + 1), item_of_user, data, n, len(LENGTHS), float(data.mean(dtype=np.float64)))
    return _CACHE["lengths"]


# the varying set: items rated ONLY by users of two ratings, each of whom shares it with an item nobody else rates.  Such an item's
# rate is half its raters -- hot at VARYING_MIN_RATE -- while its realised chain is Binomial(raters, 1/2): empty in some iterations for
# the small ones, one block in some iterations and two in others for the one of 132 raters (rate 66: a look-ahead rank from one
# block on).  The partner items have rate exactly 0.5 each: below VARYING_MIN_RATE they stay with the walk.
VARYING_RATERS = [2, 2, 3, 5, 132]
VARYING_MIN_RATE = 1.0
VARYING_ITERS = 6


def varying_set():
    """length_set() plus the VARYING_RATERS items (ids 19 ...) and their raters' partner items (behind them), the two-rating users
    appended behind the 4,068.  -> (HostCSR, ids of the added hot items)"""
    if "varying" not in _CACHE:
        base = length_set()
        rng = np.random.default_rng(7)
        n_extra = sum(VARYING_RATERS)
        first = len(LENGTHS)
        hot = np.arange(first, first + len(VARYING_RATERS))
        hot_of_user = np.repeat(hot, VARYING_RATERS)[rng.permutation(n_extra)]
        partner = first + len(VARYING_RATERS) + np.arange(n_extra)
        indices = np.concatenate([base.indices, np.stack([hot_of_user, partner], axis=1).reshape(-1)])  # ascending in every row
        data = np.concatenate([base.data, _half_stars(rng, 2 * n_extra)])
        indptr = np.concatenate([base.indptr, base.indptr[-1] + 2 * np.arange(1, n_extra + 1)])
        cols = int(partner[-1]) + 1
        _CACHE["varying"] = (api.HostCSR(indptr, indices, data, base.rows + n_extra, cols, float(data.mean(dtype=np.float64))), hot)
    return _CACHE["varying"]


def realised_chains(csr, seed, iteration):
    """How many links every item's chain has in `iteration`: the product's sample stream (cu2rec_sampler_index) replayed."""
    counts = np.zeros(csr.cols, np.int64)
    for x in range(csr.rows):
        lo, hi = int(csr.indptr[x]), int(csr.indptr[x + 1])
        if lo < hi:
            counts[csr.indices[api.sampler_index(seed, x, iteration, lo, hi)]] += 1
    return counts


def as_orc(m):
    return orc.CSR(m.indptr, m.indices, m.data, m.rows, m.cols, m.global_bias)


# ---- the starting model ----------------------------------------------------------------------------------------------------
def start_model(rows, cols, f, seed=0):
    """float32 P, Q uniform in +-min(0.5, 2 / sqrt(f)), biases uniform in +-0.3."""
    rng = np.random.default_rng(1000 * f + seed)
    s = min(0.5, 2.0 / np.sqrt(f))
    return (rng.uniform(-s, s, (rows, f)).astype(np.float32), rng.uniform(-s, s, (cols, f)).astype(np.float32),
            rng.uniform(-0.3, 0.3, rows).astype(np.float32), rng.uniform(-0.3, 0.3, cols).astype(np.float32))


# ---- the references ---------------------------------------------------------------------------------------------------------
class Reference:
    """After one call: the float64 walk's arrays, the oracle's float32 arrays, the oracle's distance from the walk, the bound."""

    def __init__(self, want, oracle):
        self.want, self.oracle = want, oracle
        self.d_orc = max(float(np.abs(o.astype(np.float64) - w).max()) for o, w in zip(oracle, want))
        self.tol = max(TOL_FLOOR, 4.0 * self.d_orc)


LENGTH_CALLS = ((0, ITERS, True),)
FROZEN_THEN_RESUMED = ((0, ITERS, False), (2, ITERS, True))


def references(name, csr, f, calls=LENGTH_CALLS, hyper=HYPER, seed=SEED):
    """The calls (iter0, n_iters, update_items) one after the other from start_model(), in the float64 walk (sgd64, bound=False) and
    in the float32 oracle (DOT_TREE16, the kernels' own dot order) beside it -> (the starting state, one Reference per call).
    Computed once per (set, width, calls) and shared by every phase-2 form; the arrays are not to be written to."""
    key = ("ref", name, f, calls, hyper, seed)
    if key not in _CACHE:
        start = start_model(csr.rows, csr.cols, f)
        st = State64(*start)
        state = [a.copy() for a in start]
        out = []
        for iter0, n, update_items in calls:
            sgd64(csr, st, csr.global_bias, hyper, seed, iter0, n, update_items=update_items, bound=False)
            orc.sgd_iterations(as_orc(csr), *state, csr.global_bias, hyper, seed, iter0, n, dot_order=orc.DOT_TREE16,
                               update_items=update_items)
            assert all(np.isfinite(a).all() for a in state), "the oracle itself is not finite"
            out.append(Reference([a.copy() for a in st.arrays()], [a.copy() for a in state]))
        _CACHE[key] = (start, out)
    return _CACHE[key]


# ---- judging a result -------------------------------------------------------------------------------------------------------
def raters_of(csr):
    key = ("raters", id(csr))
    if key not in _CACHE:
        t = csr.transpose()
        _CACHE[key] = (csr, [t.indices[t.indptr[j]:t.indptr[j + 1]] for j in range(csr.cols)])  # (csr kept: its id stays its own)
    return _CACHE[key][1]


def per_item(got, want, csr):
    """Largest |got - want| of every item's chain, per array: {array name: one value per item} -- P and user_bias over the item's raters,
    Q and item_bias its own row.  A seam bug then reads as "length 257, Q"."""
    dP = np.abs(got[0].astype(np.float64) - want[0]).max(axis=1) if got[0].shape[1] else np.zeros(csr.rows)
    dQ = np.abs(got[1].astype(np.float64) - want[1]).max(axis=1)
    dub, dib = np.abs(got[2].astype(np.float64) - want[2]), np.abs(got[3].astype(np.float64) - want[3])
    raters = raters_of(csr)
    out = {"P": np.zeros(csr.cols), "Q": dQ, "user_bias": np.zeros(csr.cols), "item_bias": dib}
    for j, users in enumerate(raters):
        if len(users):
            out["P"][j], out["user_bias"][j] = dP[users].max(), dub[users].max()
    return out


def distance(got, want):
    return max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want))


def assert_within(got, ref, csr, what):
    """Every parameter within ref.tol of the float64 walk (and tol itself under TOL_CAP); on failure the items beyond it are named
    with their number of raters and the arrays that are off.  -> the largest distance."""
    assert ref.tol <= TOL_CAP, ("the oracle is too far from the float64 walk for this case to judge anything", what, ref.d_orc)
    assert all(np.isfinite(g).all() for g in got), ("block-solve result is not finite", what)
    worst = distance(got, ref.want)
    if worst > ref.tol:
        items = per_item(got, ref.want, csr)
        raters = raters_of(csr)
        lines = ["length %d (item %d): %s" % (len(raters[j]), j, ", ".join("%s %.2e" % (n, items[n][j]) for n in NAMES if items[n][j] > ref.tol))
                 for j in range(csr.cols) if any(items[n][j] > ref.tol for n in NAMES)]
        raise AssertionError("%s: %.3e from the float64 walk, bound %.3e (oracle: %.3e)\n  %s" % (what, worst, ref.tol, ref.d_orc, "\n  ".join(lines[:40])))
    return worst


def model_from(csr, f, state):
    return cu.Model(csr.rows, csr.cols, f, csr.global_bias, *state)
