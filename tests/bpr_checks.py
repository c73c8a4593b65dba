"""TEST INFRASTRUCTURE shared by tests/test_bpr_cpu.py and tests/test_gpu_bpr.py: the sets the GPU tests judge (the CPU suite runs the
float32 restatement and every deliberate mistake over each of them, to show that they are fair and can tell), the fixture run's
settings and the figures the CPU suite measured for the GPU suite's tolerances.  Nothing here needs a GPU to be imported."""
import numpy as np

from cu2rec_amd import api

import bpr_reference64 as ref

# both edges of every E = ceil((f + 1) / 64) = 1 .. 4, and multiples of 4, where column f opens a float4 of its own
WIDTHS = [1, 3, 4, 62, 63, 64, 100, 126, 127, 128, 190, 191, 192, 252]
ROW_LENGTHS = [300, 0, 1, 2, 3, 4, 5, 7, 40]  # entries of row r: ROW_LENGTHS[r % 9]
SEEDS = (42, (1 << 40) + 7)  # the second fills the seed's high word
SWEEPS = (0, 1, ref.MAX_SWEEP - 1)
# (learning rate, P_reg, Q_reg, user_bias_reg, item_bias_reg): the regularisers distinct, so that a swap shows
HYPER = (0.1, 0.6, 0.9, 0.25, 0.4)
GRADIENT_SEED, GRADIENT_SWEEP = 42, 1

# Measured by tests/test_bpr_cpu.py (and asserted there).  The float32 restatement's worst fraction of the gradient bound over
# every case, and the least fraction any claimed mistake reaches:
RESTATEMENT_WORST = 0.25  # measured: 0.242 (f = 1, items of 65 x 1000)
MUTATION_LEAST = 30.0  # measured: 31.2
# The objective is evaluated in double on the device; its restatement in the device's order (ref.objective_blocked) is off the
# numpy value by at most a few 2^-53, where one differently rounded exp or log1p decides the figure, so the recorded distance is
# floored at what the arithmetic itself allows: every term of L has one sign, and a term is a score, an exponential, a log1p and
# two additions of a relative error of at most 2^-53 each -- 8 x 2^-53 with the sum's own roundings.
OBJECTIVE_SETS = ("f3-65x1000", "f100-65x1000", "f252-33x40", "f64-17x257")
OBJECTIVE_RESTATEMENT_ERROR = 8 * 2.0 ** -53  # measured: below it on every set

# the fixture run (tests/golden/ml_small_ratings.npz.xz: 610 x 9,724, 100,836 entries; every user's last entry held out)
FIXTURE_F, FIXTURE_SEED, FIXTURE_SWEEPS = 32, 42, 6
FIXTURE_HYPER = (0.05, 0.01, 0.01, 0.0, 0.01)
# The float64 reference's run at these settings (tests/test_bpr_cpu.py repeats it and asserts every figure): the objective, the
# triples and the triples with x_e > 0 after each of the 12 half-steps, over that sweep's triples; the sampled AUC ends at 0.9049
# (untrained: 0.4955) and the hit rate @10 of the held-out entries at 8 users of 610 (untrained: none; the held-out entry is the
# user's highest item id, rarely a popular one).  No entry goes without a triple: a user stores 2,697 of 9,724 items at the most.
# The float32 restatement's distances from that run: the objective's relative one at every half-step, the worst factor's at the end,
# the worst score's on the last sweep's triples.  auc_flips / hit_flips: the triples with |x_e| within 8 x that score distance of 0,
# and the users whose held-out score is within 16 x of the tenth best: what a run as close to float64 as the GPU test demands of
# the objectives (8 x the restatement's distance) could order differently -- the GPU test's margins on the two ranking figures.
FIXTURE_REFERENCE = {
    "objectives": [-69317.350407, -64449.825289, -63281.217425, -57088.208316, -53586.086209, -47482.736376, -44358.488513,
                   -39795.661368, -38096.087995, -34985.561725, -34241.776211, -31939.646286],
    "triples": [100226] * 12,
    "ordered": [52980, 89162, 87371, 90766, 89360, 90717, 89540, 90809, 89616, 90689, 89690, 90698],
    "hit_rate": 8 / 610,
    "objective_distance": 2.3e-9,  # measured: 2.23e-9
    "factor_distance": 1.6e-6,  # measured: 1.54e-6
    "score_distance": 3.2e-7,  # measured: 3.12e-7
    "auc_flips": 0,
    "hit_flips": 0,
}

_CACHE = {}


class Case:
    """One gradient: `csr` (user-major) is what the model is trained on, `side` the side whose gradient is judged -- every row of it."""

    def __init__(self, name, csr, side, f, seed, scale=0.3):
        self.name, self.csr, self.side, self.f, self.seed, self.scale = name, csr, side, f, seed, scale
        self.hyper = HYPER

    def state(self):
        """float32 (P, Q, user_bias, item_bias), factors of O(scale) and biases of O(0.2), with model rows past the CSR on both sides."""
        rng = np.random.default_rng(self.seed)
        rows, cols, f = self.csr.rows + 2, self.csr.cols + 3, self.f
        return (rng.normal(0, self.scale, (rows, f)).astype(np.float32), rng.normal(0, self.scale, (cols, f)).astype(np.float32),
                rng.normal(0, 0.2, rows).astype(np.float32), rng.normal(0, 0.2, cols).astype(np.float32))

    def negatives(self):
        return ref.negatives(self.csr, GRADIENT_SEED, GRADIENT_SWEEP)


def _csr(per_row, cols):
    indptr = np.zeros(len(per_row) + 1, np.int64)
    indptr[1:] = np.cumsum([len(p) for p in per_row])
    idx = np.concatenate(per_row).astype(np.int32) if per_row else np.zeros(0, np.int32)
    return api.HostCSR(indptr, idx, np.ones(len(idx), np.float32), len(per_row), cols, 0.0)


def entry_set(rows, cols, seed, full_rows=False):
    """rows x cols, user-major: row r has ROW_LENGTHS[r % 9] entries drawn with repeats, unsorted, from the columns but the last two
    (cols is larger than any stored item).  full_rows: row 0 instead stores EVERY column (shuffled, a quarter of them twice) and row
    1 every column but number 17."""
    key = (rows, cols, seed, full_rows)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        top = max(1, cols - 2)
        per_row = [rng.integers(0, top, ROW_LENGTHS[r % len(ROW_LENGTHS)]) for r in range(rows)]
        if full_rows:
            every = np.concatenate([np.arange(cols), rng.integers(0, cols, cols // 4)])
            per_row[0] = rng.permutation(every)
            per_row[1] = rng.permutation(every[every != 17])
        _CACHE[key] = _csr(per_row, cols)
    return _CACHE[key]


def negative_sets():
    """name -> csr for the exact-equality test of the negatives: the row lengths of ROW_LENGTHS, unsorted rows with repeats, cols
    past every stored item, a row that stores every column and one that stores all but one, and cols == 1."""
    return {"65x1000": entry_set(65, 1000, 11), "33x40": entry_set(33, 40, 12, full_rows=True), "17x257": entry_set(17, 257, 13),
            "5x1": _csr([np.zeros(3, int), np.zeros(0, int), np.zeros(1, int), np.zeros(2, int), np.zeros(1, int)], 1)}


def cases():
    """name -> Case: every width on one of three sets in turn, each as the user half-step and as the item half-step."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    sets = [("65x1000", entry_set(65, 1000, 11)), ("33x40", entry_set(33, 40, 12, full_rows=True)), ("17x257", entry_set(17, 257, 13))]
    out = {}
    for k, f in enumerate(WIDTHS + [3]):  # the extra one, f = 3 on the largest set, completes OBJECTIVE_SETS
        label, csr = sets[k % 3] if k < len(WIDTHS) else sets[0]
        for side in ("users", "items"):
            name = "f%d-%s%s" % (f, label, "" if side == "users" else "-items")
            out.setdefault(name, Case(name, csr, side, f, 7000 + k))
    _CACHE["cases"] = out
    return out


def saturated_case(side):
    """Factors scaled so that x_e reaches about +-200: sigma is 0 or 1 to the last bit on most triples."""
    return Case("saturated-" + side, entry_set(33, 257, 9), side, 31, 9000, scale=6.0)


def claimed(case, mutation):
    """Whether `mutation` must show (ratio above 1) on `case`.  Not claimed where it is invisible: the two mistakes in the draw need an
    entry whose negative they change; sigma-x and no-item-bias a triple; neg-dropped and neg-sign a triple and the item side;
    drop-last-entry a triple among the own rows' last entries; repeats-once a repeated pair with a triple; reg-times-n an own row
    whose entry count is not 1; regs-swapped shows everywhere (P_reg and Q_reg differ)."""
    csr, neg = case.csr, case.negatives()
    on = neg >= 0
    if mutation in ref.NEGATIVE_MUTATIONS:
        return bool((ref.negatives(csr, GRADIENT_SEED, GRADIENT_SWEEP, mutation) != neg).any())
    if mutation in ("sigma-x", "no-item-bias"):
        return bool(on.any())
    if mutation in ("neg-dropped", "neg-sign"):
        return case.side == "items" and bool(on.any())
    if mutation == "drop-last-entry":
        return bool(on[ref._last_of_own_rows(csr, case.side)].any())
    if mutation == "repeats-once":
        rows = np.repeat(np.arange(csr.rows), np.diff(csr.indptr))
        _, first = np.unique(rows * (csr.cols + 1) + csr.indices, return_index=True)
        keep = np.zeros(csr.nnz, bool)
        keep[first] = True
        return bool((on & ~keep).any())
    if mutation == "reg-times-n":
        counts = np.diff(csr.indptr) if case.side == "users" else np.bincount(csr.indices, minlength=csr.cols)
        return bool((counts != 1).any())
    return True


def hold_out_last(tr):
    """(train, held): every user's last entry moved out of `tr` into its own one-entry-per-user CSR."""
    last = tr.indptr[1:] - 1
    keep = np.ones(tr.nnz, bool)
    keep[last] = False
    indptr = np.concatenate([[0], np.cumsum(np.diff(tr.indptr) - 1)])
    train = api.HostCSR(indptr, tr.indices[keep], tr.data[keep], tr.rows, tr.cols, tr.global_bias)
    held = api.HostCSR(np.arange(tr.rows + 1), tr.indices[last], tr.data[last], tr.rows, tr.cols, tr.global_bias)
    return train, held


def fixture():
    """(train, held, start state): the ML_SMALL fixture with every user's last entry held out, and the library's own seed-42 initial
    model (what cu.Model, train() and bin/mf start from), formed on the host."""
    if "fixture" not in _CACHE:
        from conftest import ml_small
        import cu2rec_amd as cu
        train, held = hold_out_last(cu.createSparseMatrix(ml_small()))
        f = FIXTURE_F
        state = (cu.initialize_normal_array(train.rows * f, f).reshape(train.rows, f),
                 cu.initialize_normal_array(train.cols * f, f).reshape(train.cols, f),
                 cu.initialize_normal_array(train.rows, f), cu.initialize_normal_array(train.cols, f))
        _CACHE["fixture"] = (train, held, state)
    return _CACHE["fixture"]


def hit_rate_at_10(train, held, state, margin=0.0):
    """(hit rate @10 of the held-out entries among every user's items outside `train`, in float64 scores; the number of users whose
    held-out item is within `margin` of the tenth or eleventh best score: the hits a score perturbation of margin / 2 could flip).
    The user bias and the global bias do not order a user's items."""
    P, Q, _, ib = (np.asarray(a, np.float64) for a in state)
    hits = close = 0
    for u in range(train.rows):
        s = ib[:train.cols] + Q[:train.cols] @ P[u]
        target = int(held.indices[held.indptr[u]])
        mine = s[target]
        s[train.indices[train.indptr[u]:train.indptr[u + 1]]] = -np.inf
        s[target] = -np.inf
        top = np.sort(s)[-10:]  # the ten best of the others: the target is listed iff it beats the tenth
        hits += mine > top[0]
        close += abs(mine - top[0]) <= margin
    return hits / train.rows, close


def fixture_run64():
    """The float64 run on the fixture, once per process -> (state, [(L, triples, ordered)] after every half-step)."""
    if "run64" not in _CACHE:
        train, _, state = fixture()
        _CACHE["run64"] = ref.run(train, state, FIXTURE_HYPER, FIXTURE_SEED, FIXTURE_SWEEPS)
    return _CACHE["run64"]
