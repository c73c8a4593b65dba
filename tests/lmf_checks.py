"""TEST INFRASTRUCTURE shared by tests/test_lmf_cpu.py and tests/test_gpu_lmf.py: the sets the GPU gradient tests judge (the CPU suite
runs the float32 restatement and every deliberate mistake over each of them, to show that they are fair and can tell), the fixture
run's settings and the figures the CPU suite measured for the GPU suite's tolerances.  Nothing here needs a GPU to be imported."""
import numpy as np

from cu2rec_amd import api

import lmf_reference64 as ref

# both edges of every T = ceil((f + 1) / 32) = 1 .. 8, and multiples of 4, where column f opens a float4 of its own
WIDTHS = [1, 8, 30, 31, 32, 63, 64, 100, 127, 128, 191, 192, 223, 224, 252]
OWN_ROWS = [1, 31, 32, 33, 65]
PARTNERS = [1, 31, 32, 33, 127, 128, 129, 257, 1000]  # tile edges and step edges of the 128-partner walk
ROW_LENGTHS = [300, 0, 1, 2, 7, 40]  # entries of own row r: ROW_LENGTHS[r % 6]
# (learning rate, P_reg, Q_reg, user_bias_reg, item_bias_reg): all four regularisers distinct, so that a swap shows
HYPER = (0.1, 0.6, 0.9, 0.25, 0.4)
GLOBAL_BIAS = -0.75

# Measured by tests/test_lmf_cpu.py (and asserted there): the float32 restatement's relative distance from the float64 objective.
OBJECTIVE_SETS = ("f8-33x1000", "f100-65x1000", "f252-65x31", "f31-33x129")
OBJECTIVE_RESTATEMENT_ERROR = 1.4e-9  # measured: 1.38e-9, 8.7e-10, 2.6e-10, 1.6e-10

# the fixture run (tests/golden/ml_small_ratings.npz.xz: 610 x 9,724, 100,836 entries)
FIXTURE_F, FIXTURE_ALPHA, FIXTURE_SWEEPS = 32, 2.0, 8
FIXTURE_HYPER = (0.2, 0.6, 0.6, 0.0, 0.0)
# the float32 restatement's distance from the float64 run, measured and asserted by test_lmf_cpu.py: relative objective distance at
# every half-step, and the worst absolute factor distance after the last
FIXTURE_OBJECTIVE_DISTANCE = 5.6e-8  # measured: 5.56e-8
FIXTURE_FACTOR_DISTANCE = 7.0e-7  # measured: 6.90e-7

_CACHE = {}


class Case:
    """One gradient: `csr` (user-major) is what the model is trained on, `side` the side whose gradient is judged -- every row of it."""

    def __init__(self, name, csr, side, f, alpha, seed, scale=0.3):
        self.name, self.csr, self.side, self.f, self.alpha, self.seed, self.scale = name, csr, side, f, alpha, seed, scale
        self.hyper, self.gb = HYPER, GLOBAL_BIAS

    def state(self):
        """float32 (P, Q, user_bias, item_bias), factors of O(scale) and biases of O(0.2), with model rows past the CSR on both sides."""
        rng = np.random.default_rng(self.seed)
        rows, cols, f = self.csr.rows + 2, self.csr.cols + 3, self.f
        return (rng.normal(0, self.scale, (rows, f)).astype(np.float32), rng.normal(0, self.scale, (cols, f)).astype(np.float32),
                rng.normal(0, 0.2, rows).astype(np.float32), rng.normal(0, 0.2, cols).astype(np.float32))


def entry_set(own, partners, seed):
    """own x partners, user-major: row r has ROW_LENGTHS[r % 6] entries drawn with repeats, unsorted, from the partners but the last
    two (cols is larger than any stored item), in half stars 0.5 .. 5."""
    key = (own, partners, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        top = max(1, partners - 2)
        per_row = [rng.integers(0, top, ROW_LENGTHS[r % len(ROW_LENGTHS)]) for r in range(own)]
        indptr = np.zeros(own + 1, np.int64)
        indptr[1:] = np.cumsum([len(p) for p in per_row])
        idx = np.concatenate(per_row).astype(np.int32)
        data = rng.integers(1, 11, len(idx)).astype(np.float32) / 2
        _CACHE[key] = api.HostCSR(indptr, idx, data, own, partners, GLOBAL_BIAS)
    return _CACHE[key]


def cases():
    """name -> Case: every width once (own rows and partner counts cycling through their lists), every partner count at f = 8 and every
    own-row count at f = 100, each as the user half-step of the set and as the item half-step of its transpose."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    shapes = [(f, OWN_ROWS[k % len(OWN_ROWS)], PARTNERS[(2 * k) % len(PARTNERS)]) for k, f in enumerate(WIDTHS)]
    shapes += [(8, 33, n) for n in PARTNERS] + [(100, n, 1000 if n == 65 else 129) for n in OWN_ROWS]
    out = {}
    for k, (f, own, partners) in enumerate(dict.fromkeys(shapes)):
        csr = entry_set(own, partners, 100 + k)
        alpha = 2.0 if k % 2 else 1.0
        name = "f%d-%dx%d" % (f, own, partners)
        out[name] = Case(name, csr, "users", f, alpha, 7000 + k)
        out[name + "-items"] = Case(name + "-items", csr.transpose(), "items", f, alpha, 7500 + k)
    _CACHE["cases"] = out
    return out


def saturated_case(side):
    """Partner rows scaled so that the scores reach about +-200: sigma is 0 or 1 to the last bit on most pairs."""
    csr = entry_set(33, 257, 9)
    case = Case("saturated-" + side, csr if side == "users" else csr.transpose(), side, 31, 1.0, 9000, scale=6.0)
    return case


def claimed(case, mutation):
    """Whether `mutation` must show (ratio above 1) on `case`.  Not claimed where it is invisible:
    repeats-once needs a repeated pair (a row of 300 draws has them whenever there are fewer than ~10,000 partners; rows of 1 entry
    alone have none) -- claimed where some own row holds a repeat; unobserved-only needs an entry; w-sigma likewise; reg-times-n needs
    a row whose entry count is not 1; drop-last-partner, no-bias-column, no-global-bias and regs-swapped show everywhere (the global
    bias is -0.75, the four regularisers differ)."""
    indptr, indices, _, _ = ref.own_major(case.csr, case.side)
    counts = np.diff(indptr)
    if mutation in ("unobserved-only", "w-sigma"):
        return counts.max() > 0
    if mutation == "repeats-once":
        rows = np.repeat(np.arange(len(counts)), counts)
        return len(np.unique(rows * (indices.max() + 2 if len(indices) else 1) + indices)) < len(indices)
    if mutation == "reg-times-n":
        return bool((counts != 1).any())
    return True


def fixture():
    """(csr, start state): the ML_SMALL fixture and the library's own seed-42 initial model (what cu.Model, train() and bin/mf start
    from), formed on the host."""
    if "fixture" not in _CACHE:
        from conftest import ml_small
        import cu2rec_amd as cu
        tr = cu.createSparseMatrix(ml_small())
        f = FIXTURE_F
        state = (cu.initialize_normal_array(tr.rows * f, f).reshape(tr.rows, f), cu.initialize_normal_array(tr.cols * f, f).reshape(tr.cols, f),
                 cu.initialize_normal_array(tr.rows, f), cu.initialize_normal_array(tr.cols, f))
        _CACHE["fixture"] = (tr, state)
    return _CACHE["fixture"]


def fixture_run64():
    """The float64 run on the fixture, once per process -> (state, objectives after every half-step)."""
    if "run64" not in _CACHE:
        tr, state = fixture()
        _CACHE["run64"] = ref.run(tr, state, tr.global_bias, FIXTURE_HYPER, FIXTURE_ALPHA, FIXTURE_SWEEPS)
    return _CACHE["run64"]
