"""TEST INFRASTRUCTURE shared by tests/test_softmax_cpu.py and tests/test_gpu_softmax.py: the sets the GPU tests judge (the CPU suite
runs the float32 restatement and every deliberate mistake over each of them, to show that they are fair and can tell), the ML_SMALL
experiment's settings and the figures the CPU suite measured for the GPU suite's tolerances.  Nothing here needs a GPU to be imported.

The sets are lmf_checks' own -- WIDTHS, OWN_ROWS, PARTNERS, ROW_LENGTHS through its entry_set() and cases(): the tile and step edges
of the same walk -- each as the user half-step of the set and as the item half-step of its transpose, and four more."""
import functools

import numpy as np

from cu2rec_amd import api

import lmf_checks
import softmax_reference64 as ref
from lmf_checks import GLOBAL_BIAS, HYPER, OBJECTIVE_SETS, OWN_ROWS, PARTNERS, ROW_LENGTHS, WIDTHS, Case, entry_set  # noqa: F401
from svd_checks import MARGIN

# Measured by tests/test_softmax_cpu.py (and asserted there): the float32 restatement's relative distance from the float64 objective
# on lmf_checks.OBJECTIVE_SETS.
OBJECTIVE_RESTATEMENT_ERROR = 2.0e-8  # measured: 5.34e-9, 4.05e-10, 1.98e-8, 1.06e-9

# The ML_SMALL experiment (tests/golden/ml_small_ratings.npz.xz, every user's last stored entry held out, the stored values taken
# as 1, the library's seed-42 start, k = 10, the training rows excluded).  hyper: lr, P_reg, Q_reg, user_bias_reg (not read),
# item_bias_reg.
ML_SMALL_F, ML_SMALL_SWEEPS, ML_SMALL_K = 64, 6, 10
ML_SMALL_HYPER = (0.15, 1.0, 1.0, 0.0, 1.0)
# float64: the held-out hits of 610 users; the float32 restatement's distances from the float64 run, measured and asserted by
# test_softmax_cpu.py: the relative objective distance at every half-step, the worst absolute factor distance after the last, the
# scores' distance relative to max |S|, and the users a run at MARGIN x that distance may decide differently
ML_SMALL_HITS = 31
ML_SMALL_OBJECTIVE_DISTANCE = 2.5e-8  # measured: 2.48e-8
ML_SMALL_FACTOR_DISTANCE = 1.7e-4  # measured: 1.65e-4
ML_SMALL_SCORE_DISTANCE = 2.5e-5  # measured: 2.43e-5
ML_SMALL_WITHIN_REACH = 0


def large_score_case(side):
    """Factors scaled so that the scores reach about +-200 (as lmf_checks.saturated_case): expf of a raw score overflows."""
    case = lmf_checks.saturated_case(side)
    case.name = "large-score-" + side
    return case


class _DominatedCase(Case):
    """One item's bias is 30 above the others': pi is 1 on it to the last bit and e^-30 elsewhere."""

    def state(self):
        P, Q, ub, ib = super().state()
        ib[5] += np.float32(30.0)
        return P, Q, ub, ib


def extra_cases():
    """name -> Case: the large scores on both sides, one item that dominates, and a set whose second user has no entries and whose
    last three columns are stored nowhere (cols larger than any stored item)."""
    out = {}
    for side in ("users", "items"):
        case = large_score_case(side)
        out[case.name] = case
    csr = entry_set(33, 129, 11)
    out["dominated"] = _DominatedCase("dominated", csr, "users", 31, 1.0, 9100)
    out["dominated-items"] = _DominatedCase("dominated-items", csr, "items", 31, 1.0, 9101)
    rng = np.random.default_rng(12)
    lengths = [5, 0, 3, 1, 0, 9, 2]
    idx = np.concatenate([rng.integers(0, 37, n) for n in lengths]).astype(np.int32)
    sparse = api.HostCSR(np.concatenate([[0], np.cumsum(lengths)]), idx, rng.integers(1, 11, len(idx)).astype(np.float32) / 2, 7, 40,
                         GLOBAL_BIAS)
    out["empty-user"] = Case("empty-user", sparse, "users", 8, 1.0, 9200)
    out["empty-user-items"] = Case("empty-user-items", sparse, "items", 8, 1.0, 9201)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: every set of lmf_checks.cases() (both sides; alpha is not read) and extra_cases()."""
    out = dict(lmf_checks.cases())
    out.update(extra_cases())
    return out


def claimed(case, mutation):
    """Whether `mutation` must show (ratio above 1) on `case`.  Not claimed where it is invisible:
    stored-items-only, no-W (W_u = 1) and W-entry-count need an entry (the latter two a row whose W is not 1 / not its count: the
    values are half stars, so any row of two or more entries has one); repeats-once needs a repeated pair; reg-times-n a row whose
    entry count is not 1; no-max-subtraction needs a score above 89, where expf overflows; no-bias-column changes the item side
    alone (the users have no bias gradient); lse-model-shape (the model has three items past the CSR's cols, lmf_checks.Case.state)
    needs those three to carry probability, which they do not beside an item 30 above them; drop-last-partner needs the last
    partner to carry some: on the user side an item that some user with entries gives a probability above 1e-3, on the item side a
    last user with entries (W_u = 0 removes a user from every item's sum: the transposed sets end in two such users);
    stored-items-only needs a second item; regs-swapped shows everywhere: P_reg, Q_reg and item_bias_reg differ."""
    csr = case.csr
    counts = np.diff(csr.indptr)
    if mutation == "stored-items-only":
        return csr.nnz > 0 and csr.cols > 1
    if mutation == "lse-model-shape":
        return not case.name.startswith("dominated")
    if mutation == "drop-last-partner":
        if case.side == "items":
            return counts[-1] > 0
        state = case.state()
        pi_last = np.exp(scores_of(tuple(a[:n] for a, n in zip(state, (csr.rows, csr.cols) * 2)), case.gb)[:, -1] - ref.lse(csr, state, case.gb))
        return bool((pi_last[counts > 0] > 1e-3).any())
    if mutation in ("no-W", "W-entry-count"):
        return csr.nnz > 0 and counts.max() > 1
    if mutation == "repeats-once":
        rows = np.repeat(np.arange(csr.rows), counts)
        return len(np.unique(rows.astype(np.int64) * (csr.cols + 1) + csr.indices)) < csr.nnz
    if mutation == "reg-times-n":
        own = counts if case.side == "users" else np.bincount(csr.indices, minlength=csr.cols)
        return bool((own != 1).any())
    if mutation == "no-max-subtraction":
        return case.name.startswith("large-score")
    if mutation == "no-bias-column":
        return case.side == "items"
    return True


def judge(case, state, got):
    """The worst ratio of a gradient (g, gb) to the derived bound."""
    g, gb = ref.gradient(case.csr, state, case.gb, case.hyper, case.side)
    b, bb = ref.bound(case.csr, state, case.gb, case.hyper, case.side)
    assert got[0].shape == g.shape and got[1].shape == gb.shape
    return max(ref.ratio(got[0], g, b), ref.bias_ratio(got[1], gb, bb))


def judge_lse(case, state, got):
    return ref.ratio(got, ref.lse(case.csr, state, case.gb), ref.lse_bound(case.csr, state, case.gb))


def judge_mass(case, state, got):
    return ref.ratio(got, np.ones(case.csr.rows), ref.mass_bound(case.csr, state, case.gb))


# ---- the ML_SMALL experiment -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ml_small():
    """(train with the stored values taken as 1, held)."""
    import knn_checks
    train, held = knn_checks.ml_small()
    ones = api.HostCSR(train.indptr, train.indices, np.ones(train.nnz, np.float32), train.rows, train.cols, train.global_bias)
    return ones, held


@functools.lru_cache(maxsize=None)
def ml_small_start():
    """The library's own seed-42 initial model (what cu.Model, train() and bin/mf start from), formed on the host."""
    import cu2rec_amd as cu
    tr, _ = ml_small()
    f = ML_SMALL_F
    return (cu.initialize_normal_array(tr.rows * f, f).reshape(tr.rows, f), cu.initialize_normal_array(tr.cols * f, f).reshape(tr.cols, f),
            cu.initialize_normal_array(tr.rows, f), cu.initialize_normal_array(tr.cols, f))


@functools.lru_cache(maxsize=None)
def ml_small_run64():
    """The float64 run, once per process -> (state, objectives after every half-step)."""
    tr, _ = ml_small()
    return ref.run(tr, ml_small_start(), tr.global_bias, ML_SMALL_HYPER, ML_SMALL_SWEEPS)


def scores_of(state, gb):
    P, Q, ub, ib = (np.asarray(a, np.float64) for a in state)
    return float(gb) + ub[:, None] + ib[None, :] + P @ Q.T


def hits_of(state):
    import knn_reference64 as kref
    import svd_checks
    tr, held = ml_small()
    return kref.hits_at(svd_checks.lists_of(scores_of(state, tr.global_bias), tr, ML_SMALL_K), held)


def within_reach(dist, margin=MARGIN):
    """The users whose hit a run at margin x dist from float64 may decide differently: the held-out item's score and the k-th best
    other candidate's differ by a nonzero amount of at most twice the scores' error, margin x dist x max |S| (as svd_checks has it)."""
    tr, held = ml_small()
    S = scores_of(ml_small_run64()[0], tr.global_bias)
    err = margin * dist * float(np.abs(S).max())
    reach = 0
    for u in range(tr.rows):
        target = int(held.indices[held.indptr[u]])
        others = np.ones(tr.cols, bool)
        others[tr.indices[tr.indptr[u]:tr.indptr[u + 1]]] = False
        others[target] = False
        others = np.flatnonzero(others)
        kth = others[np.lexsort((others, -S[u, others]))[ML_SMALL_K - 1]]
        reach += 0 < abs(S[u, target] - S[u, kth]) <= 2 * err
    return int(reach)
