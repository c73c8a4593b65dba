"""The block-solve grid's cases are fair (CPU): what tests/test_gpu_blocksolve_grid.py takes for granted about the sets, the references
and the bound of tests/blocksolve_checks.py, shown without a GPU.
  * the chain lengths are exact: cu2rec_item_update_rates gives LENGTHS, and the sample stream replayed gives every item exactly that
    many links in both iterations; the varying set has a hot item whose chain is empty in some iteration and one that has one block in
    some iterations and two in others;
  * the bound stays under its cap at the first and last width of every phase-2 bucket (4 d_orc <= 1e-5; measured over all 63 widths:
    d_orc = 1.9e-7 .. 1.06e-6);
  * the comparison can see a subtle error: with the last float4 slot of ONE mid-chain user's starting row zeroed, or with one link
    dropped, one iteration of the float64 walk moves some parameter by at least ten times the cap, at every one of those widths, on
    the chains of 65 and of 769 links.  The zeroed entries themselves and the dropped user's own row and bias are left out: what counts
    is what the rest of the chain sees.  Measured: at least 2.5e-3 for the slot (f = 195, 769 links: 255 times the cap), at least
    5.4e-3 for the link (f = 19, 769 links)."""
import numpy as np
import pytest

from cu2rec_amd import api

import blocksolve_checks as bc
from sgd_reference64 import State64, sgd64


def test_widths_reach_every_phase2_and_lookahead_instantiation():
    assert len(bc.NSLOTS) == 63 and [(bc.width(n) + 3) // 4 for n in bc.NSLOTS] == bc.NSLOTS
    assert [bc.width(n) % 4 for n in bc.NSLOTS[:4]] == [3, 2, 1, 0]
    assert {bc.sw_bucket(n) for n in bc.NSLOTS} == {1, 2, 4, 7, 8, 12, 16}
    assert {bc.nsm_bucket(n) for n in range(1, 30)} == {4, 8, 16, 28, 29}
    # the table of the seven buckets, both ends of each
    assert [(bc.sw_bucket(n), n) for n in bc.BUCKET_EDGES] == [(1, 1), (1, 4), (2, 5), (2, 8), (4, 9), (4, 16), (7, 17), (7, 28), (8, 29),
                                                              (8, 32), (12, 33), (12, 48), (16, 49), (16, 63)]
    with pytest.raises(ValueError):
        bc.sw_bucket(64)


def test_chain_lengths_are_exact():
    tr = bc.length_set()
    assert tr.rows == sum(bc.LENGTHS) == 4068 and tr.cols == 19 and tr.nnz == tr.rows
    assert set(np.unique(tr.data)) <= {k / 2 for k in range(1, 11)}
    rate = api.item_update_rates(tr)
    assert rate.tolist() == [float(n) for n in bc.LENGTHS]
    for it in range(bc.ITERS):
        assert bc.realised_chains(tr, bc.SEED, it).tolist() == bc.LENGTHS
    # a chain's rows are scattered in P: no item's users are one run of consecutive ids
    for users in bc.raters_of(tr):
        assert len(users) < 3 or users[-1] - users[0] > len(users) - 1


def test_varying_set_has_an_empty_hot_chain_and_one_that_crosses_a_block():
    va, hot = bc.varying_set()
    rate = api.item_update_rates(va)
    assert rate[:19].tolist() == [float(n) for n in bc.LENGTHS]
    assert rate[hot].tolist() == [n / 2 for n in bc.VARYING_RATERS] and (rate[hot] >= bc.VARYING_MIN_RATE).all()
    assert (rate[hot[-1] + 1:] == 0.5).all() and 0.5 < bc.VARYING_MIN_RATE  # the partner items are walked
    chains = np.array([bc.realised_chains(va, bc.SEED, it) for it in range(bc.VARYING_ITERS)])
    assert (chains[:, :19] == bc.LENGTHS).all()
    assert (chains[:, hot] == 0).any(), chains[:, hot]
    assert any(chains[:, j].min() <= 64 < chains[:, j].max() for j in hot), chains[:, hot]


@pytest.mark.parametrize("nslots", bc.BUCKET_EDGES)
def test_oracle_distance_keeps_the_bound_under_its_cap(nslots):
    tr = bc.length_set()
    _, (ref,) = bc.references("lengths", tr, bc.width(nslots))
    assert 4.0 * ref.d_orc <= bc.TOL_CAP, ref.d_orc
    assert bc.TOL_FLOOR <= ref.tol <= bc.TOL_CAP


def _two_chains(tr, items):
    """The set with only the users of `items` keeping their rating.  Every user rates one item, so the chains are independent: on these
    items one iteration is exactly the full set's, and every other parameter stays what it was in both runs."""
    keep = np.isin(tr.indices, items)
    indptr = np.zeros(tr.rows + 1, np.int64)
    np.cumsum(keep, out=indptr[1:])
    return api.HostCSR(indptr, tr.indices[keep], tr.data[keep], tr.rows, tr.cols, tr.global_bias)


def _one_iteration(csr, start):
    return sgd64(csr, State64(*start), csr.global_bias, bc.HYPER, bc.SEED, 0, 1, bound=False).arrays()


@pytest.mark.parametrize("nslots", bc.BUCKET_EDGES)
def test_a_lost_slot_or_a_lost_link_moves_the_float64_walk_by_ten_times_the_cap(nslots):
    tr = bc.length_set()
    f = bc.width(nslots)
    items = [bc.LENGTHS.index(65), bc.LENGTHS.index(769)]
    sub = _two_chains(tr, items)
    start = bc.start_model(tr.rows, tr.cols, f)
    base = _one_iteration(sub, start)
    for j in items:
        users = bc.raters_of(tr)[j]
        x = int(users[len(users) // 2])  # mid-chain: half of the links come behind it
        # the last float4 slot of that user's row, as a kernel that skipped it would see the row
        P = start[0].copy()
        P[x, 4 * (nslots - 1):] = 0.0
        got = _one_iteration(sub, (P,) + tuple(start[1:]))
        moved = [np.abs(g - b) for g, b in zip(got, base)]
        moved[0][x, 4 * (nslots - 1):] = 0.0  # (those entries differ by what was taken from them)
        moved = max(float(m.max()) for m in moved)
        print("f=%d, %d links: a lost slot moves the walk by %.2e" % (f, bc.LENGTHS[j], moved))
        assert moved >= 10 * bc.TOL_CAP, ("a lost slot is not visible", f, bc.LENGTHS[j], moved)
        # the link dropped: the user's row emptied.  Judged on what the REST of the chain sees of it (the user's own row and bias aside)
        indptr = sub.indptr.copy()
        indptr[x + 1:] -= 1
        k = int(sub.indptr[x])
        cut = api.HostCSR(indptr, np.delete(sub.indices, k), np.delete(sub.data, k), sub.rows, sub.cols, sub.global_bias)
        got = _one_iteration(cut, start)
        others = np.arange(tr.rows) != x
        moved = max(float(np.abs(got[0][others] - base[0][others]).max()), float(np.abs(got[1] - base[1]).max()),
                    float(np.abs(got[2][others] - base[2][others]).max()), float(np.abs(got[3] - base[3]).max()))
        print("f=%d, %d links: a lost link moves the rest of the chain by %.2e" % (f, bc.LENGTHS[j], moved))
        assert moved >= 10 * bc.TOL_CAP, ("a lost link is not visible", f, bc.LENGTHS[j], moved)
