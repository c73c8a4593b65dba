"""The algebra phase 1 of the block-solve mode relies on (cu2rec_amd/csrc/blocksolve_gram.hpp), restated in float64 numpy.  These are
the FORMULAS, written out a second time: nothing here runs or reads the kernel, a change of gram_split or of gram_block's loop bounds
would not show here -- tests/test_gpu_gram_phase1.py ties the kernel to the sequential oracle.

  * The K split of the Gram products: of the S0 = ceil(nslots / 2) float4 slots of each lane half, wavefronts 0-2 contract [0, Sa) of one
    tile each and wavefront 3 contracts [Sa, S0) of all three, Sa = (3 S0 + 3) >> 2; the partial tiles are added.  Every slot is counted
    exactly once, whatever nslots, and the split sum is the plain sum up to float64 rounding.
  * The inverse factor in 16 x 16 quarters: with N = lr L = [[N00, 0], [N10, N11]] and each diagonal tile I + N.. = [[A, 0], [C, D]],
    (I + N..)^-1 = [[A^-1, 0], [-D^-1 C A^-1, D^-1]] (four unit-triangular quarters by forward substitution, 15 steps each), and
    M21 = -M22 N10 M11 one 16 x 16 quarter at a time: T = N10 M11 for the quarter's columns, then M22's row of quarters times T.
    The kernel does NOT use this form: it was built on these formulas, measured and removed (profiles/r08_phase1_ab.txt; the code:
    profiles/r08_gram_quartered_inverse.patch) -- gram_block inverts each diagonal tile in 31 steps and forms M21 on one wavefront.
    The cases stay as the algebra a later attempt has to satisfy."""
import numpy as np
import pytest

KB, KH = 64, 32


def gram_split(s0):
    return (3 * s0 + 3) >> 2


def slot_ranges(nslots):
    """[(wavefront role, lane half, slots)]: role 0 = wavefronts 0-2 (one tile each), role 1 = wavefront 3 (all three tiles)."""
    s0 = (nslots + 1) >> 1
    sa = gram_split(s0)
    out = []
    for h in range(2):
        out.append((0, h, [h * s0 + c for c in range(0, sa) if h * s0 + c < nslots]))
        out.append((1, h, [h * s0 + c for c in range(sa, s0) if h * s0 + c < nslots]))
    return s0, sa, out


@pytest.mark.parametrize("nslots", [1, 3, 4, 5, 25, 29, 63])
def test_k_split_gram_sum_is_the_plain_sum(nslots):
    rng = np.random.default_rng(nslots)
    rows = rng.normal(0.0, 0.3, size=(KB, 4 * nslots))  # a block's 64 user rows
    s0, sa, ranges = slot_ranges(nslots)
    assert 0 < sa <= s0 and 3 * sa >= 3 * (s0 - sa)  # wavefront 3 never has more than the others
    counted = sorted(s for _, _, slots in ranges for s in slots)
    assert counted == list(range(nslots))  # every slot once: nothing dropped, nothing twice
    tiles = {"G00": (slice(0, KH), slice(0, KH)), "G11": (slice(KH, KB), slice(KH, KB)), "G10": (slice(KH, KB), slice(0, KH))}
    for name, (ri, ci) in tiles.items():
        plain = rows[ri] @ rows[ci].T
        part = [np.zeros((KH, KH)), np.zeros((KH, KH))]
        for role, _, slots in ranges:
            for s in slots:
                cols = slice(4 * s, 4 * s + 4)
                part[role] += rows[ri, cols] @ rows[ci, cols].T
        assert np.abs((part[0] + part[1]) - plain).max() <= 1e-13, name


def test_k_split_gives_wavefront_3_an_empty_range_only_for_narrow_rows():
    for nslots in range(1, 64):
        s0, sa, _ = slot_ranges(nslots)
        assert (sa == s0) == (s0 <= 3)
    assert slot_ranges(25)[:2] == (13, 10)  # f = 100: 40 | 36 dependent MFMAs instead of 52


def forward_inverse(a):
    """(I + strictly lower a)^-1 by forward substitution, column by column: m[k] = delta(k, c) - sum_{j < k} a[k][j] m[j]."""
    n = a.shape[0]
    out = np.zeros((n, n))
    for c in range(n):
        m = np.zeros(n)
        for k in range(n):
            m[k] = (1.0 if k == c else 0.0) - a[k, :k] @ m[:k]
        out[:, c] = m
    return out


def quartered_inverse(n32):
    """(I + n32)^-1 of a strictly lower 32 x 32 tile from its 16 x 16 quarters."""
    ai, di = forward_inverse(n32[:16, :16]), forward_inverse(n32[16:, 16:])
    out = np.zeros((32, 32))
    out[:16, :16], out[16:, 16:] = ai, di
    out[16:, :16] = -(di @ (n32[16:, :16] @ ai))
    return out


def blockwise_m21(m11, m22, n10):
    out = np.zeros((32, 32))
    for rb in range(2):
        for cb in range(2):
            cols = slice(16 * cb, 16 * cb + 16)
            t = [n10[16 * kb:16 * kb + 16, :16] @ m11[:16, cols] + n10[16 * kb:16 * kb + 16, 16:] @ m11[16:, cols] for kb in range(2)]
            rows = slice(16 * rb, 16 * rb + 16)
            out[rows, cols] = -(m22[rows, :16] @ t[0] + m22[rows, 16:] @ t[1])
    return out


@pytest.mark.parametrize("n_valid", [1, 15, 16, 17, 31, 32, 33, 63, 64])
def test_quartered_inverse_and_blockwise_m21_are_the_inverse_of_i_plus_n(n_valid):
    lr, a, c = 0.01, 1.0 - 0.01 * 0.02, 1.0 - 0.01 * 0.02
    rng = np.random.default_rng(1000 + n_valid)
    gram = rng.uniform(-2.0, 2.0, size=(KB, KB))
    k, j = np.meshgrid(np.arange(KB), np.arange(KB), indexing="ij")
    d = k - 1 - j
    n = np.where((d >= 0) & (k < n_valid), lr * (c ** np.maximum(d, 0) + a ** np.maximum(d, 0) * gram), 0.0)  # rows past n_valid: zero
    assert np.all(np.triu(n) == 0.0)
    want = np.linalg.inv(np.eye(KB) + n)
    m11, m22 = quartered_inverse(n[:KH, :KH]), quartered_inverse(n[KH:, KH:])
    m21 = blockwise_m21(m11, m22, n[KH:, :KH])
    got = np.block([[m11, np.zeros((KH, KH))], [m21, m22]])
    assert np.abs(got - want).max() <= 1e-12
