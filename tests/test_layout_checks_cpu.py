"""The layout helper of tests/test_gpu_layouts.py and tests/test_gpu_streams.py judged on the CPU: the layout table obeys
include/cu2rec_amd.h and isolates what it claims to, and check_image is not blind -- it accepts a correct image of every layout and
rejects, with the region named, a touched guard word on either side, a nonzero padding float and rows packed at a wrong stride."""
import numpy as np
import pytest

import layout_checks as lc

WIDTHS = [1, 4, 5, 100, 252]
ROWS = 7


def _dense(f, rows=ROWS):
    return (np.arange(1, rows * f + 1, dtype=np.float32).reshape(rows, f) / 8).astype(np.float32)  # every entry distinct, none zero


def _images(f):
    """(what, dense, ld, front, back, image) for P and Q of every layout."""
    for lay in lc.LAYOUTS + [lc.DEFAULT]:
        for side, ld in (("P", lay.ldp(f)), ("Q", lay.ldq(f))):
            front, back = lc.guard_sizes(ld, lay.offset)
            dense = _dense(f)
            yield "%s %s" % (lay.name, side), dense, ld, front, back, lc.make_image(dense, ld, front, back)


@pytest.mark.parametrize("f", sorted(set(WIDTHS + lc.WIDTHS)))
def test_layout_table_obeys_the_header(f):
    for lay in lc.LAYOUTS + [lc.DEFAULT]:
        for ld in (lay.ldp(f), lay.ldq(f)):
            assert ld % 4 == 0 and ld >= f, (lay.name, f, ld)
            front, back = lc.guard_sizes(ld, lay.offset)
            assert front >= ld + 64 and back >= ld + 64
            assert (4 * front) % 256 == 4 * lay.offset  # the row region's place relative to a 256-byte aligned allocation
    crossed, dense, wide, offset16 = (lc.BY_NAME[n] for n in ("crossed", "dense", "wide", "offset16"))
    assert crossed.ldq(f) % 32 != 0 and crossed.ldp(f) > crossed.ldq(f)
    assert crossed.ldq(f) in (lc.round4(f) + 4, lc.round4(f) + 8)
    assert (dense.ldp(f) == f and dense.ldq(f) == f) == (f % 4 == 0)
    assert wide.ldp(f) == wide.ldq(f) == 2 * lc.round32(f) + 4
    assert (offset16.ldp(f), offset16.ldq(f)) == (lc.DEFAULT.ldp(f), lc.DEFAULT.ldq(f)) == (lc.round4(f), lc.round32(f))
    for ld in (offset16.ldp(f), offset16.ldq(f)):
        front, _ = lc.guard_sizes(ld, offset16.offset)
        assert front % 64 == 4 and (4 * front) % 32 == 16  # 16-byte aligned and nothing more


def test_the_schedule_test_changes_ldq_as_stated():
    assert [lc.BY_NAME[n].ldq(100) for n in ("crossed", "wide", "dense")] == [104, 260, 100]


@pytest.mark.parametrize("f", WIDTHS)
def test_check_image_accepts_a_correct_image(f):
    for what, dense, ld, front, back, image in _images(f):
        got = lc.check_image(image, ROWS, f, ld, front, back, what)
        assert got.shape == (ROWS, f)
        np.testing.assert_array_equal(got, dense, err_msg=what)
        assert np.isnan(image[:front]).all() and np.isnan(image[front + ROWS * ld:]).all()  # the sentinel is a NaN


@pytest.mark.parametrize("f", WIDTHS)
def test_check_image_rejects_a_touched_guard_word(f):
    for what, dense, ld, front, back, image in _images(f):
        n = ROWS * ld
        # the words next to the rows, the outermost ones, and one in the middle of each guard
        for region, at in [("front guard", front - 1), ("front guard", 0), ("front guard", front // 2),
                           ("back guard", front + n), ("back guard", front + n + back - 1), ("back guard", front + n + back // 2)]:
            bad = image.copy()
            bad.view(np.uint32)[at] ^= 1  # one bit: still a NaN, the comparison must be on the bits
            with pytest.raises(AssertionError, match=region) as e:
                lc.check_image(bad, ROWS, f, ld, front, back, what)
            assert "row %d, column %d" % ((at - front) // ld, (at - front) % ld) in str(e.value)
            bad = image.copy()
            bad[at] = 0.0
            with pytest.raises(AssertionError, match=region):
                lc.check_image(bad, ROWS, f, ld, front, back, what)


@pytest.mark.parametrize("f", WIDTHS)
def test_check_image_rejects_a_nonzero_padding_float(f):
    seen = 0
    for what, dense, ld, front, back, image in _images(f):
        for row, col in [(0, f), (ROWS - 1, ld - 1), (3, (f + ld) // 2)]:
            if col >= ld or col < f:
                continue  # no padding at all (dense layout, f % 4 == 0)
            for value in (1e-30, np.nan, -1.0):
                bad = image.copy()
                bad[front + row * ld + col] = value
                with pytest.raises(AssertionError, match="padding") as e:
                    lc.check_image(bad, ROWS, f, ld, front, back, what)
                assert "row %d, column %d" % (row, col) in str(e.value)
                seen += 1
    assert seen > 0


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("delta", [-4, 4])
def test_rows_packed_at_a_wrong_stride_do_not_pass(f, delta):
    """What a kernel that writes its rows at stride ld +- 4 leaves behind in an image of zero rows: the dense block read back at ld
    differs from the source, and where check_image returns at all it returns that differing block."""
    for what, dense, ld, front, back, image in _images(f):
        wrong = ld + delta
        if wrong < f:
            continue
        bad = lc.make_image(np.zeros_like(dense), ld, front, back)
        for r in range(ROWS):
            bad[front + r * wrong:front + r * wrong + f] = dense[r]
        assert not np.array_equal(lc.dense_block(bad, ROWS, f, ld, front), dense), what
        try:
            got = lc.check_image(bad, ROWS, f, ld, front, back, what)
        except AssertionError as e:
            assert "guard" in str(e) or "padding" in str(e)
            continue
        assert not np.array_equal(got, dense), what
