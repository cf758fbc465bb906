"""Word y of the mixed-row kernel's lane records (csrc/lane_records.h: mix_fix_word, the function k_mix_records runs, exported
for the host as bamm_mix_fix_word) against values worked out by hand.

The layout at W = 20 and 7 positions per lane: T = 6 groups, B = 4 narrow ones of 3 columns (columns 0..11), A = 2 wide
ones of 4 (12..15, 16..19); lane = row * 6 + group, rows 0..5 for group ends next to an exception (the strand junction),
rows 6..8 for the positions L-W+1 .. L-W+3 whose groups the edge cuts; bins of the first n1c = 11 columns are resident.
A sequence of L = 401 positions has LW1 = L - W + 1 = 382 windows; a group that ends at position p covers p-G+1 .. p.
Word y: four 7-bit codes (64 = none) and, in bit 31, "some column has a code and no resident bin": something is left to log."""
import pytest

import bammmotif2_amd as bm

W, M, L = 20, 7, 401
LOG = 1 << 31


def word(f0, f1, f2, f3, log=False):
    return f0 | f1 << 7 | f2 << 14 | f3 << 21 | (LOG if log else 0)


@pytest.fixture(scope="module")
def lay(lib):
    lay = bm.mix_layout(W, M)
    assert lay == dict(T=6, B=4, A=2, n1c=11)
    return lay


def fix_word(lay, lane, xw, xfields=0, sE=0, n1c=None):
    return bm.mix_fix_word(lane, W, lay["T"], lay["B"], lay["n1c"] if n1c is None else n1c, L, xw, xfields, sE)


def test_layouts_of_the_other_widths(lib):
    """W = 13 and 16: one wide group, every column resident; no mixed rows at a multiple of 3."""
    assert bm.mix_layout(13, 7) == dict(T=4, B=3, A=1, n1c=13)
    assert bm.mix_layout(16, 7) == dict(T=5, B=4, A=1, n1c=16)
    with pytest.raises(Exception):
        bm.mix_layout(18, 7)


def test_junction_row_that_ends_at_a_lane_boundary(lay):
    """Exceptions from position 200 on, six group ends: row 2 stands for the groups that end at position 202 = 28 * 7 + 6, the
    last slot of lane 28.  Group 1 (narrow, columns 3..5, all resident) covers 200..202: three codes, the fourth none
    whatever the record holds there; nothing to log."""
    xw = 200 | 6 << 12
    xf = word(5, 17, 63, 9)
    assert fix_word(lay, 2 * 6 + 1, xw, xf) == (word(5, 17, 63, 64), True)
    # row 5 is the last of the six; with four group ends rows 4 and 5 are no fix lanes (and rows 6.. are the edge's)
    assert fix_word(lay, 5 * 6 + 1, xw, xf) == (word(5, 17, 63, 64), True)
    assert fix_word(lay, 5 * 6 + 1, 200 | 4 << 12, xf) == (word(64, 64, 64, 64), False)
    # a group that starts before the sequence: row 0 at position 1 covers -1, 0, 1
    assert fix_word(lay, 0 * 6 + 1, 1 | 6 << 12, xf) == (word(64, 17, 63, 64), True)


def test_columns_on_either_side_of_the_resident_ones(lay):
    """Group 3 holds columns 9, 10 (resident) and 11 (logged): the flag follows column 11's code alone; with 12 resident
    columns nothing is left, with 9 all three are."""
    xw = 200 | 6 << 12
    lane = 2 * 6 + 3
    assert fix_word(lay, lane, xw, word(5, 17, 63, 9)) == (word(5, 17, 63, 64, log=True), True)
    assert fix_word(lay, lane, xw, word(5, 17, 64, 9)) == (word(5, 17, 64, 64), True)
    assert fix_word(lay, lane, xw, word(64, 64, 0, 9)) == (word(64, 64, 0, 64, log=True), True)
    assert fix_word(lay, lane, xw, word(5, 17, 63, 9), n1c=12) == (word(5, 17, 63, 64), True)
    assert fix_word(lay, lane, xw, word(5, 64, 64, 9), n1c=9) == (word(5, 64, 64, 64, log=True), True)
    # a wide group (columns 12..15) takes the fourth code as well; none of its columns is resident
    assert fix_word(lay, 2 * 6 + 4, xw, word(5, 17, 63, 9)) == (word(5, 17, 63, 9, log=True), True)
    assert fix_word(lay, 2 * 6 + 4, xw, word(64, 64, 64, 64)) == (word(64, 64, 64, 64), True)


def test_edge_row_with_two_clipped_columns(lay):
    """Row 7 stands for position LW1 + 1 = 383; the wide group 4 covers 380..383, of which 382 and 383 are beyond the last
    window.  The stream window that ends at position 381 gives the codes: position 381 its low six bits, 380 the six bits
    one base up.  0x2d7 = 10 1101 0111: 23 and 53."""
    assert fix_word(lay, 7 * 6 + 4, 200 | 6 << 12, sE=0x2D7) == (word(53, 23, 64, 64, log=True), True)
    # row 8 (position 384), narrow group 0: 382..384, wholly beyond the edge -- a fix lane with nothing to add or log
    assert fix_word(lay, 8 * 6 + 0, 200 | 6 << 12, sE=0x2D7) == (word(64, 64, 64, 64), True)
    # row 6 (position 382), narrow group 2 (columns 6..8, resident): 380, 381 and one clipped column; nothing to log
    assert fix_word(lay, 6 * 6 + 2, 200 | 6 << 12, sE=0x2D7) == (word(53, 23, 64, 64), True)


def test_lanes_beyond_the_fix_rows(lay):
    """Lanes 54..63 (rows 9 and 10) have no role: no fix lane, no code, nothing to log, whatever the inputs."""
    for lane in (54, 59, 63):
        assert fix_word(lay, lane, 200 | 6 << 12, word(5, 17, 63, 9), sE=0x2D7) == (word(64, 64, 64, 64), False)
