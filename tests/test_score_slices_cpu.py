"""The slices of motif columns the scorer takes a log-odds table beyond one CU's LDS in (bamm_score_slice_geometry,
csrc/score.cpp): as many columns as fit 160 KiB, the fewest slices, those balanced.  Pure host arithmetic: no device."""
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi

LDS = 163840


@pytest.mark.parametrize("K,W,slices,columns", [(5, 9, 1, 9), (5, 10, 2, 5), (5, 20, 3, 7), (4, 39, 1, 39), (4, 40, 2, 20),
                                                (6, 2, 1, 2), (6, 3, 2, 2), (6, 12, 6, 2), (3, 160, 2, 80)])
def test_listed_values(K, W, slices, columns):
    assert bm.score_slice_geometry(K, W) == (columns, slices)


def test_refusals():
    lib = abi.load()
    assert lib.bamm_score_slice_geometry(5, 0, None, None) == abi.ERR_ARG
    assert lib.bamm_score_slice_geometry(11, 4, None, None) == abi.ERR_ARG                    # beyond BAMM_MAX_ORDER
    for K in (7, 8, 9, 10):                                                                    # not one column fits
        assert lib.bamm_score_slice_geometry(K, 4, None, None) == abi.ERR_ARG
    assert lib.bamm_score_slice_geometry(6, 4, None, None) == abi.OK                          # either pointer may be NULL
    with pytest.raises(abi.BammError):
        bm.score_slice_geometry(7, 4)


def test_every_slice_fits_and_the_slices_cover_the_motif():
    for K in range(7):
        column_bytes = (4 ** (K + 1) + 1) * 4
        for W in range(1, 65):
            columns, slices = bm.score_slice_geometry(K, W)
            assert columns * column_bytes <= LDS, (K, W)
            assert slices * columns >= W > (slices - 1) * columns, (K, W)
            assert (slices == 1) == (W * column_bytes <= LDS), (K, W)
