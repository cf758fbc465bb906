"""The tiles the scorer cuts a long sequence into (bamm_score_tile_geometry, csrc/scorer.hip): a tile of
tile_positions positions starts on a multiple of the stride and emits the windows that start in its first `stride`
positions, the last tile up to L - W.  Pure host arithmetic: no device."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi

WIDTHS = [1, 2, 16, 17, 30, 100]


def emit_ranges(L, W, tile_positions, stride):
    """[first, last] window of every tile of a sequence of L positions, from the two numbers alone."""
    windows = L - W + 1
    out = []
    for k in range(-(-windows // stride)):
        t0 = k * stride
        first, last = t0, min(t0 + stride, windows) - 1
        assert last + W - 1 < t0 + tile_positions          # the tile holds every position of every window it emits
        out.append((first, last))
    return out


@pytest.mark.parametrize("W", WIDTHS)
def test_stride_and_cover(W):
    tile_positions, stride = bm.score_tile_geometry(W)
    assert tile_positions % 64 == 0 and 64 <= tile_positions <= 8192
    assert stride % 16 == 0
    assert 16 <= stride <= tile_positions - W + 1
    for L in (8193, tile_positions, tile_positions + 1, stride + W - 1, stride + W, 3 * stride + 5):
        seen = np.zeros(L - W + 1, np.int64)
        for first, last in emit_ranges(L, W, tile_positions, stride):
            assert first % stride == 0 and first <= last
            seen[first:last + 1] += 1
        assert np.array_equal(seen, np.ones(L - W + 1, np.int64)), (W, L)


def test_refusals():
    tile_positions, _ = bm.score_tile_geometry(1)
    lib = abi.load()
    assert lib.bamm_score_tile_geometry(0, None, None) == abi.ERR_ARG
    assert lib.bamm_score_tile_geometry(tile_positions - 14, None, None) == abi.ERR_ARG      # would leave a stride of 15
    assert lib.bamm_score_tile_geometry(tile_positions - 15, None, None) == abi.OK           # ... of 16
    with pytest.raises(abi.BammError):
        bm.score_tile_geometry(tile_positions + 1)
