"""The tiles an EM pass cuts a sequence beyond 8192 positions into (bamm_em_tile_geometry, csrc/em_tiles.hip): a tile of
tile_positions positions starts on a multiple of the stride and owns the windows that start in its first `stride`
positions, the last tile up to L - W; every window a tile owns lies wholly inside it.  Pure host arithmetic: no device."""
import ctypes as C

import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi


@pytest.mark.parametrize("W", [1, 12, 20, 30])
def test_stride_is_the_largest_multiple_of_16_that_leaves_the_overlap(W):
    tile_positions, stride = bm.em_tile_geometry(W)
    assert tile_positions % 64 == 0 and 64 <= tile_positions <= 8192
    assert stride % 16 == 0 and stride >= 16
    assert stride + W - 1 <= tile_positions                # the last window a tile owns ends inside it
    assert stride + 16 + W - 1 > tile_positions            # ... and the next multiple of 16 would not
    for L in (8193, tile_positions, stride + W - 1, stride + W, 3 * stride + 5):   # every window has exactly one owner
        windows = L - W + 1
        tiles = -(-windows // stride)
        assert (tiles - 1) * stride < windows <= tiles * stride
        assert min(tiles * stride, windows) - 1 + W - 1 < (tiles - 1) * stride + tile_positions


def test_refusals():
    tile_positions, _ = bm.em_tile_geometry(1)
    lib = abi.load()
    assert lib.bamm_em_tile_geometry(0, None, None) == abi.ERR_ARG
    assert lib.bamm_em_tile_geometry(tile_positions - 14, None, None) == abi.ERR_ARG         # would leave a stride of 15
    assert lib.bamm_em_tile_geometry(tile_positions - 15, None, None) == abi.OK              # ... of 16
    with pytest.raises(abi.BammError):
        bm.em_tile_geometry(tile_positions + 1)
    assert lib.bamm_em_tile_plan(None, None, None, None) == abi.ERR_ARG                      # no handle


def test_symbols_are_exported():
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("bamm_em_tile_geometry", "bamm_em_tile_plan"):
        assert name in abi.SYMBOLS and hasattr(lib, name), name
