"""The conditions that make tests/test_coarse_unit_gpu.py meaningful, asserted without a GPU on regime R1_context with
the fp64 E step of tests/regimes.py.

(a) Enough windows lie where a coarse unit drops what a fine one keeps: at least 1 % with r in [2^-40, 2^-32) and at
    least 5 % in [2^-32, 2^-24).  (g_k0_ds_w2 has none of either: it is not among the coarse flavours.)
(b) The fp64 counts with every window truncated at 2^-s stay inside coarse_unit.count_bar and never rise above the
    untruncated ones.
(c) A deliberate mistake -- the scale applied twice in a list threshold, which drops every window with
    r < 2^-(2s - 40) -- breaches count_bar on every flavour at s = 24, and at s = 32 on every flavour but `sliced` and
    `order_7`, whose cells hold too few addends (the integer bound of the GPU test covers those).
(d) Under R1_context more than half of the cells that count at 2^-40 still count at every s >= 31 (what the GPU test
    asserts there); under R2_sharp the reference itself keeps fewer than half on two shapes, which is why the GPU test
    asserts a per-cell condition instead.
Also: the fp64 update restated in coarse_unit.update_v_f64 reproduces the oracle's, and the staircase of units.

Each test prints its figures (`gate ...` lines; run with -s).
"""
import numpy as np
import pytest

from tests import coarse_unit as cu
from tests import regimes

# one flavour per shape of the GPU test (layouts and tunings of a shape share their reference)
FLAVOURS = ["per_column", "layout0_k2_ds_N", "grouped_g5", "grouped_k3_odd", "mixed_a1", "mixed_a2", "sliced",
            "window_by_window", "order_7", "layout0_k1_ss"]
FEW_ADDENDS = ("sliced", "order_7")
REGIME = "R1_context"

_M: dict = {}


def bound_all_orders(inp, flavour):
    if flavour not in _M:
        m = cu.all_orders(inp, cu.addend_bound(inp))
        m.setflags(write=False)
        _M[flavour] = m
    return _M[flavour]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_windows_lie_between_the_units(flavour, orc):
    inp, ref = regimes.case(orc, REGIME, flavour)
    r = cu.windows_r(inp, ref.r64)
    fine = float(((r >= 2.0 ** -40) & (r < 2.0 ** -32)).mean())
    coarse = float(((r >= 2.0 ** -32) & (r < 2.0 ** -24)).mean())
    print(f"\ngate coarse {flavour}: {len(r)} windows, [2^-40, 2^-32) {100 * fine:.1f} %, [2^-32, 2^-24) {100 * coarse:.1f} %")
    assert fine >= 0.01 and coarse >= 0.05


def test_the_w2_shape_has_no_such_windows(orc):
    inp, ref = regimes.case(orc, REGIME, "layout0_k0_ds_w2")
    r = cu.windows_r(inp, ref.r64)
    assert not ((r >= 2.0 ** -40) & (r < 2.0 ** -24)).any()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_truncated_reference_stays_inside_the_bar(flavour, orc):
    inp, ref = regimes.case(orc, REGIME, flavour)
    m = bound_all_orders(inp, flavour)
    whole = cu.counts_from_r(inp, ref.r64)
    np.testing.assert_allclose(whole, ref.n_np, rtol=1e-12, atol=1e-300)
    for s in (39, 32, 24):
        cut = cu.counts_from_r(inp, ref.r64, cu.truncate(s))
        assert (cut <= whole).all()
        assert (whole - cut <= m * 2.0 ** -s).all()          # less than one unit per addend
        lo, hi = cu.count_bar(ref.n64, m, s)
        n64 = ref.n64.astype(np.float64)
        worst = float(np.max((n64 - cut) / (n64 - lo)))
        print(f"\ngate coarse {flavour} s={s}: max loss / bar {worst:.2f}")
        assert cu.inside(cut, ref.n64, m, s).all()
        # what margins.check is given on the GPU says the same as the bar
        folded = cu.fold_low_side(cut, ref.n64, m, s)
        assert (np.abs(folded - n64) <= regimes.N_ATOL + regimes.N_RTOL * np.abs(n64)).all()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_scale_applied_twice_breaches_the_bar(flavour, orc):
    inp, ref = regimes.case(orc, REGIME, flavour)
    m = bound_all_orders(inp, flavour)
    top = slice(regimes.v_offset(inp.K, inp.W), None)          # the accumulator's cells: order K
    for s in (32, 24):
        wrong = cu.counts_from_r(inp, ref.r64, cu.applied_twice(s))
        out = ~cu.inside(wrong, ref.n64, m, s)[top]
        print(f"\ngate coarse {flavour} s={s}: scale applied twice breaches {int(out.sum())}/{out.size} cells")
        if s == 32 and flavour in FEW_ADDENDS:
            continue
        assert out.any()
        # ... and folding the allowed deficit away does not hide it from margins.check
        folded = cu.fold_low_side(wrong, ref.n64, m, s)
        n64 = ref.n64.astype(np.float64)
        assert (np.abs(folded - n64) > regimes.N_ATOL + regimes.N_RTOL * np.abs(n64)).any()


def kept(inp, ref, s):
    """Of the cells that count at 2^-40 in fp64, the share that still counts at 2^-s."""
    top = slice(regimes.v_offset(inp.K, inp.W), None)
    at40 = cu.counts_from_r(inp, ref.r64, cu.truncate(40))[top] != 0
    return float(np.count_nonzero(cu.counts_from_r(inp, ref.r64, cu.truncate(s))[top][at40]) / at40.sum())


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_more_than_half_of_the_cells_still_count(flavour, orc):
    """The GPU test asserts it under R1_context at s >= 32, where the fp64 reference keeps 82 % of the cells or more.  Under
    R2_sharp it is no property of the regime: one window per sequence holds r ~ 1 and most cells that count at 2^-40 hold
    nothing but addends below 2^-32 (`long` keeps 35 % of them at 32, `m_k7` 39 %), so there the GPU test asserts, cell by
    cell, that a cell with an addend of r >= 2^(1-s) is not empty (coarse_unit.largest_addend)."""
    inp, ref = regimes.case(orc, REGIME, flavour)
    shares = {s: kept(inp, ref, s) for s in (39, 33, 32, 31)}
    print(f"\ngate coarse {flavour}: cells still counting " + "  ".join(f"s={s} {100 * x:.0f} %" for s, x in shares.items()))
    assert min(shares.values()) > 0.75
    top = cu.largest_addend(inp, ref.r64)
    for s in (39, 32, 24):
        must = top >= 2.0 ** (1 - s)
        cut = cu.counts_from_r(inp, ref.r64, cu.truncate(s))[regimes.v_offset(inp.K, inp.W):].reshape(top.shape)
        assert must.any() and (cut[must] > 0).all()


@pytest.mark.parametrize("flavour", ["window_by_window", "order_7"])
def test_a_sharp_model_empties_most_cells_at_32(flavour, orc):
    inp, ref = regimes.case(orc, "R2_sharp", flavour)
    share = kept(inp, ref, 32)
    print(f"\ngate coarse R2_sharp {flavour}: cells still counting at s=32 {100 * share:.0f} %")
    assert share < 0.5


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_fp64_update_from_counts_is_the_oracles(flavour, orc):
    """coarse_unit.update_v_f64 on the fp64 counts against em_step_f64's model (rounded to float once)."""
    inp, ref = regimes.case(orc, REGIME, flavour)
    v = cu.update_v_f64(inp, ref.n_np)
    np.testing.assert_allclose(v, ref.v64, rtol=2e-7, atol=1e-12)


def test_addend_bound_counts_every_window_once(orc):
    inp, ref = regimes.case(orc, REGIME, "per_column")
    m = cu.addend_bound(inp)
    lens = np.diff(inp.off.astype(np.int64)) - inp.W + 1
    for j in range(inp.W):
        assert m[:, j].sum() == np.maximum(lens - j, 0).sum()
    # with every r equal to one the counts are the bound itself
    ones = np.ones_like(ref.r64)
    for o, LW1, _ in cu._windows(inp):
        ones[o + LW1:o + LW1 + inp.W - 1] = 0.0
    assert np.array_equal(cu.counts_from_r(inp, ones), cu.all_orders(inp, m).astype(np.float64))


def test_staircase_of_units():
    for s, bound in cu.BOUNDS.items():
        assert cu.fix_shift_of(bound) == s and cu.fix_shift_of(bound + 1) == max(s - 1, 24), (s, bound)
    assert cu.fix_shift_of(1 << 22) == 40 and cu.fix_shift_of((1 << 22) + 1) == 39 and cu.fix_shift_of(1) == 40
    assert cu.fix_shift_of(1 << 62) == 24
    for bits in range(0, 39):                                 # the int64 total stays below 2^62 up to 2^38 sequences
        assert (1 << bits) * (1 << cu.fix_shift_of(1 << bits)) <= 1 << 62
