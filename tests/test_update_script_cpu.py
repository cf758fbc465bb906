"""The expectations and scripts of tests/update_script.py, checked where no GPU is needed.

tests/test_update_exact_gpu.py and tests/test_optimize_script_gpu.py compare the device's model update bit for bit with
expected_update(); what that is made of is pinned here: its marginalisation against the oracle's own lower orders, every
script against orc.update_v's finiteness, the knife-edge inputs of the loop tests against their conditions, and the
read-out the GPU cases assert their form with against the header and the binding.
"""
import os
import re

import numpy as np
import pytest

from bammmotif2_amd import abi
from tests import update_script as us

SHAPES = [(0, 5), (1, 7), (2, 8), (3, 8), (4, 1), (4, 2), (5, 3), (7, 2)]


@pytest.mark.parametrize("K,W", SHAPES, ids=[f"K{k}_W{w}" for k, w in SHAPES])
def test_marginalisation_equals_the_oracles_lower_orders(K, W, orc):
    """orc.mstep_counts sums r into order K and then runs EM.cpp:247-254 itself: from ITS top order the numpy chain must
    give ITS lower orders, bit for bit."""
    rs = np.random.RandomState(100 * K + W)
    N, L = 6, W + 12
    off = (np.arange(N + 1) * L).astype(np.uint64)
    kmer = rs.randint(0, 4 ** 11, size=N * L).astype(np.uint64)
    r = rs.random_sample(N * L).astype(np.float32)
    n = orc.mstep_counts(kmer, off, K, W, r)
    top = n[us.v_offset(K, W):]
    assert top.size == us.cells_of(K, W) and np.count_nonzero(top) > 0
    assert np.array_equal(us.bits(us.marginalise(top, K, W)), us.bits(n))


def test_marginalisation_order_matters_at_float32():
    """the check above can tell ((c0 + c1) + c2) + c3 from another grouping: on these four rows they differ"""
    c = np.array([[2.0 ** 24], [1.0], [1.0], [1.0]], np.float32)            # K = 1, W = 1: rows y = d * 4 + 0 of order 1
    nK = np.zeros((16, 1), np.float32)
    nK[[0, 4, 8, 12]] = c
    got = us.marginalise(nK, 1, 1)[0]
    assert got == np.float32(2.0 ** 24)                       # 2^24 + 1 rounds back to 2^24, three times
    assert np.float32(np.float32(c[1, 0] + c[2, 0]) + c[3, 0]) + c[0, 0] == np.float32(2.0 ** 24 + 4)


@pytest.mark.parametrize("kind", sorted(us.COUNTS))
@pytest.mark.parametrize("K,W", [(0, 6), (2, 8), (4, 2), (3, 9)], ids=lambda x: str(x))
@pytest.mark.parametrize("regime", [None] + list(us.ALPHA_REGIMES))
def test_every_script_keeps_update_v_finite(kind, K, W, regime, orc):
    inp = us.tiny_inputs(orc, K, W, regime=regime)
    for shift in (40, 32, 24):
        for r in us.script(kind, 3, K, W, 2, inp.N):
            n, v, s, *_ = us.expected_update(r, shift, K, W, min(2, K), inp.A, inp.vbg, inp.v, inp.q, True, 0, orc)
            assert np.isfinite(n).all() and np.isfinite(v).all() and np.isfinite(s).all()
            assert (v >= 0).all()


def test_statistics_words_decode_as_documented():
    assert us.decode_stats(us.stats(-3.5, 2.25, 17)) == (-3.5, 2.25, 17.0)
    llh, sum_r, nseq = us.decode_stats(us.stats(1.0, 0.5, 33, bad=2))
    assert np.isnan(llh) and sum_r == 0.5 and nseq == 33.0    # a plausible count stays in the low bits under the flag


@pytest.mark.parametrize("kind", sorted(us.LOOP_KINDS))
def test_knife_edge_scripts_satisfy_their_conditions(kind, orc):
    """The loop tests put epsilon at float32(D) and one float above it.  D (every pass from the second on) and D1 (the
    first pass) must round to the same float32 under any fp64 grouping, and the first pass must not stop under either
    epsilon.  Conditions on the inputs: a seed that misses them is replaced, the conditions stay."""
    D1, D = us.knife_edge(orc, kind)
    assert D > 0 and us.far_from_a_tie(D) and us.far_from_a_tie(D1)
    above = np.nextafter(np.float32(D), np.float32(np.inf))
    assert np.float32(D1) >= above                            # v_diff < epsilon is false at pass 1 for both epsilons
    assert not (np.float32(D) < np.float32(D)) and np.float32(D) < above


def test_far_from_a_tie_refuses_a_midpoint():
    f = np.float32(1.0)
    g = np.nextafter(f, np.float32(2.0))
    mid = 0.5 * (float(f) + float(g))
    assert not us.far_from_a_tie(mid) and not us.far_from_a_tie(mid * (1 + 1e-10))
    assert us.far_from_a_tie(mid * (1 + 1e-8)) and us.far_from_a_tie(1.0)


def test_header_declares_and_abi_binds_plan_update(lib):
    hdr = open(os.path.join(os.path.dirname(abi.HERE), "include", "bamm_em.h")).read()
    m = re.search(r"\bint\s+bamm_em_plan_update\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 3
    assert "bamm_em_plan_update" in abi.SYMBOLS and len(lib.bamm_em_plan_update.argtypes) == 3
    assert lib.bamm_em_plan_update(None, None, None) == abi.ERR_ARG          # no handle; no device work either way
