"""The fix lanes of the mixed-row kernel after their record took over more of their work (csrc/lane_records.h, csrc/mixed_kernel.h):
the fix-lane flag rides in the window word, the record says whether a lane has anything left to log, the lane extracts
each column's code once for its two uses, reads the single-column table at one base plus constant offsets, adds to the
resident bins at one base plus constant offsets under masks formed by the scalar unit, and skips the fourth add where no
wide group has a resident bin.

What can go wrong with that and is tested here: a sum that goes to the wrong bin or to both the bin and the log (the
resident and the logged columns, the two on either side of the boundary on their own, widths where every column is
resident and the fourth add is issued), an offset or mask that depends on the wave or the block (the integer accumulator
for launches of 1, 2 and 5 blocks), the junction's first virtual row on every slot of a lane with consecutive sequences
of a wave differing in it, and neutral codes: the narrow groups' fourth column, the edge rows' clipped columns, beside a
set of which a part goes to the per-column kernel.

All handles are forced onto the mixed rows and run with two blocks (tests/test_lane_records_gpu.py: mixed_em).  The bars
are that file's first test's (r against the oracle with the zero pattern, llh, v after one pass against the fp64
restatement) and, for the counts after one M-step against the oracle's, the suite's own (tests/test_parity_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth
from bammmotif2_amd.em import v_offset
from tests.cases import Case
from tests.test_lane_records_gpu import mixed_em
from tests.test_partition_exact_gpu import accumulator

pytestmark = pytest.mark.gpu

_POSITIONS = (4, 5, 6, 7, 8, 10)                             # per lane: the length classes of the mixed rows


def positions_per_lane(L):
    return next(m for m in _POSITIONS if 64 * m >= L)


class Ref:
    """One case through the oracle, once: r and llh of the E step at the seed, the counts of its M step, v after the step in fp64."""

    def __init__(self, c, orc):
        self.c = c
        self.seq, self.kmer, self.off, self.vbg = c.encode(orc)
        self.pk = bm.PackedSeqs.from_kmers(self.kmer, self.off)
        self.r, self.llh = orc.estep(self.kmer, self.off, c.K, c.W, orc.linear_s(c.v0, self.vbg, c.K, c.W, min(c.bg_order, c.K)), c.q)
        self.n = orc.mstep_counts(self.kmer, self.off, c.K, c.W, self.r)
        self.v64 = orc.em_step_f64(self.kmer, self.off, c.K, c.W, c.bg_order, self.vbg, c.A, c.v0, c.q)[0]


_REFS = {}


def ref_of(key, make, orc):
    if key not in _REFS:
        _REFS[key] = Ref(make(), orc)
    return _REFS[key]


def column(n, K, W, j):
    """The counts of motif column j, every order (layout [k][y][j])."""
    return np.concatenate([n[v_offset(k, W):v_offset(k + 1, W)].reshape(-1, W)[:, j] for k in range(K + 1)])


def one_step(ctx, ref):
    """E step, M step and a fused pass of mixed-row handles against the reference; returns (counts, (grouped, other))."""
    c = ref.c
    ss = bm.SeqSet(ctx, ref.pk)
    em = mixed_em(ctx, ss, c, ref.vbg)
    grouped, other, _ = em.plan()
    assert em.plan_mixed() == grouped > 0
    em.EStep()
    r_g = em.getR()
    np.testing.assert_allclose(r_g, ref.r, rtol=1e-5, atol=1e-12)
    assert np.array_equal(r_g == 0, ref.r == 0)
    np.testing.assert_allclose(em.getLLH(), ref.llh, rtol=2e-6, atol=2e-6 * c.N)
    em.MStep()
    n_g = em.getCounts()
    np.testing.assert_allclose(n_g, ref.n, rtol=1e-5, atol=1e-6)
    em.close()
    em = mixed_em(ctx, ss, c, ref.vbg)
    em.iterate(1)
    np.testing.assert_allclose(em.getV(), ref.v64, rtol=1e-6, atol=1e-9)
    em.close(); ss.close()
    return n_g, (grouped, other)


@pytest.mark.parametrize("W", [20, 13, 16])
def test_resident_and_logged_bins(W, gpu_ctx, orc):
    """W = 20: 11 of 20 columns have resident bins, the rest are logged; W = 13 and 16: all columns are resident, the wide
    group's fourth column among them.  The counts after one M step, then the integers for 1, 2 and 5 blocks."""
    lay = bm.mix_layout(W, 7)
    assert lay["n1c"] == (11 if W == 20 else W) and lay["B"] + lay["A"] == lay["T"]
    ref = ref_of(("bins", W), lambda: Case(name="fix_bins", N=240, L0=200, W=W, K=2), orc)
    c = ref.c
    assert positions_per_lane(2 * c.L0 + 1) == 7
    n_g, (grouped, other) = one_step(gpu_ctx, ref)
    assert grouped == c.N and other == 0
    hip = C.CDLL("libamdhip64.so")
    shape = dict(N=c.N, K=c.K, W=c.W, tune=dict(group_layout=8))
    cells = 4 ** (c.K + 1) * c.W
    acc = [accumulator(gpu_ctx, hip, ref.pk, 0, c.N, shape, ref.vbg, c.A, c.v0, (blocks, 0)) for blocks in (1, 2, 5)]
    assert acc[0][cells + 2] == c.N and acc[0][cells] != 0 and np.count_nonzero(acc[0][:cells]) > cells // 2
    assert np.array_equal(acc[0], acc[1]) and np.array_equal(acc[0], acc[2])


def test_the_columns_on_either_side_of_the_boundary(gpu_ctx, orc):
    """W = 20: the last column with a resident bin and the first logged one, each against the oracle on its own."""
    W = 20
    n1c = bm.mix_layout(W, 7)["n1c"]
    assert 0 < n1c < W
    ref = ref_of(("bins", W), lambda: Case(name="fix_bins", N=240, L0=200, W=W, K=2), orc)
    c = ref.c
    ss = bm.SeqSet(gpu_ctx, ref.pk)
    em = mixed_em(gpu_ctx, ss, c, ref.vbg)
    em.EStep(); em.MStep()
    n_g = em.getCounts()
    em.close(); ss.close()
    for j in (n1c - 1, n1c):
        want = column(ref.n, c.K, W, j)
        assert np.count_nonzero(want[-64:]) > 32, "the column's order-2 counts are meant to be populated"
        np.testing.assert_allclose(column(n_g, c.K, W, j), want, rtol=1e-5, atol=1e-6, err_msg=f"column {j}")


def junction_case():
    """240 sequences of 176 .. 190 bp in turn (L = 353 .. 381: one length class, six positions per lane), so that the
    strand junction -- the first virtual row -- falls on every slot of a lane, lane boundaries included, and differs
    between consecutive sequences of a wave."""
    c = Case(name="fix_junction", N=240, L0=190, W=20, K=2)
    lens = 176 + np.arange(c.N) % 15
    assert lens.min() == 176 and lens.max() == 176 + 2 * 7
    keep = np.concatenate([np.arange(int(c.in_off[n]), int(c.in_off[n]) + int(lens[n])) for n in range(c.N)])
    c.codes = c.codes[keep]
    c.in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return c


def test_junction_on_every_slot_of_a_lane(gpu_ctx, orc):
    ref = ref_of("junction", junction_case, orc)
    c = ref.c
    lens = np.diff(ref.off.astype(np.int64))
    M = positions_per_lane(int(lens.max()))
    assert positions_per_lane(int(lens.min())) == M, "one length class"
    junction = (lens - 1) // 2                               # position of the strand separator
    assert len(set(junction % M)) == M and np.all(np.diff(junction) != 0)
    ss = bm.SeqSet(gpu_ctx, ref.pk)
    em = mixed_em(gpu_ctx, ss, c, ref.vbg)
    grouped, other, launches = em.plan()
    em.close(); ss.close()
    assert grouped == c.N and other == 0 and launches == 1, "all sequences in one launch of the mixed-row kernel"
    one_step(gpu_ctx, ref)


_NEUTRAL = [(100, 14), (100, 17), (140, 14), (140, 17)]


@pytest.mark.parametrize("n_frac", [0.0, 0.01], ids=["clean", "with_N"])
@pytest.mark.parametrize("L0,W", _NEUTRAL, ids=[f"L0_{l}_W{w}" for l, w in _NEUTRAL])
def test_neutral_and_clipped_columns(L0, W, n_frac, gpu_ctx, orc):
    """Two wide groups after narrow ones (the narrow groups' fourth code is neutral), edge rows with clipped columns; with
    N bases a part of the set goes to the per-column kernel and the whole set's counts still meet the bar."""
    ref = ref_of(("neutral", L0, W, n_frac), lambda: Case(name="fix_neutral", N=240, L0=L0, W=W, K=2, n_frac=n_frac), orc)
    _, (grouped, other) = one_step(gpu_ctx, ref)
    assert grouped + other == ref.c.N
    if n_frac:
        assert other > 0, "part of the set is meant to go through k_em_seq"
    else:
        assert other == 0
