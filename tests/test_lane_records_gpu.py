"""The lane records of the mixed-row kernel (bammmotif2_amd/csrc/lane_records.h): k_em_mix loads every lane's stream
window and fix-lane codes from a record built once per handle and bucket instead of deriving them in every pass.

What can go wrong with that and is tested here: a record derived for another length class or width (every instantiated
M with one and with two wide groups), the window of the last lanes and the edge fix lanes when lengths and the strand
junction change from sequence to sequence of a wave, a record read from the wrong launch slot (index lists, shards,
fold masks, other launch shapes), state carried from one sequence of a wave to the next (a fix lane whose fields are all
neutral must still rewrite its virtual cells), and records that belong to the handle, not to the set (two handles of
different width on one set, closed in either order).

All handles are forced onto the mixed rows (group_layout 8) and run with two blocks, so that a few hundred sequences
give every wave several sequences in a row: the one-ahead prefetch and the stale virtual rows are exercised.

Group ends next to an exception: a sequence reaches this kernel with none or with 4..6 of them (the strand junction's
three k-mers carry independent random digits, Sequence.cpp:38, so any subset of them differs from the stream, and the
widest group adds three positions); fewer than 4 only exist clipped at the sequence's end, beyond the EM.cpp:167 edge,
where the planner hands the sequence to k_em_seq."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth
from tests.cases import Case
from tests.test_partition_exact_gpu import accumulator

pytestmark = pytest.mark.gpu


def mixed_em(ctx, ss, c, vbg, W=None, blocks=2, **kw):
    ctx.set_tuning(group_layout=8)
    ctx.set_launch(blocks, 0)
    try:
        W = W or c.W
        A = c.A if W == c.W else synth.alpha_matrix(c.alpha, W)
        v0 = c.v0 if W == c.W else width_seed(c, W)
        em = bm.EM(ctx, ss, c.K, W, vbg, A, v0, c.q, bg_order=c.bg_order, **kw)
    finally:
        ctx.set_launch(0, 0)
        ctx.set_tuning(group_layout=-1)
    assert em.plan_mixed() > 0
    return em


def width_seed(c, W):
    pwm = synth.make_pwm(W, c.seed)
    return synth.bamm_from_pwm((0.7 * pwm + 0.3 * 0.25).astype(np.float32), c.K)


# L = 2 L0 + 1 -> 4, 5, 6, 7, 8, 10 positions per lane; every M once with one wide group (W 13 / 16) and once with two
# (W 14 / 17 / 20)
_EVERY_M = [(100, 13), (100, 14), (140, 16), (140, 17), (180, 13), (180, 20), (200, 16), (200, 20), (240, 13), (240, 17),
            (300, 16), (300, 14)]


@pytest.mark.parametrize("L0,W", _EVERY_M, ids=[f"L0_{l}_W{w}" for l, w in _EVERY_M])
def test_every_length_class_and_both_widths_of_the_tail(L0, W, gpu_ctx, orc):
    """One pass's r against the oracle (zero pattern included), v after one pass against the fp64 restatement, then the
    uniform rows: the bars of test_mixed_rows_agree_with_exact_arithmetic_and_uniform_rows."""
    c = Case(name="rec_m", N=240, L0=L0, W=W, K=2, n_frac=0.002 if W % 3 == 2 else 0.0)
    seq, kmer, off, vbg = c.encode(orc)
    ss = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_kmers(kmer, off))
    em = mixed_em(gpu_ctx, ss, c, vbg)
    grouped = em.plan()[0]
    assert em.plan_mixed() == grouped
    em.EStep()
    r_o, llh_o = orc.estep(kmer, off, c.K, c.W, orc.linear_s(c.v0, vbg, c.K, c.W, min(c.bg_order, c.K)), c.q)
    r_g = em.getR()
    np.testing.assert_allclose(r_g, r_o, rtol=1e-5, atol=1e-12)
    assert np.array_equal(r_g == 0, r_o == 0)
    np.testing.assert_allclose(em.getLLH(), llh_o, rtol=2e-6, atol=2e-6 * c.N)
    v64, *_ = orc.em_step_f64(kmer, off, c.K, c.W, c.bg_order, vbg, c.A, c.v0, c.q)
    em.iterate(1)
    np.testing.assert_allclose(em.getV(), v64, rtol=1e-6, atol=1e-9)
    em.iterate(3)
    v_mix, llh_mix, n_mix = em.getV(), em.trace()[0].copy(), em.getCounts()
    em.close()
    gpu_ctx.set_tuning(group_layout=3)
    try:
        em = bm.EM(gpu_ctx, ss, c.K, c.W, vbg, c.A, c.v0, c.q, bg_order=c.bg_order)
    finally:
        gpu_ctx.set_tuning(group_layout=-1)
    assert abs(em.plan()[0] - grouped) <= 2 and em.plan_mixed() == 0
    em.iterate(4)
    np.testing.assert_allclose(llh_mix, em.trace()[0], rtol=2e-6)
    np.testing.assert_allclose(n_mix, em.getCounts(), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(v_mix, em.getV(), rtol=2e-5, atol=1e-9)
    em.close(); ss.close()


class Ragged:
    """320 double-stranded sequences of 193..221 bp (L = 387..443: all of them 7 positions per lane), so that L - W + 1
    and the junction move from sequence to sequence; every fourth has an N one to three bases in front of the junction
    (more, or other, group ends next to an exception; runs too long for the virtual rows), every sixteenth an N
    somewhere else as well (two exception sites: the mixed rows cannot take it, the bucket carries an index list)."""

    def __init__(self, orc):
        c = Case(name="rec_ragged", N=320, L0=207, W=20, K=2, ragged=14)
        rs = np.random.RandomState(11)
        lens = np.diff(c.in_off.astype(np.int64))
        for n in range(c.N):
            b = int(c.in_off[n])
            if n % 4 == 1:
                c.codes[b + lens[n] - 1 - (n % 3)] = 0
            if n % 16 == 5:
                c.codes[b + 30 + rs.randint(0, lens[n] - 60)] = 0
        self.c = c
        self.seq, self.kmer, self.off, self.vbg = c.encode(orc)
        self.pk = bm.PackedSeqs.from_kmers(self.kmer, self.off)
        self.f64 = {}
        self.orc = orc

    def v64(self, W):                                        # v after one step in exact arithmetic, per width
        if W not in self.f64:
            c = self.c
            A = c.A if W == c.W else synth.alpha_matrix(c.alpha, W)
            v0 = c.v0 if W == c.W else width_seed(c, W)
            self.f64[W] = self.orc.em_step_f64(self.kmer, self.off, c.K, W, c.bg_order, self.vbg, A, v0, c.q)[0]
        return self.f64[W]


@pytest.fixture(scope="module")
def ragged(orc):
    return Ragged(orc)


def test_ragged_lengths_within_one_class(ragged, gpu_ctx, orc):
    c = ragged.c
    ss = bm.SeqSet(gpu_ctx, ragged.pk)
    em = mixed_em(gpu_ctx, ss, c, ragged.vbg)
    grouped, other, _ = em.plan()
    assert 0 < em.plan_mixed() == grouped < c.N and other == c.N - grouped, "the bucket is meant to carry an index list"
    em.EStep()
    r_o, llh_o = orc.estep(ragged.kmer, ragged.off, c.K, c.W, orc.linear_s(c.v0, ragged.vbg, c.K, c.W, min(c.bg_order, c.K)), c.q)
    r_g = em.getR()
    np.testing.assert_allclose(r_g, r_o, rtol=1e-5, atol=1e-12)
    assert np.array_equal(r_g == 0, r_o == 0)
    np.testing.assert_allclose(em.getLLH(), llh_o, rtol=2e-6, atol=2e-6 * c.N)
    em.iterate(1)
    np.testing.assert_allclose(em.getV(), ragged.v64(c.W), rtol=1e-6, atol=1e-9)
    em.close(); ss.close()


def test_records_follow_the_launch_slot(ragged, gpu_ctx):
    """Integers: the counts do not depend on which wave gets which slot, with and without a fold mask, and the
    accumulators of two shards add up to the whole set's word for word."""
    c = ragged.c
    ss = bm.SeqSet(gpu_ctx, ragged.pk)
    mask = (np.arange(c.N) % 5 != 2).astype(np.uint8)
    for kw in (dict(), dict(mask=mask)):
        counts = []
        for blocks in (1, 3):
            em = mixed_em(gpu_ctx, ss, c, ragged.vbg, blocks=blocks, **kw)
            em.iterate(1)
            counts.append(em.getCounts())
            em.close()
        assert np.array_equal(counts[0], counts[1]), kw.keys()
    ss.close()
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    shape = dict(N=c.N, K=c.K, W=c.W, tune=dict(group_layout=8))
    whole = accumulator(gpu_ctx, hip, ragged.pk, 0, c.N, shape, ragged.vbg, c.A, c.v0, (2, 0))
    cells = 4 ** (c.K + 1) * c.W
    assert whole[cells + 2] == c.N and whole[cells] != 0
    for cuts in ((0, c.N // 2, c.N), (0, 37, c.N)):
        total = np.zeros_like(whole)
        for b, e in zip(cuts[:-1], cuts[1:]):
            total += accumulator(gpu_ctx, hip, ragged.pk, b, e, shape, ragged.vbg, c.A, c.v0, (3, 0))
        assert np.array_equal(total, whole), cuts


@pytest.mark.parametrize("first_closed", [0, 1])
def test_records_belong_to_the_handle(first_closed, ragged, gpu_ctx):
    """Two handles of different width on one set, alive together, closed in either order; a third one afterwards."""
    c = ragged.c
    ss = bm.SeqSet(gpu_ctx, ragged.pk)
    widths = (14, 20)
    ems = [mixed_em(gpu_ctx, ss, c, ragged.vbg, W=w) for w in widths]
    for em in ems:                                           # both created before either runs
        em.iterate(1)
    for em, w in zip(ems, widths):
        np.testing.assert_allclose(em.getV(), ragged.v64(w), rtol=1e-6, atol=1e-9)
    ems[first_closed].close()
    other = ems[1 - first_closed]
    third = mixed_em(gpu_ctx, ss, c, ragged.vbg, W=17)       # takes over the closed handle's scratch
    other.iterate(1)                                         # the survivor's records are intact
    third.iterate(1)
    np.testing.assert_allclose(third.getV(), ragged.v64(17), rtol=1e-6, atol=1e-9)
    fresh = mixed_em(gpu_ctx, ss, c, ragged.vbg, W=widths[1 - first_closed])
    fresh.iterate(1); fresh.iterate(1)
    assert np.array_equal(other.getV(), fresh.getV())
    for em in (other, third, fresh):
        em.close()
    ss.close()
