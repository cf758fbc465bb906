"""Log-odds tables beyond one CU's LDS through the register-resident scorer, a slice of motif columns per launch
(csrc/scorer.hip: k_score_slice, k_score_tile_slice, which go on with the one score_chain where the slice before them
stopped; bamm_ctx_set_tuning "score_slices").  Every case is scored three ways -- score_slices=1, score_slices=0 (the
window-by-window scorer of long_seq.hip, today's route for such tables) and the CPU oracle's log-odds -- and mops, zoops
and z must be equal element for element; bamm_score_plan must report the routing by length under 1 and window_seqs under 0.

Models: the first sliced width of each order (K = 5, W = 10: 2 x 5 columns; K = 4, W = 40; K = 6, W = 3: slices of 2 and 1
columns), six slices (K = 6, W = 12), a table that fits whole (K = 5, W = 9: the key changes nothing) and one of which no
column fits (K = 7, W = 4: window by window whatever the key says).  Records: the edges of k_score's length classes, the
lengths around the tile boundaries that test_score_tiles_gpu.py uses, both strands, N at the ends and inside, and records
made of one 64-base unit, whose maxima recur.  A set holds at most 15 records of at most about 12 300 positions."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth
from tests.test_score_tiles_gpu import LONG, Scored, bases, geometry

pytestmark = pytest.mark.gpu

LDS = 160 * 1024
MODELS = [(5, 10), (5, 9), (4, 40), (6, 3), (6, 12), (7, 4)]


class Sliced(Scored):
    """Scored, with the key under test: the context is left as the library creates it (score_slices=0)."""

    def gpu(self, slices, **kw):
        self.ctx.set_tuning(score_slices=1 if slices else 0)
        try:
            return bm.logodds(self.ctx, self.seqs, self.K, self.W, self.bg_order, self.v, self.vbg, **kw)
        finally:
            self.ctx.set_tuning(score_slices=0)

    def plan(self, slices):
        self.ctx.set_tuning(score_slices=1 if slices else 0)
        try:
            return bm.score_plan(self.ctx, self.seqs, self.K, self.W)
        finally:
            self.ctx.set_tuning(score_slices=0)

    def expected_plan(self, slices=False):
        tp, stride = geometry(self.W)
        lds = self.W * (4 ** (self.K + 1) + 1) * 4 <= LDS or (slices and self.K <= 6)   # from order 7 on no column fits
        long_ = self.lens > LONG
        tiled = int(long_.sum()) if lds else 0
        tiles = int(sum(-(-(L - self.W + 1) // stride) for L in self.lens[long_])) if lds else 0
        windows = 0 if lds else len(self.lens)
        return dict(wave_seqs=len(self.lens) - tiled - windows, tiled_seqs=tiled, tiles=tiles, window_seqs=windows)

    def check(self):
        """slices == score_slices=0 == oracle, and the plan says who went where under either value of the key"""
        for slices in (True, False):
            assert self.plan(slices) == self.expected_plan(slices), (slices, self.plan(slices), self.expected_plan(slices))
        got, plain = self.gpu(True), self.gpu(False)
        for name, g, p, o in zip(("mops", "zoops", "z"), got, plain, self.oracle):
            bad = np.nonzero(g != o)[0]
            assert np.array_equal(g, o), f"{name}: slices differ from the oracle at {bad[:8]} (of {len(bad)})"
            assert np.array_equal(p, o), f"{name}: score_slices=0 differs from the oracle"
        for slices in (True, False):                          # without mops the carrier is a block of the (poisoned) scratch pool
            none, zoops, z = self.gpu(slices, want_mops=False)
            assert none is None and np.array_equal(zoops, self.oracle[1]) and np.array_equal(z, self.oracle[2]), slices
        return got

    def check_masks(self):
        """every sequence left out once, members of every route in and out: what is left out stays zero"""
        for first in (0, 1):
            mk = ((np.arange(len(self.lens)) + first) % 2).astype(np.uint8)
            want = [a.copy() for a in self.oracle]
            for n in np.nonzero(mk == 0)[0]:
                want[0][self.moff[n]:self.moff[n + 1]] = 0
                want[1][n] = 0
                want[2][n] = 0
            for slices in (True, False):
                got = self.gpu(slices, mask=mk)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (first, slices)
                none, zoops, z = self.gpu(slices, mask=mk, want_mops=False)
                assert none is None and np.array_equal(zoops, want[1]) and np.array_equal(z, want[2]), (first, slices)


def with_n(L, K, seed, ends=True, inside=True):
    """L random bases with runs of N (code 0) at both ends and one of K + 3 in the middle"""
    r = bases(L, seed)
    if ends and L > 16:
        r[:3] = 0
        r[-(K + 2):] = 0
    if inside and L > 64:
        r[L // 2:L // 2 + K + 3] = 0
    return r


def class_edge_records(K, W):
    """a single window, two, the first class's last length and the second's first, ..., the last length of k_score and the
    first of the tiles; then the 64-base unit over and over, in k_score and across tiles"""
    recs = [bases(W, 100), bases(W + 1, 101)]
    recs += [with_n(max(L, W), K, 102 + i, ends=i % 2 == 0) for i, L in enumerate((64, 65, 300, 4096, LONG, LONG + 1))]
    unit = bases(64, 61)
    return recs + [np.tile(unit, 10), np.tile(unit, 130)]      # 640 and 8320 positions


@pytest.mark.parametrize("K,W", MODELS)
def test_length_class_edges_and_recurring_maxima(gpu_ctx, orc, K, W):
    recs = class_edge_records(K, W)
    s = Sliced(gpu_ctx, orc, recs, True, K, W)
    try:
        assert np.array_equal(s.lens, [len(r) for r in recs])
        mops, zoops, z = s.check()
        tp, stride = geometry(W)
        for n in (len(recs) - 2, len(recs) - 1):              # the maximum recurs (in the long record: in several tiles) ...
            at = np.nonzero(mops[s.moff[n]:s.moff[n + 1]] == zoops[n])[0]
            assert len(at) > 1 and z[n] == at[0]              # ... and the lowest window is reported
        assert at[-1] // stride > at[0] // stride
        s.check_masks()
    finally:
        s.close()


@pytest.mark.parametrize("K,W", MODELS)
def test_lengths_around_the_tile_boundaries(gpu_ctx, orc, K, W):
    tp, stride = geometry(W)
    b = (LONG // stride + 1) * stride                         # the first tile boundary a long record reaches
    lengths = [LONG + 1, stride + W - 1, stride + W, 300, 3 * stride + 5, 2 * stride, 2 * stride + 1, tp, tp + 1,
               b + W - 1, b + W, b, b + 1]
    s = Sliced(gpu_ctx, orc, [with_n(L, K, 11 + i, ends=i % 3 == 0, inside=i % 2 == 0) for i, L in enumerate(lengths)], True, K, W)
    try:
        plan = s.plan(True)
        assert K > 6 or (plan["tiled_seqs"] >= 5 and plan["tiles"] > plan["tiled_seqs"])
        s.check()
        s.check_masks()
    finally:
        s.close()


@pytest.mark.parametrize("K,W", MODELS)
def test_both_strands(gpu_ctx, orc, K, W):
    """2 * L + 1 positions per record, the separator inside: 4096 bases make the first long record"""
    inputs = [max(W, 20), 150, 2100, LONG // 2, 5000]
    s = Sliced(gpu_ctx, orc, [with_n(L, K, 31 + i, ends=i % 2 == 1) for i, L in enumerate(inputs)], False, K, W)
    try:
        assert np.array_equal(s.lens, [2 * L + 1 for L in inputs]) and (s.lens > LONG).sum() == 2
        s.check()
        s.check_masks()
    finally:
        s.close()


def test_callers_inherit_the_slices(gpu_ctx, orc):
    """bamm_occurrences and bamm_fdr_add_set score through the same planner: every array equal to the score_slices=0 run"""
    K, W = 5, 10
    s = Sliced(gpu_ctx, orc, [bases(LONG + 700, 81), bases(300, 82), bases(LONG + 1, 83), bases(200, 84)], True, K, W)
    assert s.plan(True) == s.expected_plan(True) and s.plan(True)["tiled_seqs"] == 2 and s.plan(False)["window_seqs"] == 4
    ncodes, noff = synth.make_sequences(200, 200, synth.make_pwm(W, 4), 8, 0.0, 0.0, 0)
    neg = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_codes(ncodes, noff, True, seed=42))
    res = {}
    for slices in (1, 0):
        gpu_ctx.set_tuning(score_slices=slices)
        try:
            occ = bm.occurrences(gpu_ctx, s.seqs, neg, K, W, 2, s.v, s.vbg, 0.05)
            f = bm.FdrMops(gpu_ctx)
            try:
                f.add_set(False, s.seqs, K, W, 2, s.v, s.vbg)
                f.add_set(True, neg, K, W, 2, s.v, s.vbg)
                f.statistics(3, 200, True)
                res[slices] = (occ, f.info(), f.rows(), f.pvalues())
            finally:
                f.close()
        finally:
            gpu_ctx.set_tuning(score_slices=0)
    (oa, ia, ra, pa), (ob, ib, rb, pb) = res[1], res[0]
    assert oa.n_hits > 0
    for name in ("seq", "pos", "score", "fp", "p", "e"):
        assert np.array_equal(getattr(oa, name), getattr(ob, name)), name
    assert (oa.n_neg_scores, oa.n_top, oa.s_ntop, oa.lambda_, oa.n_candidates) == (ob.n_neg_scores, ob.n_top, ob.s_ntop, ob.lambda_, ob.n_candidates)
    assert ia == ib and ia["n_pos"] == int(s.moff[-1])
    assert all(np.array_equal(ra[k], rb[k]) for k in ra) and np.array_equal(pa, pb)
    neg.close()
    s.close()
