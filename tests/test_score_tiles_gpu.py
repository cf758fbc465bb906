"""Sequences beyond 8192 positions through the scorer tile by tile (csrc/scorer.hip: k_score_tile, which runs the one score_chain that k_score runs): every case is
scored three ways -- the tiles, the same context with score_tiles=0 (the window-by-window scorer of long_seq.hip) and the
CPU oracle's log-odds -- and mops, zoops and z must be equal element for element.  Tile size and stride come from
bamm_score_tile_geometry; the cases put N, strand junctions, sequence ends and equal maxima on the tile boundaries.

Sets hold at most 6 records.  A record is long from 8193 positions on, which is more than three tiles of the measured
geometry (2048 positions), so the long records here run to the first tile boundary they need: about 12 200 positions at
most, every case well under a second."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth

pytestmark = pytest.mark.gpu

LONG = 8192                                               # BAMM_MAX_SEQ_POSITIONS: longer records leave k_score
ALPHA_BG = np.array([1.0, 10.0, 10.0], np.float32)


def geometry(W):
    return bm.score_tile_geometry(W)


def bases(n, seed):
    return np.random.RandomState(seed).randint(1, 5, size=int(n)).astype(np.uint8)


def model(K, W, seed=3):
    return synth.bamm_from_pwm((0.7 * synth.make_pwm(W, seed) + 0.075).astype(np.float32), K)


class Scored:
    """One set (a list of code arrays, 0 = N) encoded by the oracle, resident on the device, with the oracle's scores."""

    def __init__(self, ctx, orc, records, ss, K, W, bg_order=2):
        self.ctx, self.K, self.W, self.bg_order = ctx, K, W, bg_order
        in_off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
        _, self.kmer, self.off = orc.encode_set(np.concatenate(records), in_off, ss, 42)
        self.lens = np.diff(self.off.astype(np.int64))
        self.vbg = orc.bg_model(self.kmer, self.off, bg_order, ALPHA_BG)
        self.v = model(K, W)
        self.seqs = bm.SeqSet(ctx, bm.PackedSeqs.from_kmers(self.kmer, self.off))
        s_log = orc.log_s(self.v, self.vbg, K, W, min(bg_order, K))
        self.oracle = orc.logodds(self.kmer, self.off, K, W, s_log)
        self.moff = np.concatenate([[0], np.cumsum(self.lens - W + 1)])

    def gpu(self, tiles, **kw):
        self.ctx.set_tuning(score_tiles=1 if tiles else 0)
        try:
            return bm.logodds(self.ctx, self.seqs, self.K, self.W, self.bg_order, self.v, self.vbg, **kw)
        finally:
            self.ctx.set_tuning(score_tiles=1)

    def expected_plan(self):
        tp, stride = geometry(self.W)
        fits = self.W * (4 ** (self.K + 1) + 1) * 4 <= 160 * 1024
        long_ = self.lens > LONG
        tiled = int(long_.sum()) if fits else 0
        tiles = int(sum(-(-(L - self.W + 1) // stride) for L in self.lens[long_])) if fits else 0
        windows = 0 if fits else len(self.lens)
        return dict(wave_seqs=len(self.lens) - tiled - windows, tiled_seqs=tiled, tiles=tiles, window_seqs=windows)

    def check(self, need_tiles=True):
        """tiles == score_tiles=0 == oracle, and the plan says who went where"""
        plan = bm.score_plan(self.ctx, self.seqs, self.K, self.W)
        assert plan == self.expected_plan(), (plan, self.expected_plan())
        if need_tiles:
            assert plan["tiled_seqs"] > 0 and plan["tiles"] > plan["tiled_seqs"]
        self.ctx.set_tuning(score_tiles=0)
        try:
            off_plan = bm.score_plan(self.ctx, self.seqs, self.K, self.W)
        finally:
            self.ctx.set_tuning(score_tiles=1)
        assert off_plan["tiles"] == 0 and off_plan["tiled_seqs"] == 0 and off_plan["window_seqs"] == plan["window_seqs"] + plan["tiled_seqs"]
        got, plain = self.gpu(True), self.gpu(False)
        for name, g, p, o in zip(("mops", "zoops", "z"), got, plain, self.oracle):
            bad = np.nonzero(g != o)[0]
            assert np.array_equal(g, o), f"{name}: tiles differ from the oracle at {bad[:8]} (of {len(bad)})"
            assert np.array_equal(p, o), f"{name}: score_tiles=0 differs from the oracle"
        return got

    def close(self):
        self.seqs.close()


def long_len(stride, more=0):
    """a length that is long and has at least two tiles, `more` beyond"""
    return max(LONG + 1, stride + 200) + more


@pytest.mark.parametrize("K,W", [(0, 1), (2, 12), (4, 30), (0, 30), (4, 1), (2, 30)])
def test_lengths_around_the_tile_boundaries(gpu_ctx, orc, K, W):
    tp, stride = geometry(W)
    b = (LONG // stride + 1) * stride                     # the first tile boundary a long record reaches
    for group in ([LONG + 1, stride + W - 1, stride + W, 300, 3 * stride + 5], [2 * stride, 2 * stride + 1, 300, tp, tp + 1],
                  [b + W - 1, b + W, b, b + 1, 300]):     # ... the last tile full, of one window, and as the lengths before
        s = Scored(gpu_ctx, orc, [bases(max(L, W), 11 + i) for i, L in enumerate(group)], True, K, W)
        s.check(need_tiles=max(group) > LONG)
        s.close()


def test_table_beyond_the_lds_keeps_the_window_scorer(gpu_ctx, orc):
    K, W = 6, 12                                          # 12 * (4^7 + 1) * 4 bytes = 786 KiB
    tp, stride = geometry(W)
    s = Scored(gpu_ctx, orc, [bases(LONG + 1, 1), bases(300, 2)], True, K, W)
    assert bm.score_plan(gpu_ctx, s.seqs, K, W) == dict(wave_seqs=0, tiled_seqs=0, tiles=0, window_seqs=2)
    s.check(need_tiles=False)
    s.close()


def test_single_strand_and_junction_inside_a_tile(gpu_ctx, orc):
    K, W = 2, 12
    tp, stride = geometry(W)
    s = Scored(gpu_ctx, orc, [bases(long_len(stride, 77), 5), bases(300, 6)], True, K, W)
    s.check()
    s.close()
    half = long_len(stride) // 2 + 50                     # both strands: 2 * half + 1 positions, the separator at `half`
    assert half % stride > K + W and half % stride < stride - K - W
    s = Scored(gpu_ctx, orc, [bases(half, 7), bases(150, 8)], False, K, W)
    s.check()
    s.close()


@pytest.mark.parametrize("K,W", [(2, 12), (4, 30)])
def test_junction_on_a_tile_boundary(gpu_ctx, orc, K, W):
    """both strands, the input padded to the length that puts the separator (position = input length) at b - 1, b and
    b + K for a tile boundary b: the junction's exceptions then lie in the one tile, in both, in the other"""
    tp, stride = geometry(W)
    k = 1
    while 2 * (k * stride - 1) + 1 <= LONG:               # the first boundary at which such a record is a long one
        k += 1
    b = k * stride
    s = Scored(gpu_ctx, orc, [bases(b - 1, 21), bases(b, 22), bases(b + K, 23), bases(150, 24)], False, K, W)
    assert (s.lens[:3] > LONG).all()
    s.check()
    s.close()


@pytest.mark.parametrize("K,W", [(2, 12), (4, 30), (0, 1)])
def test_isolated_n_on_the_tile_edges(gpu_ctx, orc, K, W):
    tp, stride = geometry(W)
    t0 = stride                                           # the second tile's first position
    L = max(long_len(stride), tp + 100)
    spots = [t0 - 1, t0, t0 + K, stride + W - 2, tp - 1]  # ..., the last position the first tile's windows use, the last of its overlap with the second
    records = []
    for i, p in enumerate(spots):
        r = bases(L + i, 31 + i)
        r[p] = 0
        records.append(r)
    s = Scored(gpu_ctx, orc, records + [bases(300, 40)], True, K, W)
    s.check()
    s.close()
    every = bases(L, 41)                                  # all of them in one record, and again one tile further on
    for p in spots:
        every[p] = 0
        if p + stride < L:
            every[p + stride] = 0
    s = Scored(gpu_ctx, orc, [every, bases(300, 42)], True, K, W)
    s.check()
    s.close()


def test_a_tile_inside_a_run_of_n(gpu_ctx, orc):
    K, W = 2, 12
    tp, stride = geometry(W)
    a = stride - 25                                       # the run [a, a + tp + 50) holds the whole second tile
    r = bases(max(LONG + 1, a + tp + 50 + 200), 51)
    r[a:a + tp + 50] = 0
    s = Scored(gpu_ctx, orc, [r, bases(300, 52)], True, K, W)
    s.check()
    s.close()


def test_equal_maxima_in_different_tiles(gpu_ctx, orc):
    K, W = 2, 12
    tp, stride = geometry(W)
    unit = bases(64, 61)
    L = long_len(stride, 64)
    s = Scored(gpu_ctx, orc, [np.tile(unit, L // 64 + 1)[:L], bases(300, 62)], True, K, W)
    mops, zoops, z = s.check()
    at = np.nonzero(mops[:s.moff[1]] == zoops[0])[0]
    assert at[-1] // stride > at[0] // stride              # the maximum is reached in more than one tile ...
    assert z[0] == at[0]                                   # ... and the lowest window is reported
    s.close()


def test_masks_and_missing_mops(gpu_ctx, orc):
    K, W = 2, 12
    tp, stride = geometry(W)
    s = Scored(gpu_ctx, orc, [bases(long_len(stride, 3), 71), bases(300, 72), bases(long_len(stride, 40), 73)], True, K, W)
    for mask in ([0, 1, 1], [1, 1, 0], [0, 1, 0], [1, 0, 1]):
        mk = np.array(mask, np.uint8)
        want = [a.copy() for a in s.oracle]
        for n in np.nonzero(mk == 0)[0]:
            want[0][s.moff[n]:s.moff[n + 1]] = 0
            want[1][n] = 0
            want[2][n] = 0
        for tiles in (True, False):
            got = s.gpu(tiles, mask=mk)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (mask, tiles)
    for tiles in (True, False):
        none, zoops, z = s.gpu(tiles, want_mops=False)
        assert none is None and np.array_equal(zoops, s.oracle[1]) and np.array_equal(z, s.oracle[2])
    s.close()


def test_callers_inherit_the_tiles(gpu_ctx, orc):
    """bamm_occurrences and bamm_fdr_add_set score through the same planner: every array equal to the score_tiles=0 run"""
    K, W = 2, 12
    tp, stride = geometry(W)
    s = Scored(gpu_ctx, orc, [bases(long_len(stride, 9), 81), bases(300, 82), bases(long_len(stride, 100), 83)], True, K, W)
    assert bm.score_plan(gpu_ctx, s.seqs, K, W)["tiled_seqs"] == 2
    ncodes, noff = synth.make_sequences(200, 200, synth.make_pwm(W, 4), 8, 0.0, 0.0, 0)
    neg = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_codes(ncodes, noff, True, seed=42))
    res = {}
    for tiles in (1, 0):
        gpu_ctx.set_tuning(score_tiles=tiles)
        try:
            occ = bm.occurrences(gpu_ctx, s.seqs, neg, K, W, 2, s.v, s.vbg, 0.05)
            f = bm.FdrMops(gpu_ctx)
            try:
                f.add_set(False, s.seqs, K, W, 2, s.v, s.vbg)
                f.add_set(True, neg, K, W, 2, s.v, s.vbg)
                f.statistics(3, 200, True)
                res[tiles] = (occ, f.info(), f.rows(), f.pvalues())
            finally:
                f.close()
        finally:
            gpu_ctx.set_tuning(score_tiles=1)
    (oa, ia, ra, pa), (ob, ib, rb, pb) = res[1], res[0]
    assert oa.n_hits > 0
    for name in ("seq", "pos", "score", "fp", "p", "e"):
        assert np.array_equal(getattr(oa, name), getattr(ob, name)), name
    assert (oa.n_neg_scores, oa.n_top, oa.s_ntop, oa.lambda_, oa.n_candidates) == (ob.n_neg_scores, ob.n_top, ob.s_ntop, ob.lambda_, ob.n_candidates)
    assert ia == ib and ia["n_pos"] == int(s.moff[-1])
    assert all(np.array_equal(ra[k], rb[k]) for k in ra) and np.array_equal(pa, pb)
    neg.close()
    s.close()
