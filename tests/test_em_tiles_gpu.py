"""EM passes over sequences beyond 8192 positions tile by tile (csrc/em_tiles.hip: k_em_tile, k_em_tile_norm) against
the references, against the window-by-window path of the same library (em_tiles=0: k_long_em, csrc/long_seq.hip) and
against themselves.

What is exact and what is not: a window's product, pos_i, the r expression and the 2^-40 conversion are the operations of
k_long_em in the same order, so given the same 1/Z they give the same bits.  Z is in both paths a double sum of the same
fp32 terms rounded once to fp32, in another order: the double sums differ by about n * 2^-53 relative, so the two Z are
equal except within that distance of a rounding boundary, and then 1 ulp apart; 1/Z then at most about 2 ulps, r at most
about 3 ulps = 3 * 2^-23 < 2^-21 relative.  Hence r (tiles) against r (em_tiles=0) at rtol 2^-21 (R_ATOL for
denormals), the counts at rtol 2^-21 with atol = (windows of the set) * 2^-40 (an addend next to the 2^-40 threshold may
flip between 0 and one unit, which is also why the zero patterns of the two paths are not compared).  A sequence's Z
depends on its own tiles only, so everything the tile path computes is bit-identical across launch geometries, shards,
masks, callers and runs.

Sets hold at most 6 records of at most about 12 300 positions (the shapes taken from tests/test_long_gpu.py excepted); a
record is long from 8193 positions on, four tiles of the geometry and more."""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth
from tests.cases import Case
from tests.test_long_gpu import LONG_CASES
from tests.test_parity_gpu import LLH_RTOL, R_ATOL, V_RTOL
from tests.test_sites_gpu import check as check_sites

pytestmark = pytest.mark.gpu

LONG = 8192                                               # BAMM_MAX_SEQ_POSITIONS
R_TILE_RTOL = 2.0 ** -21                                  # 3 ulps of fp32, see above


def bases(n, seed):
    return np.random.RandomState(seed).randint(1, 5, size=int(n)).astype(np.uint8)


class TileSet:
    """One set (a list of code arrays, 0 = N) encoded by the oracle and resident on the device, with a seed model."""

    def __init__(self, ctx, orc, records, ss, K, W, bg_order=2, q=0.3, v0=None):
        self.ctx, self.orc, self.ss, self.K, self.W, self.bg_order, self.q = ctx, orc, ss, K, W, bg_order, q
        in_off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
        _, self.kmer, self.off = orc.encode_set(np.concatenate(records), in_off, ss, 42)
        self.lens = np.diff(self.off.astype(np.int64))
        self.vbg = orc.bg_model(self.kmer, self.off, bg_order, np.array([1.0] + [10.0] * bg_order, np.float32))
        self.A = synth.alpha_matrix(synth.default_alpha(K), W)
        self.v0 = v0 if v0 is not None else synth.bamm_from_pwm((0.7 * synth.make_pwm(W, 3) + 0.075).astype(np.float32), K)
        self.pk = bm.PackedSeqs.from_kmers(self.kmer, self.off)
        self.seqs = bm.SeqSet(ctx, self.pk)
        self.cells = 4 ** (K + 1) * W
        self.windows = int((self.lens - W + 1).sum())

    @classmethod
    def from_case(cls, ctx, orc, c):
        records = [c.codes[int(a):int(b)] for a, b in zip(c.in_off[:-1], c.in_off[1:])]
        return cls(ctx, orc, records, c.ss, c.K, c.W, c.bg_order, c.q, c.v0)

    def em(self, tiles=True, seqs=None, **kw):
        """a handle on the set (or on `seqs`) created under em_tiles = tiles; the context is left at the default"""
        self.ctx.set_tuning(em_tiles=1 if tiles else 0)
        try:
            return bm.EM(self.ctx, seqs if seqs is not None else self.seqs, self.K, self.W, self.vbg, self.A, self.v0, self.q,
                         bg_order=self.bg_order, **kw)
        finally:
            self.ctx.set_tuning(em_tiles=1)

    def expected_plan(self, in_envelope=True):
        tp, stride = bm.em_tile_geometry(self.W)
        long_ = self.lens > LONG
        if not in_envelope:
            return dict(tiled_seqs=0, tiles=0, window_seqs=int(long_.sum()))
        return dict(tiled_seqs=int(long_.sum()), tiles=int(sum(-(-(L - self.W + 1) // stride) for L in self.lens[long_])), window_seqs=0)

    def close(self):
        self.seqs.close()


_hip = None


def raw(ctx, em):
    """the pass's integer accumulator after one accumulating pass: [cells | llh | sum r | sequences] (as
    tests/test_long_gpu.py::test_long_and_short_paths_add_the_same_integers reads it)"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    em.accumulate()
    ctx.sync()
    p, n = em.reduce_buffer()
    h = np.zeros(n, np.int64)
    assert _hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(p), n * 8, 2) == 0
    return h


def check_references(ts, oracle_rtol=None):
    """tiles on: one iterate() against the fp64 restatement, EStep / getR / getLLH / MStep against the fp32 oracle at the
    bars of tests/test_long_gpu.py (oracle_rtol: the oracle's own error where it exceeds those bars, see the W = 1 case)"""
    orc, K, W = ts.orc, ts.K, ts.W
    Kb = min(ts.bg_order, K)
    em = ts.em()
    plan = em.tile_plan()
    assert plan == ts.expected_plan() and plan["tiled_seqs"] > 0, (plan, ts.expected_plan())
    # the oracle sums Z sequentially in fp32 (EM.cpp:179-182): over >10^4 windows that sum is itself ~1e-5 off
    long_tol = max(1.0, 4e-4 * ts.lens.max() / (1 if ts.ss else 2))
    if oracle_rtol is not None:
        long_tol = max(long_tol, oracle_rtol / 1e-5)
    v, q = em.getV(), em.getQ()
    em.EStep()
    s_o = orc.linear_s(v, ts.vbg, K, W, Kb)
    r_o, llh_o = orc.estep(ts.kmer, ts.off, K, W, s_o, q)
    np.testing.assert_allclose(em.getR(), r_o, rtol=1e-5 * long_tol, atol=R_ATOL)
    # llh: that file's bar against the fp64 restatement.  The fp32 oracle's own llh carries its Z's summation error -- on sets
    # of three records of 10^4 positions the two CPU references are 6.6e-5 (K = 3, W = 20) and 2.6e-4 (W = 1) apart, more than
    # the bar -- so against it the bar is widened by exactly the distance between the two references, the device not involved.
    v64, _, llh64, _ = orc.em_step_f64(ts.kmer, ts.off, K, W, ts.bg_order, ts.vbg, ts.A, v, q)
    llh_atol = 2e-9 * float(ts.off[-1])
    print(f"llh: device {em.getLLH():.9g}, fp64 restatement {llh64:.9g}, fp32 oracle {llh_o:.9g}")
    np.testing.assert_allclose(em.getLLH(), llh64, rtol=LLH_RTOL, atol=llh_atol)
    np.testing.assert_allclose(em.getLLH(), llh_o, rtol=LLH_RTOL, atol=llh_atol + abs(llh_o - llh64))
    em.MStep()
    n_o = orc.mstep_counts(ts.kmer, ts.off, K, W, r_o)
    np.testing.assert_allclose(em.getCounts(), n_o, rtol=1e-5 * long_tol, atol=1e-6)
    np.testing.assert_allclose(em.getV(), orc.update_v(n_o, ts.A, ts.vbg, K, W), rtol=V_RTOL * long_tol, atol=1e-9)
    em.close()
    em = ts.em()                                          # (v, q above are the seed's: v64 is the fresh handle's first step)
    em.iterate(1)
    np.testing.assert_allclose(em.getV(), v64, rtol=1e-6, atol=1e-9)
    em.close()


def check_against_windows(ts):
    """the same set through two handles, tiles and em_tiles=0"""
    et, ew = ts.em(True), ts.em(False)
    assert ew.tile_plan() == ts.expected_plan(in_envelope=False)
    ht, hw = raw(ts.ctx, et), raw(ts.ctx, ew)
    unit = 2.0 ** -40                                     # sets this small count in units of 2^-40
    np.testing.assert_allclose(ht[:ts.cells] * unit, hw[:ts.cells] * unit, rtol=R_TILE_RTOL, atol=ts.windows * unit)
    assert ht[ts.cells + 2] == hw[ts.cells + 2] == len(ts.lens)
    et.EStep()
    ew.EStep()
    rt, rw = et.getR(), ew.getR()
    print(f"r tiles / windows: {int((rt != rw).sum())} of {len(rt)} differ, max rel {np.max(np.abs(rt - rw) / np.maximum(np.abs(rw), 1e-30)):.3g}")
    np.testing.assert_allclose(rt, rw, rtol=R_TILE_RTOL, atol=R_ATOL)
    np.testing.assert_allclose(et.getLLH(), ew.getLLH(), rtol=LLH_RTOL)
    et.close()
    ew.close()


def check_both(ts, oracle_rtol=None):
    check_references(ts, oracle_rtol)
    check_against_windows(ts)
    ts.close()


# ---- 1. the plan ----------------------------------------------------------------------------------------------------
def plan_records(W):
    tp, stride = bm.em_tile_geometry(W)
    return [bases(LONG + 1, 1), bases(300, 2), bases(5 * stride + 5, 3), bases(max(W, 40), 4)]


@pytest.mark.parametrize("K,W,ss", [(2, 12, True), (0, 1, True), (3, 20, True), (1, 9, False)])
def test_plan_in_the_envelope(gpu_ctx, orc, K, W, ss):
    records = plan_records(W) if ss else [bases(LONG // 2 + 40, 1), bases(300, 2), bases(5000, 3)]
    ts = TileSet(gpu_ctx, orc, records, ss, K, W)
    assert (ts.lens > LONG).sum() >= 1 and (ts.lens <= LONG).sum() >= 1
    on, off = ts.em(True), ts.em(False)
    assert on.tile_plan() == ts.expected_plan()
    assert on.tile_plan()["tiles"] >= 4 * on.tile_plan()["tiled_seqs"] > 0
    assert off.tile_plan() == ts.expected_plan(in_envelope=False)
    assert on.plan()[2] == off.plan()[2] and on.plan_paths()[2] == off.plan_paths()[2] == int((ts.lens > LONG).sum())
    for x in (on, off, ts):
        x.close()


@pytest.mark.parametrize("K,W", [(4, 30), (7, 6)])
def test_plan_outside_the_envelope(gpu_ctx, orc, K, W):
    """a sliced handle and one whose tables stay in global memory (every sequence in the long class) keep k_long_em"""
    ts = TileSet(gpu_ctx, orc, [bases(LONG + 1, 1), bases(300, 2)], True, K, W)
    on, off = ts.em(True), ts.em(False)
    n_window = 1 if K == 4 else 2
    assert on.plan_paths()[0] == (K == 4)
    for em in (on, off):
        assert em.tile_plan() == dict(tiled_seqs=0, tiles=0, window_seqs=n_window)
        assert em.plan_paths()[2] == n_window
    assert on.plan()[2] == off.plan()[2]
    for x in (on, off, ts):
        x.close()


# ---- 2. / 3. the shapes of tests/test_long_gpu.py inside the envelope (k = 4 is sliced), and (3, 20) ----------------------
SHAPES = [d for d in LONG_CASES if d["name"] != "long_k4_sliced"] + [
    dict(name="long_k3_w20", N=4, L0=9600, W=20, K=3, ss=True, ragged=1600, n_frac=0.0005)]


@pytest.mark.parametrize("spec", SHAPES, ids=[d["name"] for d in SHAPES])
def test_shapes_against_the_references_and_the_window_path(spec, gpu_ctx, orc):
    ts = TileSet.from_case(gpu_ctx, orc, Case(**spec))
    assert ts.lens.max() > LONG
    check_both(ts)


# ---- 4. edges ---------------------------------------------------------------------------------------------------------
def first_long_boundary(stride):
    return (LONG // stride + 1) * stride                  # the first tile boundary a long record reaches


@pytest.mark.parametrize("K,W", [(2, 12), (0, 1), (3, 20)])
def test_lw1_on_a_tile_boundary(gpu_ctx, orc, K, W):
    """L - W + 1 = b - 1, b, b + 1: the last tile full but for one window, full, and a further tile that owns one window"""
    tp, stride = bm.em_tile_geometry(W)
    b = first_long_boundary(stride)
    ts = TileSet(gpu_ctx, orc, [bases(b - 1 + W - 1, 11), bases(b + W - 1, 12), bases(b + 1 + W - 1, 13), bases(300, 14)], True, K, W)
    assert ts.expected_plan()["tiles"] == 3 * (b // stride) + 1
    # W = 1, K = 0: a record's 10^4 terms take four values of one size, and the oracle's sequential fp32 sum of them (EM.cpp:
    # 179-182) drifts one way: its Z is 1.4e-4 off the double sum of the same terms on the second record here (measured on
    # the CPU, no device involved), beyond the 4e-5 of the other shapes' bar.  The bar for this shape is the textbook bound
    # of a recursive sum, n * 2^-24 relative; the fp64 restatement and the window path below keep their own bars.
    check_both(ts, oracle_rtol=float(ts.lens.max()) * 2.0 ** -24 if W == 1 else None)


def test_strand_junction_on_a_tile_boundary(gpu_ctx, orc):
    """both strands: the separator (position = input length) at b - 1, b and b + K for a tile boundary b"""
    K, W = 2, 12
    tp, stride = bm.em_tile_geometry(W)
    k = 1
    while 2 * (k * stride - 1) + 1 <= LONG:
        k += 1
    b = k * stride
    ts = TileSet(gpu_ctx, orc, [bases(b - 1, 21), bases(b, 22), bases(b + K, 23), bases(150, 24)], False, K, W)
    assert (ts.lens[:3] > LONG).all()
    check_both(ts)


def test_isolated_n_on_the_tile_edges(gpu_ctx, orc):
    K, W = 2, 12
    tp, stride = bm.em_tile_geometry(W)
    t0 = stride                                           # the second tile's first position
    L = max(LONG + 1, tp + 100)
    spots = [t0 - 1, t0, t0 + K, stride + W - 2, tp - 1]  # ..., the last position the first tile's windows use, the last of its overlap
    records = []
    for i, p in enumerate(spots):
        r = bases(L + i, 31 + i)
        r[p] = 0
        records.append(r)
    every = bases(L, 41)                                  # all of them in one record, and again one tile further on
    for p in spots:
        every[p] = 0
        every[p + stride] = 0
    check_both(TileSet(gpu_ctx, orc, records + [every], True, K, W))


def test_a_tile_inside_a_run_of_n_and_n_beyond_the_last_window(gpu_ctx, orc):
    K, W = 2, 12
    tp, stride = bm.em_tile_geometry(W)
    a = stride - 25                                       # the run [a, a + tp + 50) holds the whole second tile
    run = bases(max(LONG + 1, a + tp + 50 + 200), 51)
    run[a:a + tp + 50] = 0
    tail = bases(LONG + 60, 52)                           # N at positions >= LW1 = L - W + 1, which take no part ...
    tail[[len(tail) - 1, len(tail) - W + 1]] = 0
    last = bases(LONG + 61, 53)                           # ... and at LW1 - 1, the last window's first position, which does
    last[len(last) - W] = 0
    check_both(TileSet(gpu_ctx, orc, [run, tail, last, bases(300, 54)], True, K, W))


@pytest.mark.parametrize("lengths", [[LONG + 1, LONG + 700, 9000], [200, 9100, 300, 64, 500]], ids=["every_record_long", "one_long_among_short"])
def test_sets_all_long_and_one_long(gpu_ctx, orc, lengths):
    check_both(TileSet(gpu_ctx, orc, [bases(L, 61 + i) for i, L in enumerate(lengths)], True, 2, 12))


# ---- 5. exact invariances of the tile path -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inv(gpu_ctx, orc):
    ts = TileSet(gpu_ctx, orc, [bases(L, 71 + i) for i, L in enumerate([LONG + 9, 300, 500, 9000, 200])], True, 2, 12)
    assert ts.em().tile_plan()["tiled_seqs"] == 2
    yield ts
    ts.close()


def test_shards_add_the_same_integers(inv, gpu_ctx):
    whole = inv.em()
    hw = raw(gpu_ctx, whole)
    whole.close()
    parts = np.zeros_like(hw)
    for begin, end in ((0, 2), (2, 5)):                  # a long record in each shard
        seqs = bm.SeqSet(gpu_ctx, inv.pk, begin, end)
        em = inv.em(seqs=seqs)
        assert em.tile_plan()["tiled_seqs"] == 1
        parts += raw(gpu_ctx, em)
        em.close()
        seqs.close()
    assert np.array_equal(hw, parts)
    assert hw[:inv.cells].sum() > 0 and hw[inv.cells + 2] == 5


def test_launch_geometry_does_not_show(inv, gpu_ctx):
    em = inv.em()
    want = raw(gpu_ctx, em)
    em.EStep()
    want_r = em.getR()
    em.close()
    gpu_ctx.set_launch(blocks=1)
    try:
        em = inv.em()
        got = raw(gpu_ctx, em)
        em.EStep()
        got_r = em.getR()
        em.close()
    finally:
        gpu_ctx.set_launch()
    assert np.array_equal(got, want) and np.array_equal(got_r, want_r)


def test_fold_mask_against_the_subset(inv, gpu_ctx):
    """the mask drops the first long record: the same integers as the set uploaded without it"""
    masked = inv.em(mask=np.array([0, 1, 1, 1, 1], np.uint8))
    assert masked.tile_plan() == inv.expected_plan()       # the tiles are planned without the mask
    hm = raw(gpu_ctx, masked)
    masked.close()
    first = int(inv.off[1])
    pk = bm.PackedSeqs.from_kmers(inv.kmer[first:], inv.off[1:] - inv.off[1])
    seqs = bm.SeqSet(gpu_ctx, pk)
    sub = inv.em(seqs=seqs)
    hs = raw(gpu_ctx, sub)
    sub.close()
    seqs.close()
    assert np.array_equal(hm, hs) and hm[inv.cells + 2] == 4


def test_getr_ranges_and_sites(inv):
    em = inv.em()
    em.iterate(2)
    em.EStep()
    whole = em.getR()
    per_record = np.concatenate([em.getR(n, n + 1) for n in range(len(inv.lens))])
    assert np.array_equal(whole, per_record)
    assert np.array_equal(em.getR(3, 5), whole[int(inv.off[3]):])
    check_sites(em, inv.lens, inv.W)
    check_sites(em, inv.lens, inv.W, 3, 4, cutoffs=(0.3, 0.0))
    em.close()


def test_runs_repeat_and_optimize_stops_where_iterate_does(inv):
    a, b = inv.em(), inv.em()
    a.iterate(3)
    b.iterate(3)
    assert np.array_equal(a.getV(), b.getV()) and a.getLLH() == b.getLLH() and a.getQ() == b.getQ()
    a.close()
    b.close()
    opt = inv.em(epsilon=0.05, max_iterations=40)
    n = opt.optimize()
    assert 1 <= n <= 40
    it = inv.em(epsilon=0.05, max_iterations=40)
    it.iterate(n)
    assert opt.iteration() == it.iteration() == n
    assert np.array_equal(opt.getV(), it.getV()) and opt.getLLH() == it.getLLH()
    opt.close()
    it.close()


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------
def test_a_tiled_handle_returns_its_blocks(inv):
    before = bm.device_blocks_live()
    em = inv.em()
    assert em.tile_plan()["tiles"] > 0
    em.iterate(1)
    em.EStep()
    em.getR(0, 1)
    assert bm.device_blocks_live() > before
    em.close()
    assert bm.device_blocks_live() == before
