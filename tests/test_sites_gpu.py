"""bamm_em_sites (csrc/sites.hip, csrc/sites.cpp) against the same handle's getR(): the windows with r >= cut-off, and
every sequence's best window, derived from the downloaded r in numpy must EQUAL what the device lists -- both read the same
r bits, so there is no tolerance anywhere in this file except against the reference's own r (the last test)."""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi
from tests import golden_util as gu
from tests.cases import Case

pytestmark = pytest.mark.gpu
CUTOFFS = (0.3, 1e-4, 0.0, 2.0)


def derive(r, lens, W, cutoff, begin=0):
    """(seq, pos, r), (z, r_best, count) from flat r in the reference's layout (window start i at L-W-i): EM.cpp:585-592
    for the sites, GibbsSampling.cpp:105-116 for z (strict `>` from 0, i ascending: the first maximum)."""
    seq, pos, val = [], [], []
    z, best, count = np.zeros(len(lens), np.uint32), np.zeros(len(lens), np.float32), np.zeros(len(lens), np.uint32)
    o = 0
    for n, L in enumerate(int(x) for x in lens):
        v = r[o + L - W - np.arange(L - W + 1)]
        hit = np.flatnonzero(v >= np.float32(cutoff))
        seq.append(np.full(len(hit), begin + n, np.uint64)); pos.append(hit.astype(np.uint32)); val.append(v[hit])
        count[n] = len(hit)
        if v.max() > 0:
            z[n], best[n] = int(np.argmax(v)) + 1, v.max()
        o += L
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return (cat(seq, np.uint64), cat(pos, np.uint32), cat(val, np.float32)), (z, best, count)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, what):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


def check(em, lens, W, begin=0, end=None, cutoffs=CUTOFFS, posterior=True):
    """Every cut-off against ONE download of r; returns the per-cut-off device results.  posterior: every r is a
    probability, so 2.0 lists nothing (EM::mask's r_ is not: EM.cpp:423-427 divides r_[n][0] by the norm once more than
    the others and leaves the unlisted windows at what the order-0 pass wrote, and getR() reports it so)."""
    end = len(lens) if end is None else end
    r = em.getR(begin, end)
    out = {}
    for cut in cutoffs:
        want_sites, want_best = derive(r, lens[begin:end], W, cut, begin)
        sites, best = em.sites_and_best(cut, begin, end)
        assert_same(sites, want_sites, ("seq", "pos", "r"))
        assert_same(best, want_best, ("z", "r_best", "count"))
        assert int(best[2].sum()) == len(sites[0])
        out[cut] = (sites, best)
    if 0.0 in out:
        assert len(out[0.0][0][0]) == int((lens[begin:end].astype(np.int64) - W + 1).sum())
    if 2.0 in out and posterior:
        assert len(out[2.0][0][0]) == 0
    return out


def make(gpu_ctx, c, mask=None, ss=None, **tune):
    pk = bm.PackedSeqs.from_codes(c.codes, c.in_off, c.ss, seed=42)
    ss = bm.SeqSet(gpu_ctx, pk) if ss is None else ss
    vbg = pk.bg_model(c.bg_order, c.alpha_bg)
    reset = {"group_layout": -1, "grouped": 1, "e_fused": 1}
    gpu_ctx.set_tuning(**tune)
    try:
        em = bm.EM(gpu_ctx, ss, c.K, c.W, vbg, c.A, c.v0, c.q, bg_order=c.bg_order, mask=mask)
    finally:
        gpu_ctx.set_tuning(**{k: reset[k] for k in tune})
    return ss, em


@pytest.fixture(scope="module")
def bench_shape():
    return Case("sites_k2", N=300, L0=200, W=20, K=2, n_frac=0.002)


@pytest.mark.parametrize("tune", [{}, {"group_layout": 8}, {"group_layout": 3}, {"grouped": 0}],
                         ids=["planner", "k_em_mix", "k_em_grp", "k_em_seq"])
def test_fused_kernel_flavours(tune, bench_shape, gpu_ctx):
    c = bench_shape
    ss, em = make(gpu_ctx, c, **tune)
    grouped, other, _ = em.plan()
    if tune.get("group_layout") == 8:
        assert grouped > 0 and em.plan_mixed() == grouped
    if tune.get("group_layout") == 3:
        assert grouped > 0 and em.plan_mixed() == 0
    if "grouped" in tune:
        assert grouped == 0 and other == c.N
    em.iterate(3)
    out = check(em, ss.lengths, c.W)
    # ranks cross strides of 64 windows: at 0.0 in every sequence (382 windows); at 1e-4 this model lists at most some 20
    # windows of a sequence -- the order-0 and K = 4 cases below are the ones with more than 64 there
    assert out[0.0][1][2].min() > 64 and len(out[0.3][0][0]) > 100
    em.close(); ss.close()


def test_single_strand_order_0_unequal_lengths(gpu_ctx):
    c = Case("sites_k0_ss", N=120, L0=60, W=9, K=0, ss=True, n_frac=0.03, ragged=51)    # 11 .. 111 positions
    parts = [c.codes[int(a):int(b)] for a, b in zip(c.in_off[:-1], c.in_off[1:])]
    parts[7] = parts[7][:c.W]                                  # ... and one that is a single window
    c.codes = np.concatenate(parts)
    c.in_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    lens = np.diff(c.in_off.astype(np.int64))
    assert lens.min() == c.W and lens.max() > 100
    assert sum((c.codes[int(a):int(b)] == 0).any() for a, b in zip(c.in_off[:-1], c.in_off[1:])) >= 5
    ss, em = make(gpu_ctx, c)
    em.iterate(3)
    out = check(em, ss.lengths, c.W)
    assert out[0.0][1][2][7] == 1
    assert out[1e-4][1][2].max() > 64                          # more than one stride of hits in one sequence
    em.close(); ss.close()


@pytest.fixture(scope="module")
def sliced_shape():
    """K = 4, W = 30: the odds and count tables together exceed one CU's LDS (the shape of test_parity_gpu.py's
    SLICED_CASES), the odds table alone does not -- so `e_fused` decides between k_em_seq's and k_e_slice's layout of r."""
    return Case("sites_k4_sliced", N=40, L0=150, W=30, K=4, ss=True, ragged=20, n_frac=0.01)


@pytest.mark.parametrize("e_fused", [1, 0], ids=["e_fused", "slot_indexed"])
def test_sliced_path(e_fused, sliced_shape, gpu_ctx):
    c = sliced_shape
    ss, em = make(gpu_ctx, c, e_fused=e_fused)
    _, twin = make(gpu_ctx, c, ss=ss, e_fused=e_fused)
    assert em.plan_paths()[:2] == (True, bool(e_fused)), "not the sliced path / not the layout this case is about"
    em.iterate(3); twin.iterate(3)
    check(em, ss.lengths, c.W)
    check(em, ss.lengths, c.W, 5, 33)
    # the replayed E pass behind the calls above left the pass counters and the model's trajectory alone
    em.iterate(2); twin.iterate(2)
    assert np.array_equal(em.getV().view(np.uint32), twin.getV().view(np.uint32))
    assert em.iteration() == twin.iteration() == 5
    em.close(); twin.close(); ss.close()


def test_order_4_in_one_kernel(gpu_ctx):
    """K = 4, W = 12 fits the LDS: k_em_seq, not sliced; more than a stride of hits per sequence at 1e-4."""
    c = Case("sites_k4", N=64, L0=150, W=12, K=4, n_frac=0.002)
    ss, em = make(gpu_ctx, c)
    assert em.plan_paths()[0] is False and em.plan()[0] == 0
    em.iterate(3)
    out = check(em, ss.lengths, c.W)
    assert out[1e-4][1][2].max() > 64
    em.close(); ss.close()


def test_after_mask(bench_shape, gpu_ctx):
    c = bench_shape
    ss, em = make(gpu_ctx, c)
    em.mask(0.05)
    check(em, ss.lengths, c.W, posterior=False)
    check(em, ss.lengths, c.W, 17, 230, posterior=False)
    em.close(); ss.close()


@pytest.fixture(scope="module")
def long_mixed():
    """One single-strand sequence of more than 8192 positions among short ones."""
    c = Case("sites_long", N=12, L0=150, W=12, K=2, ss=True, ragged=40, n_frac=0.001, seed=5)
    rs = np.random.RandomState(3)
    long_codes = rs.randint(1, 5, size=9100).astype(np.uint8)
    lens = np.diff(c.in_off.astype(np.int64))
    parts = [c.codes[int(c.in_off[n]):int(c.in_off[n + 1])] for n in range(c.N)]
    parts.insert(4, long_codes)
    c.codes = np.concatenate(parts)
    c.in_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    c.N += 1
    assert lens.max() < 8192
    return c


def test_sequence_beyond_8192_positions(long_mixed, gpu_ctx):
    c = long_mixed
    ss, em = make(gpu_ctx, c)
    assert em.plan_paths()[2] == 1, "the 9100-position sequence is not on the window-by-window path (long_seq.hip)"
    em.iterate(3)
    out = check(em, ss.lengths, c.W)
    assert out[0.0][1][2][4] == 9100 - c.W + 1
    # a budget far below the long sequence: it forms a chunk of its own, the short ones around it are grouped
    gpu_ctx.set_tuning(sites_chunk_positions=1000)
    try:
        for cut in CUTOFFS:
            sites, best = em.sites_and_best(cut)
            assert_same(sites, out[cut][0], ("seq", "pos", "r"))
            assert_same(best, out[cut][1], ("z", "r_best", "count"))
    finally:
        gpu_ctx.set_tuning(sites_chunk_positions=0)
    em.close(); ss.close()


def test_seq_mask_still_reports(bench_shape, gpu_ctx):
    c = bench_shape
    mask = (np.arange(c.N) % 3 != 0).astype(np.uint8)
    ss, em = make(gpu_ctx, c, mask=mask)
    em.iterate(3)
    out = check(em, ss.lengths, c.W)
    assert (out[0.0][1][2][mask == 0] == ss.lengths[mask == 0] - c.W + 1).all()
    em.close(); ss.close()


def test_sub_ranges_chunks_repeatability_and_handle_state(bench_shape, gpu_ctx):
    c = bench_shape
    ss, em = make(gpu_ctx, c)
    _, twin = make(gpu_ctx, c, ss=ss)
    em.iterate(3); twin.iterate(3)
    whole = check(em, ss.lengths, c.W)
    for begin, end in ((7, c.N), (0, 201), (33, 34), (150, 150)):
        part = check(em, ss.lengths, c.W, begin, end)
        for cut in CUTOFFS:
            keep = (whole[cut][0][0] >= begin) & (whole[cut][0][0] < end)          # sequence indices are absolute
            assert_same(part[cut][0], tuple(a[keep] for a in whole[cut][0]), ("seq", "pos", "r"))
            assert_same(part[cut][1], tuple(a[begin:end] for a in whole[cut][1]), ("z", "r_best", "count"))
    empty = em.sites(0.3, 150, 150), em.best_sites(150, 150)
    assert all(len(a) == 0 for pair in empty for a in pair)
    # many chunks of whole sequences (401 positions each, two per chunk) give the arrays of the one-chunk call
    gpu_ctx.set_tuning(sites_chunk_positions=1000)
    try:
        for cut in CUTOFFS:
            sites, best = em.sites_and_best(cut)
            assert_same(sites, whole[cut][0], ("seq", "pos", "r"))
            assert_same(best, whole[cut][1], ("z", "r_best", "count"))
        assert_same(em.sites(1e-4, 7, 298), tuple(a[(whole[1e-4][0][0] >= 7) & (whole[1e-4][0][0] < 298)] for a in whole[1e-4][0]),
                    ("seq", "pos", "r"))
    finally:
        gpu_ctx.set_tuning(sites_chunk_positions=0)
    # two calls in a row
    assert_same(em.sites(1e-4), em.sites(1e-4), ("seq", "pos", "r"))
    assert_same(em.best_sites(), em.best_sites(), ("z", "r_best", "count"))
    # the calls above left no trace in the model's trajectory
    em.iterate(2); twin.iterate(2)
    assert np.array_equal(em.getV().view(np.uint32), twin.getV().view(np.uint32))
    assert em.iteration() == twin.iteration() == 5
    em.close(); twin.close(); ss.close()


def test_errors(bench_shape, gpu_ctx):
    c = bench_shape
    ss, em = make(gpu_ctx, c)
    lib, h = gpu_ctx.lib, C.c_void_p()
    # a handle that has not run an E-step: whatever bamm_em_get_r says about it
    buf = np.zeros(int(ss.off[2]), np.float32)
    rc_r = lib.bamm_em_get_r(em.h, 0, 2, buf, len(buf))
    rc_s = lib.bamm_em_sites(em.h, 0, 2, C.c_float(0.3), C.byref(h))
    assert rc_s == rc_r
    if rc_s == abi.OK:
        check(em, ss.lengths, c.W, 0, 2)
        lib.bamm_sites_destroy(h)
    em.iterate(1)
    assert lib.bamm_em_sites(em.h, 0, c.N, C.c_float(float("nan")), C.byref(h)) == abi.ERR_ARG
    assert lib.bamm_em_sites(em.h, 0, c.N + 1, C.c_float(0.3), C.byref(h)) == abi.ERR_ARG
    assert lib.bamm_em_sites(em.h, 5, 4, C.c_float(0.3), C.byref(h)) == abi.ERR_ARG
    assert lib.bamm_em_get_r(em.h, 0, c.N + 1, buf, len(buf)) == abi.ERR_ARG
    with pytest.raises(bm.abi.BammError):
        em.sites(float("nan"))
    # accessors refuse arrays that are too short
    assert lib.bamm_em_sites(em.h, 0, c.N, C.c_float(0.0), C.byref(h)) == abi.OK
    n_sites, n_seqs = C.c_uint64(), C.c_uint64()
    assert lib.bamm_sites_info(h, C.byref(n_sites), C.byref(n_seqs)) == abi.OK
    assert n_seqs.value == c.N and n_sites.value == int((ss.lengths.astype(np.int64) - c.W + 1).sum())
    assert lib.bamm_sites_get(h, None, None, None, n_sites.value - 1) == abi.ERR_ARG
    assert lib.bamm_sites_best(h, None, None, None, c.N - 1) == abi.ERR_ARG
    assert lib.bamm_sites_get(h, None, None, None, n_sites.value) == abi.OK
    lib.bamm_sites_destroy(h)
    em.close(); ss.close()


GOLDEN_WITH_R = [n for n in gu.fixture_names() if all(f"r_{i}" in np.load(f"{gu.GOLDEN_DIR}/{n}.npz").files for i in range(3))]
NEAR = 2e-5     # twice the suite's flat 1e-5 bar on r: a window this close to the cut-off could fall on either side


@pytest.mark.parametrize("name", GOLDEN_WITH_R)
def test_sites_of_the_reference_own_r(name, gpu_ctx):
    """The replay of test_golden_gpu.py; after each of the three E-steps the sites at 0.3 must be those of the golden r.  No
    golden r lies within NEAR of 0.3 -- asserted from the fixture alone, before anything is compared -- so no window is
    left out of the comparison."""
    c, g = gu.load(name)
    nr = int(g["r_seqs"])
    for it in range(3):
        assert int((np.abs(g[f"r_{it}"].astype(np.float64) - 0.3) <= NEAR).sum()) == 0
    pk = bm.PackedSeqs.from_codes(c.codes, c.in_off, c.ss, seed=42)
    ss = bm.SeqSet(gpu_ctx, pk)
    em = bm.EM(gpu_ctx, ss, c.K, c.W, g["vbg"], c.A, c.v0, c.q, bg_order=c.bg_order)
    for it in range(3):
        em.EStep()
        (w_seq, w_pos, _), (_, _, w_count) = derive(g[f"r_{it}"], ss.lengths[:nr], c.W, 0.3)
        (seq, pos, _), (_, _, count) = em.sites_and_best(0.3, 0, nr)
        assert np.array_equal(seq, w_seq) and np.array_equal(pos, w_pos), f"pass {it + 1}"
        assert np.array_equal(count, w_count)
        em.MStep()
    em.close(); ss.close()
