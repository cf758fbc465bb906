"""Every M-step flavour at coarse accumulator units (2^-39 .. 2^-24), against the same handle at 2^-40.

bamm_em_params.n_seqs_bound sizes the unit of the int64 accumulator (csrc/em.cpp, bamm_em_create); every accumulating
kernel carries the scale 2^(fix_shift - 40) and every update entry reads the counts back through the unit.  The rest of
the suite runs all of that at the scale 1.  tests/coarse_unit.py says what holds between two units -- exactly per addend,
within the number of addends per cell, word for word on the statistics -- and tests/test_coarse_unit_cpu.py pins the
reference side.  The bound argument alone reaches every code path at the small shapes of tests/regimes.py.

n_seqs_bound also feeds the planner (mixed rows from a size on), so both handles of a pair are created under the same
forced tuning and their plans are compared; regimes' open_em refuses a kernel other than the flavour's.

One deliberate mistake was tried on the GPU build and reverted: fix_scale dropped from k_m_list's conversion
(kernels.hip).  All ten cases of test_sliced_variants_at_a_coarse_unit fail, and the seven cases of
test_integers_at_a_coarse_unit on `sliced` whose second pass takes lists; nothing older does (parity, partition, regimes,
fused update, harvest totals, update blocks, fuzz), since nothing older runs that line with a scale other than 1.

The largest observed ((acc_40 >> d) - acc_s) / m per (flavour, regime, s) goes through margins.check into the session's
parity-margin table (quantity `short / m`, allowed 1; kept in profiles/coarse_unit_margins.txt).
"""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth
from tests import coarse_unit as cu
from tests import margins, regimes
from tests.cases import SMALL_CASES, Case
from tests.test_parity_gpu import make_em
from tests.test_regimes_gpu import open_em

pytestmark = pytest.mark.gpu

FLAVOURS = ["per_column", "layout0_k2_ds_N", "layout2_k2_ds_N", "layout3_k2_ds_N", "grouped_g5", "grouped_k3_odd",
            "mixed_a1", "mixed_a2", "mixed_w20", "sliced", "window_by_window", "order_7", "layout0_k1_ss"]
MORE_UNITS = ["per_column", "layout3_k2_ds_N", "mixed_w20", "sliced"]
INT_CASES = [(f, r, s) for f in FLAVOURS for r in ("R1_context", "R2_sharp") for s in (39, 32, 24)]
INT_CASES += [(f, r, s) for f in MORE_UNITS for r in ("R1_context", "R2_sharp") for s in (33, 31)]

# the sliced path's variants (tests/test_parity_gpu.py::test_sliced_paths_agree_bit_for_bit)
SLICED_TUNINGS = {"list": dict(adaptive_lists=0), "lists_from_pass_2": dict(list_threshold_pct=100), "dense": dict(e_list=0),
                  "e_sliced": dict(e_fused=0)}
SLICED_DEFAULTS = dict(e_list=1, e_fused=1, adaptive_lists=1, list_threshold_pct=45)

_HIP = None
_M: dict = {}
_TOP: dict = {}
_ACC40: dict = {}


def read_accumulator(ctx, em, passes=1):
    """The int64 words of the accumulator after `passes` accumulate() calls on the current model, one array per pass."""
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
    out = []
    for _ in range(passes):
        em.accumulate()
        ctx.sync()
        p, n = em.reduce_buffer()
        h = np.zeros(n, np.int64)
        assert _HIP.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(p), n * 8, 2) == 0
        out.append(h)
    return out


def first_pass(ctx, inp, flavour, bound, tune=None, passes=1):
    """(accumulator per pass, the planner's report) of a fresh handle at this bound."""
    ctx.set_tuning(**(tune or {}))
    try:
        em, ss = open_em(ctx, inp, flavour, n_seqs_bound=bound)
    finally:
        ctx.set_tuning(**{k: SLICED_DEFAULTS[k] for k in (tune or {})})
    plan = (em.plan(), em.plan_mixed(), em.plan_paths())
    acc = read_accumulator(ctx, em, passes)
    em.close(); ss.close()
    return acc, plan


def addends(inp, flavour, regime):
    key = (regime, regimes.flavours()[flavour][0]["name"])
    if key not in _M:
        m = cu.addend_bound(inp)
        m.setflags(write=False)
        _M[key] = m
    return _M[key]


def largest(inp, ref, flavour, regime):
    key = (regime, regimes.flavours()[flavour][0]["name"])
    if key not in _TOP:
        top = cu.largest_addend(inp, ref.r64)
        top.setflags(write=False)
        _TOP[key] = top
    return _TOP[key]


def at_40(ctx, inp, flavour, regime, tag=None, passes=1):
    """The pair's handle at 2^-40 (bound = the set's own size), computed once."""
    key = (flavour, regime, tag, passes)
    if key not in _ACC40:
        acc, plan = first_pass(ctx, inp, flavour, inp.N, SLICED_TUNINGS[tag] if tag else None, passes)
        for a in acc:
            a.setflags(write=False)
        _ACC40[key] = (acc, plan)
    return _ACC40[key]


def check_integers(acc40, acc_s, m, s, what, flavour, largest, dense_model):
    """The two-sided bound cell by cell, the statistics words, and that the coarse handle still counts: no cell is empty
    that holds an addend of r >= 2^(1-s) in fp64 (twice the unit: r on the device is within 2e-5 of fp64), and under a
    model that spreads r (R1_context, s >= 32) more than half of the cells that count at 40 count at s.  Under R2_sharp
    most cells that count at 40 hold nothing but addends below 2^-32: the fp64 reference itself keeps 35 % (long) and
    39 % (m_k7) of them at 32 (tests/test_coarse_unit_cpu.py), so "more than half" is no property of that regime."""
    cells, d = m.size, 40 - s
    assert len(acc40) == len(acc_s) == cells + 3
    assert np.array_equal(acc_s[cells:], acc40[cells:]), (what, acc_s[cells:], acc40[cells:])
    assert acc40[cells + 2] > 0 and acc40[cells + 1] > 0
    short = (acc40[:cells] >> d) - acc_s[:cells]
    mm = m.ravel()
    assert (acc_s[:cells] >= 0).all() and (short >= 0).all(), (what, int(short.min()), int((short < 0).sum()))
    over = short > mm
    assert not over.any(), (what, int(over.sum()), int(short[over].max()), int(mm[over].min()))
    nz = acc40[:cells] != 0
    assert nz.any()
    must = largest.ravel() >= 2.0 ** (1 - s)
    assert must.any() and acc_s[:cells][must].all(), (what, int(must.sum()), int((acc_s[:cells][must] == 0).sum()))
    if s >= 32 and dense_model:
        assert np.count_nonzero(acc_s[:cells][nz]) > nz.sum() // 2, what
    # the same bound once more, as a row of the margin table: |worst - 0| <= 1 * |0| + 1
    margins.check(what, flavour, "short / m", float(np.max(short[mm > 0] / mm[mm > 0])), 0.0, 1.0, 1.0, against="acc_40 >> d")


@pytest.mark.parametrize("flavour,regime,s", INT_CASES, ids=[f"{f}-{r}-s{s}" for f, r, s in INT_CASES])
def test_integers_at_a_coarse_unit(flavour, regime, s, gpu_ctx, orc):
    """(i) 0 <= (acc_40 >> d) - acc_s <= m cell by cell, equal statistics words, equal plans.  A second pass over the
    same model gives the same words (on the sliced path it may be the one that takes lists: the device chooses from the
    first pass's count of non-zero windows, itself a test that reads the scale)."""
    inp, ref = regimes.case(orc, regime, flavour)
    m = addends(inp, flavour, regime)
    (acc40, again40), plan40 = at_40(gpu_ctx, inp, flavour, regime, passes=2)
    (acc_s, again_s), plan_s = first_pass(gpu_ctx, inp, flavour, cu.BOUNDS[s], passes=2)
    assert plan_s == plan40, (plan_s, plan40)
    assert np.array_equal(again40, acc40) and np.array_equal(again_s, acc_s)
    check_integers(acc40, acc_s, m, s, f"{regime} {inp.case.name} s={s}", flavour, largest(inp, ref, flavour, regime), regime == "R1_context")


@pytest.mark.parametrize("regime", ["R1_context", "R2_sharp"])
@pytest.mark.parametrize("s", [39, 33, 32, 31, 24])
def test_sliced_variants_at_a_coarse_unit(s, regime, gpu_ctx, orc):
    """(ii) The list threshold (k_em_seq), k_m_list and k_m_slice each read the scale on their own.  Two passes on the same
    model per variant -- with list_threshold_pct = 100 the first is dense and the second takes lists, chosen on the device
    from the first one's count of non-zero windows: the same integers in both passes, the bound of (i) in each variant, and
    the same integers in every variant that holds the whole odds table (the E chain cut into column ranges, e_fused = 0,
    multiplies in another grouping and is held to the bound against its own handle at 40, and to the others' statistics
    only as far as test_sliced_paths_agree_bit_for_bit holds it: not bit for bit)."""
    inp, ref = regimes.case(orc, regime, "sliced")
    m = addends(inp, "sliced", regime)
    top = largest(inp, ref, "sliced", regime)
    got = {}
    for tag, tune in SLICED_TUNINGS.items():
        acc40, plan40 = at_40(gpu_ctx, inp, "sliced", regime, tag, passes=2)
        acc_s, plan_s = first_pass(gpu_ctx, inp, "sliced", cu.BOUNDS[s], tune, passes=2)
        assert plan_s == plan40, (tag, plan_s, plan40)
        assert plan_s[2][1] == (tag != "e_sliced"), (tag, plan_s)
        assert np.array_equal(acc_s[0], acc_s[1]) and np.array_equal(acc40[0], acc40[1]), tag
        check_integers(acc40[0], acc_s[0], m, s, f"{regime} {inp.case.name} s={s}", f"sliced/{tag}", top, regime == "R1_context")
        got[tag] = acc_s[0]
    for tag in ("lists_from_pass_2", "dense"):
        assert np.array_equal(got["list"], got[tag]), tag


STEP_CASES = [(f, s) for f in FLAVOURS for s in (39, 32, 24)]


@pytest.mark.parametrize("flavour,s", STEP_CASES, ids=[f"{f}-s{s}" for f, s in STEP_CASES])
def test_one_step_against_fp64_at_a_coarse_unit(flavour, s, gpu_ctx, orc):
    """(iii) iterate(1): the counts within the fuzz bar widened by m * 2^-s on the low side; the model within the fuzz bar
    at s = 39, and at 32 and 24 within it against the fp64 update of the device's OWN counts (the truncation is the
    kernels', the unit the update reads them in is what is checked here)."""
    regime = "R1_context"
    inp, ref = regimes.case(orc, regime, flavour)
    m = cu.all_orders(inp, addends(inp, flavour, regime))
    em, ss = open_em(gpu_ctx, inp, flavour, n_seqs_bound=cu.BOUNDS[s])
    em.iterate(1)
    v, counts = em.getV(), em.getCounts()
    name = f"{regime} {inp.case.name} s={s}"
    margins.check(name, flavour, "counts", cu.fold_low_side(counts, ref.n64, m, s), ref.n64, regimes.N_RTOL, regimes.N_ATOL,
                  against="fp64 - m 2^-s")
    if s == 39:
        margins.check(name, flavour, "v", v, ref.v64, *regimes.v_bar(regime, inp.case.name), against="fp64")
    margins.check(name, flavour, "v", v, cu.update_v_f64(inp, counts), regimes.V_RTOL, regimes.V_ATOL,
                  against="fp64 update, own n")
    margins.check(name, flavour, "llh trace", em.trace()[0][-1], ref.llh64, regimes.LLH_RTOL, regimes.llh_atol(inp.N), against="fp64")
    em.close(); ss.close()


ENTRY_CASES = [(f, s) for f in MORE_UNITS for s in (39, 24)]


@pytest.mark.parametrize("flavour,s", ENTRY_CASES, ids=[f"{f}-s{s}" for f, s in ENTRY_CASES])
def test_both_update_entries_read_the_same_unit(flavour, s, gpu_ctx, orc):
    """(iv) Two passes stepwise (every update a launch of its own) and as iterate(2) (the first update in the second
    pass's block prologue where the handle allows it): the same bits, as test_both_update_entries_read_the_same_alpha."""
    inp, _ = regimes.case(orc, "R1_context", flavour)
    em, ss = open_em(gpu_ctx, inp, flavour, n_seqs_bound=cu.BOUNDS[s])
    for _ in range(2):
        em.EStep(); em.MStep()
    twin, _ = open_em(gpu_ctx, inp, flavour, ss=ss, n_seqs_bound=cu.BOUNDS[s])
    twin.iterate(2)
    assert em.getCounts().any()
    assert np.array_equal(em.getV().view(np.uint32), twin.getV().view(np.uint32))
    assert np.array_equal(em.getCounts().view(np.uint32), twin.getCounts().view(np.uint32))
    assert np.array_equal(em.getS().view(np.uint32), twin.getS().view(np.uint32))
    em.close(); twin.close(); ss.close()


def test_update_over_blocks_reads_the_same_unit(gpu_ctx):
    """(iv) k_update_counts + k_update_model against the one-block update at 2^-24, on the smallest table of
    tests/test_update_blocks_gpu.py that is beyond the update's LDS form, cut to 600 sequences."""
    N, L0, W, K = 600, 200, 20, 3
    pwm = synth.make_pwm(W, 9)
    codes, in_off = synth.make_sequences(N, L0, pwm, 9, 0.5, 0.0, 0)
    packed = bm.PackedSeqs.from_codes(codes, in_off, False, seed=42)
    A = synth.alpha_matrix(synth.default_alpha(K), W)
    vbg = packed.bg_model(2, np.array([1.0, 10.0, 10.0], np.float32))
    v0 = synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K)
    res = []
    for blocks in (1, 0):
        gpu_ctx.set_tuning(update_blocks=blocks)
        try:
            seqs = bm.SeqSet(gpu_ctx, packed)
            em = bm.EM(gpu_ctx, seqs, K, W, vbg, A, v0, 0.3, optimizeQ=True, n_seqs_bound=cu.BOUNDS[24])
        finally:
            gpu_ctx.set_tuning(update_blocks=1)
        em.iterate(3)
        em.EStep(); em.MStep(); em.optimize_q()
        res.append((em.getV(), em.getCounts(), em.getS(), np.float32(em.getQ()), np.float32(em.getLLH())))
        em.close(); seqs.close()
    assert res[0][1].any()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    # ... and the unit is the one asked for: the same counts as at 2^-40, up to the truncation
    seqs = bm.SeqSet(gpu_ctx, packed)
    fine = bm.EM(gpu_ctx, seqs, K, W, vbg, A, v0, 0.3, optimizeQ=True, n_seqs_bound=N)
    fine.iterate(1)
    coarse = bm.EM(gpu_ctx, seqs, K, W, vbg, A, v0, 0.3, optimizeQ=True, n_seqs_bound=cu.BOUNDS[24])
    coarse.iterate(1)
    top = slice(regimes.v_offset(K, W), None)
    lost = fine.getCounts().astype(np.float64)[top] - coarse.getCounts().astype(np.float64)[top]
    # at most one unit per window and cell (both strands and the junction: fewer than 2 L0 + 2 windows per sequence), and
    # never a gain beyond the float rounding of the two read-outs
    assert (lost >= -3e-7 * fine.getCounts()[top]).all() and 0 < lost.max() <= N * (2 * L0 + 2) * 2.0 ** -24
    fine.close(); coarse.close(); seqs.close()


MASK_SPECS = [SMALL_CASES[0], dict(name="m_k7", N=60, L0=260, W=6, K=7, ragged=60, n_frac=0.002)]


@pytest.mark.parametrize("s", [39, 32])
@pytest.mark.parametrize("spec", MASK_SPECS, ids=[d["name"] for d in MASK_SPECS])
def test_mask_at_a_coarse_unit(spec, s, gpu_ctx, orc):
    """(v) EM::mask: cut-off, listed count and q equal the oracle's as at 2^-40; counts and model within the flat bar of
    tests/test_mask_gpu.py plus one unit per listed window."""
    from tests.test_mask_gpu import CASES
    assert spec in CASES
    c = Case(**spec)
    em, ss, kmer, off, vbg = make_em(gpu_ctx, c, orc, epsilon=0.0, max_iterations=2, n_seqs_bound=cu.BOUNDS[s])
    it = em.mask(0.1)
    res = orc.mask(kmer, off, c.K, c.W, c.bg_order, vbg, c.A, c.v0, c.q, f=0.1, epsilon=0.0, max_iter=2)
    assert it == res["iterations"] == 2
    assert np.float32(em.last_mask["cutoff"]) == np.float32(res["cutoff"])
    assert em.last_mask["listed"] == res["listed"]
    assert np.float32(em.getQ()) == np.float32(res["q"])
    name, fl = f"mask {c.name} f=0.1 s={s}", "mask kernels"
    room = res["listed"] * 2.0 ** -s
    assert em.getCounts().any()
    margins.check(name, fl, "n pass 2", em.getCounts(), res["n"], 1e-5, 1e-7 + room, against="fp32 restatement")
    margins.check(name, fl, "v pass 2", em.getV(), res["v"], 1e-5, 1e-9 + room, against="fp32 restatement")
    em.close(); ss.close()


@pytest.mark.parametrize("layout", [3, 8])
def test_shards_add_up_at_a_coarse_unit(layout, gpu_ctx):
    """(vi) At 2^-32 the shards' accumulators add up to the whole set's word for word: uniform and mixed rows."""
    from tests.test_partition_exact_gpu import accumulator
    hip = C.CDLL("libamdhip64.so")
    shape = dict(N=600, L0=200, W=20, K=2, tune=dict(group_layout=layout))
    N, W, K = shape["N"], shape["W"], shape["K"]
    pwm = synth.make_pwm(W, 3)
    codes, off = synth.make_sequences(N, shape["L0"], pwm, 3, 0.5)
    pk = bm.PackedSeqs.from_codes(codes, off, False, seed=42)
    vbg = pk.bg_model(2, np.array([1.0, 10.0, 10.0], np.float32))
    A = synth.alpha_matrix(synth.default_alpha(K), W)
    v0 = synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K)
    bound = cu.BOUNDS[32]
    whole = accumulator(gpu_ctx, hip, pk, 0, N, shape, vbg, A, v0, bound=bound)
    fine = accumulator(gpu_ctx, hip, pk, 0, N, shape, vbg, A, v0)
    cells = 4 ** (K + 1) * W
    assert whole[cells + 2] == N and np.array_equal(whole[cells:], fine[cells:])
    # the unit is 2^-32: column 0 holds every window once, so its cells sum to the sum of r (a statistic, in 2^-30)
    col0 = float(whole[:cells].reshape(-1, W)[:, 0].sum())
    assert abs(np.log2(col0 / (float(whole[cells + 1]) / 2.0 ** 30)) - 32) < 0.01
    for cuts in ((0, N // 2, N), (0, 1, N // 7, N)):
        total = np.zeros_like(whole)
        for b, e in zip(cuts[:-1], cuts[1:]):
            total += accumulator(gpu_ctx, hip, pk, b, e, shape, vbg, A, v0, bound=bound)
        assert np.array_equal(total, whole), cuts


def test_two_ranks_at_a_common_coarse_unit_equal_one_rank(gpu_ctx, orc):
    """(vi) Two ranks in one process over the host-staged communicator, both at n_seqs_bound = 2^30: verify_comm accepts
    the common unit and the model equals the one-rank run at that bound bit for bit."""
    from tests.test_comm_gpu import _two_local_ranks
    c = Case(**SMALL_CASES[6])
    bound = cu.BOUNDS[32]
    one, ss, *_ = make_em(gpu_ctx, c, orc, optimizeQ=True, max_iterations=60, n_seqs_bound=bound)
    one.iterate(3)
    want = (one.getV(), one.getQ(), one.trace()[0], one.getCounts())
    one.close(); ss.close()

    def calls(em, r):
        em.iterate(3)
        return em.getV(), em.getQ(), em.trace()[0], em.getCounts()

    out, errs = _two_local_ranks(c, orc, (bound, bound), calls)
    assert errs == [None, None], errs
    assert want[3].any()
    for r in range(2):
        assert out[r][1] == want[1]
        for k in (0, 2, 3):
            assert np.array_equal(out[r][k], want[k]), (r, k)


STAIRCASE = [(1 << 22, 0, 40), ((1 << 22) + 1, 0, 39), (1 << 23, 0, 39), ((1 << 23) + 1, 0, 38), (1 << 30, 0, 32), (1 << 38, 0, 24),
             ((1 << 38) + 1, 0, 24), (1 << 62, 0, 24), (0, 1 << 30, 32), (0, 0, 40)]


@pytest.mark.parametrize("bound,n_global,want", STAIRCASE, ids=[f"bound{b:#x}-global{g:#x}" for b, g, _ in STAIRCASE])
def test_the_unit_follows_the_bound(bound, n_global, want, gpu_ctx, orc):
    """(vii) fix_shift inferred from a tiny handle's accumulator: column 0 holds every window once, so its cells sum to
    the sum of r in units of 2^-fix_shift, and the statistics carry the sum of r in units of 2^-30."""
    c = Case("tiny", N=8, L0=40, W=6, K=1)
    assert cu.fix_shift_of(bound or n_global or c.N) == want
    assert bound > (1 << 38) or bound * (1 << want) <= 1 << 62
    em, ss, *_ = make_em(gpu_ctx, c, orc, n_seqs_bound=bound, n_seqs_global=n_global)
    (acc,) = read_accumulator(gpu_ctx, em)
    em.close(); ss.close()
    cells = 4 ** (c.K + 1) * c.W
    col0 = float(acc[:cells].reshape(-1, c.W)[:, 0].sum())
    sum_r = float(acc[cells + 1]) / 2.0 ** 30
    assert acc[cells + 2] == c.N and sum_r > 0.5
    assert abs(np.log2(col0 / sum_r) - want) < 0.01, (col0, sum_r)
    assert int(np.rint(np.log2(col0 / sum_r))) == want
