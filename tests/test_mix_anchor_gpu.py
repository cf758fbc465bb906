"""The start-anchored flavour of k_em_mix (csrc/mixed_kernel.h, template flag ANCH; csrc/plan.cpp: plan_class_split).

A sequence of a mixed-row launch runs in the shortest length class whose 64 M slots reach every table row that is not
neutral when the windows sit at their first group end: 64 M >= (L - W + 1) + 2 + 3 (4 - B), B the motif's narrow groups
(W = 3 B + 4 A).  For W = 20 (B = 4) that is 64 M >= L - W + 3: 200 bp on both strands (L = 401) runs at 6 positions per
lane instead of 7.  `mix_anchor` = 0 (bamm_ctx_set_tuning) keeps every sequence in the class of its length.

What is checked, all with mixed rows forced (group_layout = 8) on 96..160 sequences, both strands:
  * the rule at its boundaries and the plan read-out (Context.set_tuning / EM.plan_launches);
  * r, counts and model of three passes against the fp64 restatement (tests/regimes.py: estep_f64, the oracle's
    em_step_f64), at the bars tests/test_regimes_gpu.py holds k_em_mix to (regimes.R_RTOL ... V_ATOL);
  * r against the end-anchored flavour of the same build: the window products have the same bits, only Z is summed
    over another assignment of windows to lanes;
  * what must stay exact: counts = the integer sum of the truncated kernel's own r, shards add up word for word,
    iterate(n) = optimize() with epsilon = 0 bit for bit.

A class-12 bucket (641..768 positions) is no mixed-row launch (mix_geometry: up to 10 positions per lane), so the class of
10 positions per lane is never the target of the rule; the case `w20_no_mixed_rows` pins that.
"""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth
from tests import coarse_unit as cu
from tests import regimes
from tests.cases import Case

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)

# (name, L0, W, positions per lane the launch runs at, start-anchored).  L = 2 L0 + 1; span = L - W + 3 + 3 (4 - B).
BOUNDARY = [
    ("w20_L399", 199, 20, 6, True),          # span 382
    ("w20_L401", 200, 20, 6, True),          # span 384 = 64 * 6 exactly: the bench shape
    ("w20_L403", 201, 20, 7, False),         # span 386: one position past it, stays in the class of its length
    ("w20_to_m4", 136, 20, 4, True),         # L 273 (class 5), span 256
    ("w20_to_m5", 168, 20, 5, True),         # L 337 (class 6), span 320
    ("w20_to_m8", 264, 20, 8, True),         # L 529 (class 10, 768 threads), span 512: 1024 threads in the class run
    ("w13_b3_a1", 195, 13, 6, True),         # B = 3: span L - 7 = 384
    ("w13_past", 196, 13, 7, False),         # ... 386
    ("w14_b2_a2", 194, 14, 6, True),         # B = 2: span L - 5 = 384
    ("w16_b4_a1", 198, 16, 6, True),         # B = 4: span L - 13 = 384
    ("w17_b3_a2", 197, 17, 6, True),         # B = 3: span L - 11 = 384
]
IDS = [b[0] for b in BOUNDARY]
ANCHORED = [b for b in BOUNDARY if b[4]]


def open_mixed(ctx, c, orc, anchor=1, layout=8, ss=None, **kw):
    """(em, ss, kmer, off, vbg) with mixed rows forced and the flavour chosen; the tuning is back at its defaults after."""
    seq, kmer, off, vbg = c.encode(orc)
    if ss is None:
        ss = bm.SeqSet(ctx, bm.PackedSeqs.from_kmers(kmer, off))
    ctx.set_tuning(group_layout=layout, mix_anchor=anchor)
    try:
        em = bm.EM(ctx, ss, c.K, c.W, vbg, c.A, c.v0, c.q, bg_order=c.bg_order, **kw)
    finally:
        ctx.set_tuning(group_layout=-1, mix_anchor=1)
    return em, ss, kmer, off, vbg


def case_of(name, L0, W, N=96, **kw):
    return Case(name=name, N=N, L0=L0, W=W, K=2, **kw)


@pytest.mark.parametrize("name,L0,W,m_run,anchored", BOUNDARY, ids=IDS)
def test_rule_and_three_passes_against_fp64(name, L0, W, m_run, anchored, gpu_ctx, orc):
    c = case_of(name, L0, W)
    em, ss, kmer, off, vbg = open_mixed(gpu_ctx, c, orc)
    assert em.plan() == (c.N, 0, 1) and em.plan_mixed() == c.N
    assert em.plan_launches() == [dict(count=c.N, positions_per_lane=m_run, mixed=True, anchored=anchored)]
    # the same set with the flavour off: the class of the length
    off_em, _, *_ = open_mixed(gpu_ctx, c, orc, anchor=0, ss=ss)
    (plain,) = off_em.plan_launches()
    assert plain["mixed"] and not plain["anchored"] and plain["positions_per_lane"] == -(-(2 * L0 + 1) // 64) + (2 * L0 + 1 > 512)
    off_em.close()
    for _ in range(3):
        v = em.getV()
        inp = regimes.Inputs(c, kmer, off, v, c.q, c.A, vbg)
        r64, _, llh64, _, _ = regimes.estep_f64(inp)
        v64, n64, *_ = orc.em_step_f64(kmer, off, c.K, c.W, c.bg_order, vbg, c.A, v, c.q)
        em.EStep()
        r = em.getR()
        np.testing.assert_allclose(r, r64, rtol=regimes.R_RTOL * regimes.r_len_factor(off), atol=regimes.R_ATOL)
        np.testing.assert_allclose(em.getLLH(), llh64, rtol=regimes.LLH_RTOL, atol=regimes.llh_atol(c.N))
        em.MStep()
        np.testing.assert_allclose(em.getCounts(), n64, rtol=regimes.N_RTOL, atol=regimes.N_ATOL)
        np.testing.assert_allclose(em.getV(), v64, rtol=regimes.V_RTOL, atol=regimes.V_ATOL)
    em.close(); ss.close()


def test_a_class_12_bucket_is_no_mixed_row_launch(gpu_ctx, orc):
    c = case_of("w20_no_mixed_rows", 328, 20, N=48)          # L 657, span 640 = 64 * 10, but the bucket's class is 12
    em, ss, *_ = open_mixed(gpu_ctx, c, orc)
    assert em.plan_mixed() == 0 and not any(l["anchored"] for l in em.plan_launches())
    em.close(); ss.close()


def rel_diff(a, b):
    """Largest |a - b| / |b| over the windows either flavour gives a normal number; both must be zero together."""
    assert np.array_equal(a == 0, b == 0)
    ok = np.abs(b) > 1e-30
    return float(np.max(np.abs(a[ok].astype(np.float64) - b[ok]) / np.abs(b[ok].astype(np.float64))))


@pytest.mark.parametrize("name,L0,W,m_run,anchored", ANCHORED, ids=[b[0] for b in ANCHORED])
def test_r_against_the_end_anchored_flavour(name, L0, W, m_run, anchored, gpu_ctx, orc):
    """The two flavours multiply the same factors in the same order, so they differ through Z alone: a sum of the same
    n = L - W + 1 non-negative fp32 terms plus 1 - q, over M_a or M_e terms per lane, six levels across the wave and the
    final add.  A sum of non-negative terms along k additions is within k u of exact (u = eps / 2), so the two Z agree
    within (M_a + M_e + 14) u; 1 / Z (reciprocal and one Newton step) and the product r = U / Z add at most 1.5 eps on
    either side.  Bound: ((M_a + M_e + 14) / 2 + 3) eps -- 16.5 eps for 6 and 7 positions per lane.  And the pair must not
    differ more than the two flavours the project already has, mixed and uniform rows (which also group the products
    differently), do on the same input."""
    c = case_of(name, L0, W)
    r = {}
    ss = None
    for tag, layout, anchor in (("anchored", 8, 1), ("end", 8, 0), ("uniform", 3, 1)):
        em, ss, *_ = open_mixed(gpu_ctx, c, orc, anchor=anchor, layout=layout, ss=ss)
        (launch,) = em.plan_launches()
        assert (launch["mixed"], launch["anchored"]) == (layout == 8, tag == "anchored"), (tag, launch)
        if tag == "end":
            m_end = launch["positions_per_lane"]
        em.EStep()
        r[tag] = em.getR()
        em.close()
    ss.close()
    bound = ((m_run + m_end + 14) / 2 + 3) * EPS
    new_pair, old_pair = rel_diff(r["anchored"], r["end"]), rel_diff(r["end"], r["uniform"])
    print(f"{name}: anchored vs end-anchored {new_pair / EPS:.2f} eps (bound {bound / EPS:.1f}), mixed vs uniform rows {old_pair / EPS:.2f} eps")
    assert new_pair <= bound
    assert new_pair <= old_pair


def accumulator_words(ctx, em):
    hip = C.CDLL("libamdhip64.so")
    em.accumulate()
    ctx.sync()
    p, n = em.reduce_buffer()
    h = np.zeros(n, np.int64)
    assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(p), n * 8, 2) == 0
    return h


@pytest.mark.parametrize("shift", [40, 32])
@pytest.mark.parametrize("name,L0,W", [("w20_L401", 200, 20), ("w13_b3_a1", 195, 13)])
def test_counts_are_the_integer_sum_of_the_kernels_own_r(name, L0, W, shift, gpu_ctx, orc):
    """cell [y][j] = sum over the windows i with i + j < L - W + 1 (EM.cpp:167, 236-242) of floor(r 2^shift), r as getR()
    of the same flavour returns it: equality, at the finest unit and at 2^-32."""
    c = case_of(name, L0, W)
    em, ss, kmer, off, vbg = open_mixed(gpu_ctx, c, orc, n_seqs_bound=c.N if shift == 40 else cu.BOUNDS[shift])
    assert em.plan_launches()[0]["anchored"]
    em.EStep()
    r = em.getR().astype(np.float64)
    acc = accumulator_words(gpu_ctx, em)
    em.close(); ss.close()
    Y, o = 64, np.asarray(off).astype(np.int64)
    want = np.zeros((Y, W), np.int64)
    for n in range(c.N):
        L = int(o[n + 1] - o[n])
        LW1 = L - W + 1
        y = (kmer[o[n]:o[n] + LW1] % np.uint64(Y)).astype(np.int64)
        f = np.floor(r[o[n]:o[n] + LW1][::-1] * 2.0 ** shift).astype(np.int64)      # by window start
        for j in range(W):
            np.add.at(want[:, j], y[j:], f[:LW1 - j])
    assert want.any()
    assert np.array_equal(acc[:Y * W], want.ravel())
    assert acc[Y * W + 2] == c.N


def mixed_length_set(N=160):
    """Two lengths in one bucket of 7 positions per lane: L = 401 runs start-anchored at 6, L = 421 stays at 7."""
    W, K = 20, 2
    pwm = synth.make_pwm(W, 3)
    ca, oa = synth.make_sequences(N // 2, 200, pwm, 3, 0.5)
    cb, ob = synth.make_sequences(N // 2, 210, pwm, 4, 0.5)
    # interleaved, so that every shard holds both lengths in another proportion
    codes, off = [], [0]
    for i in range(N // 2):
        for cs, os_ in ((ca, oa), (cb, ob)):
            codes.append(cs[int(os_[i]):int(os_[i + 1])])
            off.append(off[-1] + len(codes[-1]))
    return np.concatenate(codes), np.array(off, np.uint64), W, K, pwm


def test_a_mixed_bucket_splits_and_shards_add_up(gpu_ctx):
    """One bucket, two launches (each with its own lane records); whole, in 2 and in 3 uneven shards with n_seqs_bound
    set: the accumulators -- counts, llh, sum of r, sequence count, all the model update reads -- add up word for word."""
    from tests.test_partition_exact_gpu import accumulator
    hip = C.CDLL("libamdhip64.so")
    codes, off, W, K, pwm = mixed_length_set()
    N = len(off) - 1
    pk = bm.PackedSeqs.from_codes(codes, off, False, seed=42)
    vbg = pk.bg_model(2, np.array([1.0, 10.0, 10.0], np.float32))
    A = synth.alpha_matrix(synth.default_alpha(K), W)
    v0 = synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K)
    shape = dict(N=N, W=W, K=K, tune=dict(group_layout=8))
    gpu_ctx.set_tuning(group_layout=8)
    try:
        ss = bm.SeqSet(gpu_ctx, pk)
        em = bm.EM(gpu_ctx, ss, K, W, vbg, A, v0, 0.3, n_seqs_bound=N)
    finally:
        gpu_ctx.set_tuning(group_layout=-1)
    assert sorted(em.plan_launches(), key=lambda l: l["positions_per_lane"]) == [
        dict(count=N // 2, positions_per_lane=6, mixed=True, anchored=True),
        dict(count=N // 2, positions_per_lane=7, mixed=True, anchored=False)]
    em.close(); ss.close()
    whole = accumulator(gpu_ctx, hip, pk, 0, N, shape, vbg, A, v0)
    cells = 64 * W
    assert whole[cells + 2] == N and whole[:cells].any()
    for cuts in ((0, N // 2 + 1, N), (0, 7, N // 3, N)):
        total = np.zeros_like(whole)
        for b, e in zip(cuts[:-1], cuts[1:]):
            total += accumulator(gpu_ctx, hip, pk, b, e, shape, vbg, A, v0)
        assert np.array_equal(total, whole), cuts


@pytest.mark.parametrize("which", ["single_length", "mixed_bucket"])
def test_both_parts_of_a_bucket_against_fp64_and_iterate_equals_optimize(which, gpu_ctx, orc):
    """A single-length bucket (one launch) and a mixed one (two): one step against the fp64 restatement, r of every
    sequence of either part, and iterate(6) = optimize() with epsilon = 0 and max_iterations = 6, bit for bit."""
    c = case_of("w20_L401", 200, 20, N=128, ragged=0 if which == "single_length" else 8)   # L 385..417: one bucket, both sides of 401
    em, ss, kmer, off, vbg = open_mixed(gpu_ctx, c, orc, optimizeQ=True, epsilon=0.0, max_iterations=6)
    launches = sorted(em.plan_launches(), key=lambda l: l["positions_per_lane"])
    assert len(launches) == (1 if which == "single_length" else 2) and all(l["mixed"] for l in launches)
    assert sum(l["count"] for l in launches) == c.N and launches[0]["anchored"] and launches[0]["positions_per_lane"] == 6
    if which == "mixed_bucket":
        assert not launches[1]["anchored"] and launches[1]["positions_per_lane"] == 7 and launches[1]["count"] > 0
    inp = regimes.Inputs(c, kmer, off, c.v0, c.q, c.A, vbg)
    r64, *_ = regimes.estep_f64(inp)
    em.EStep()
    np.testing.assert_allclose(em.getR(), r64, rtol=regimes.R_RTOL * regimes.r_len_factor(off), atol=regimes.R_ATOL)
    twin, *_ = open_mixed(gpu_ctx, c, orc, ss=ss, optimizeQ=True, epsilon=0.0, max_iterations=6)
    assert twin.optimize() == 6
    em.iterate(6)
    for a, b in ((em.getV(), twin.getV()), (em.getCounts(), twin.getCounts()), (em.getS(), twin.getS())):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.float32(em.getQ()) == np.float32(twin.getQ())
    em.close(); twin.close(); ss.close()


def with_n(c, where):
    """The case's sequences with an N (code 0) put at `where(length)` of every fourth input sequence."""
    codes, off = c.codes.copy(), c.in_off.astype(np.int64)
    for n in range(0, c.N, 4):
        codes[off[n] + where(int(off[n + 1] - off[n]))] = 0
    c.codes = codes
    return c


@pytest.mark.parametrize("which", ["junction_only", "n_within_w_of_the_edge", "n_inside", "fold_mask"])
def test_junction_edge_and_mask(which, gpu_ctx, orc):
    """The strand junction (every sequence of a double-stranded set carries its N at position L0) alone; an extra N within
    W of the sequence's end, whose virtual rows would meet the edge rows (those sequences leave the grouped launch: both
    launches are checked); an extra N in the middle; sequences the fold mask leaves out.  One step against fp64."""
    c = case_of("w20_L401_" + which, 200, 20, N=120)
    if which == "n_within_w_of_the_edge":
        c = with_n(c, lambda length: 5)                      # strand 2 ends with the complement of the input's start
    elif which == "n_inside":
        c = with_n(c, lambda length: length // 3)
    mask = (np.arange(c.N) % 5 != 2).astype(np.uint8) if which == "fold_mask" else None
    em, ss, kmer, off, vbg = open_mixed(gpu_ctx, c, orc, mask=mask)
    grouped, other, _ = em.plan()
    launches = [l for l in em.plan_launches() if l["mixed"]]
    assert launches and all(l["anchored"] and l["positions_per_lane"] == 6 for l in launches)
    if which == "n_within_w_of_the_edge":
        assert other >= c.N // 4 and grouped + other == c.N
    elif which != "n_inside":
        assert (grouped, other) == (c.N, 0)
    keep = np.arange(c.N) if mask is None else np.flatnonzero(mask)
    o = np.asarray(off).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum(o[keep + 1] - o[keep])]).astype(np.uint64)
    sub_kmer = np.concatenate([kmer[o[n]:o[n + 1]] for n in keep])
    inp = regimes.Inputs(c, kmer, off, c.v0, c.q, c.A, vbg)
    r64, *_ = regimes.estep_f64(inp)
    v64, n64, *_ = orc.em_step_f64(sub_kmer, sub_off, c.K, c.W, c.bg_order, vbg, c.A, c.v0, c.q)
    em.EStep()
    np.testing.assert_allclose(em.getR(), r64, rtol=regimes.R_RTOL * regimes.r_len_factor(off), atol=regimes.R_ATOL)   # masked-out sequences too
    em.MStep()
    np.testing.assert_allclose(em.getCounts(), n64, rtol=regimes.N_RTOL, atol=regimes.N_ATOL)
    np.testing.assert_allclose(em.getV(), v64, rtol=regimes.V_RTOL, atol=regimes.V_ATOL)
    em.close(); ss.close()
