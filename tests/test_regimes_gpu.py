"""The EM pass across numerical regimes (tests/regimes.py), crossed with the kernel flavours, at small shapes.

Everything else in the suite feeds the kernels one point in the space of numbers (tests/cases.py::Case); the places
where the kernels deliberately differ from the reference's arithmetic -- group products rounded first, 1/Z as v_rcp_f32
plus a Newton step, log Z as v_log_f32 * ln 2, the 0 * x = 0 product, the 2^-40 truncation with its scale riding on
1/Z, the non-finite flag of the statistics word -- only show away from it.

References: r against the numpy fp64 E step, llh / v / counts against the oracle's em_step_f64, both pinned by
tests/test_regimes_cpu.py; the bars are the fuzz sweep's own (tests/fuzz_parity.py), through margins.check so that the
observed margins land in the session's parity-margin table (profiles/regimes_parity_margins.txt).

Two deliberate mistakes were tried against the whole `-m gpu` suite.  The update reading A[k][0] for every column: only
the R6 cases of test_one_step_in_every_regime fail (all 18), nothing older.  A group product of the K = 2, G = 3 rows taking
its middle column's odds from the neighbouring context: the R1 / R2 / R3 / R8 cases on grouped_6mer and on layout0 / layout3
fail -- and so do some eighty older tests, because the odds are v / vbg and the LEARNED background depends on the context
even where v does not.  Context mix-ups were never invisible to the suite; a constant-alpha assumption was.
"""
import numpy as np
import pytest

import bammmotif2_amd as bm
from tests import margins, regimes

pytestmark = pytest.mark.gpu

TUNING_DEFAULTS = dict(group_layout=-1, grouped=1)
EXACT_ZERO_PATTERN = ("R3_zeros", "R4_odds_one", "R5_q_0")


def open_em(ctx, inp, flavour, ss=None, q=None, **kw):
    """(em, ss) of the flavour, with the planner's report checked: a case cannot silently run another kernel."""
    _, tuning, kind = regimes.flavours()[flavour]
    if ss is None:
        ss = bm.SeqSet(ctx, bm.PackedSeqs.from_kmers(inp.kmer, inp.off))
    ctx.set_tuning(**tuning)
    try:
        em = bm.EM(ctx, ss, inp.K, inp.W, inp.vbg, inp.A, inp.v, inp.q if q is None else q, bg_order=inp.bg_order, **kw)
    finally:
        ctx.set_tuning(**{k: TUNING_DEFAULTS[k] for k in tuning})
    grouped, other, _ = em.plan()
    sliced, _, long_seqs = em.plan_paths()
    mixed = em.plan_mixed()
    what = f"{flavour}: plan {(grouped, other)}, mixed {mixed}, sliced {sliced}, long {long_seqs}"
    if kind == "per_column":
        assert grouped == 0 and other == inp.N and not sliced and long_seqs == 0, what
    elif kind == "order_7":                                   # beyond the grouped kernels (K <= 3)
        assert grouped == 0 and other == inp.N, what
    elif kind == "grouped":
        assert grouped > 0 and mixed == 0 and not sliced and long_seqs == 0, what
    elif kind == "mixed":
        assert grouped > 0 and mixed == grouped and long_seqs == 0, what
    elif kind == "sliced":
        assert sliced and long_seqs == 0, what
    elif kind == "long":
        assert long_seqs >= 1, what
    else:
        raise KeyError(kind)
    return em, ss


def check_scorer(ctx, ss, inp, orc):
    """bm.logodds on the regime's model against the oracle, bit for bit (as test_logodds_bit_exact)."""
    Kb = min(inp.bg_order, inp.K)
    mops_o, zoops_o, z_o = orc.logodds(inp.kmer, inp.off, inp.K, inp.W, orc.log_s(inp.v, inp.vbg, inp.K, inp.W, Kb))
    mops, zoops, z = bm.logodds(ctx, ss, inp.K, inp.W, inp.bg_order, inp.v, inp.vbg)
    assert np.array_equal(mops, mops_o) and np.array_equal(zoops, zoops_o) and np.array_equal(z, z_o)


PAIRS = regimes.pairs()


@pytest.mark.parametrize("regime,flavour", PAIRS, ids=[f"{r}-{f}" for r, f in PAIRS])
def test_one_step_in_every_regime(regime, flavour, gpu_ctx, orc):
    inp, ref = regimes.case(orc, regime, flavour)
    em, ss = open_em(gpu_ctx, inp, flavour)
    name = f"{regime} {inp.case.name}"
    off = inp.off.astype(np.int64)

    em.EStep()
    r = em.getR()
    margins.check(name, flavour, "r", r, ref.r64, regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL, against="fp64")
    if regime in EXACT_ZERO_PATTERN:
        assert np.array_equal(r == 0, ref.r64 == 0)
    else:
        assert not r[ref.r32 == 0].any()
    llh_atol = regimes.llh_atol(inp.N)
    margins.check(name, flavour, "llh EStep", em.getLLH(), ref.llh64, regimes.LLH_RTOL, llh_atol, against="fp64")

    em.iterate(1)
    v, counts = em.getV(), em.getCounts()
    margins.check(name, flavour, "v", v, ref.v64, *regimes.v_bar(regime, inp.case.name), against="fp64")
    margins.check(name, flavour, "counts", counts, ref.n64, regimes.N_RTOL, regimes.N_ATOL, against="fp64")
    margins.check(name, flavour, "llh trace", em.trace()[0][-1], ref.llh64, regimes.LLH_RTOL, llh_atol, against="fp64")

    if regime == "R3_zeros":
        for n in inp.zero_seqs:
            assert not r[off[n]:off[n + 1]].any()
    if regime == "R4_odds_one":
        r_cf, llh_cf, nK_cf = regimes.odds_one_closed_form(inp)
        margins.check(name, flavour, "r", r, r_cf, regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL, against="closed form")
        margins.check(name, flavour, "counts", counts[regimes.v_offset(inp.K, inp.W):], nK_cf.ravel(), regimes.N_RTOL, regimes.N_ATOL,
                      against="closed form")
        margins.check(name, flavour, "llh trace", em.trace()[0][-1], llh_cf, regimes.LLH_RTOL, llh_atol, against="closed form")
    if regime == "R5_q_0":
        assert not r.any() and not counts.any() and em.getLLH() == 0.0 and em.trace()[0][-1] == 0.0
    check_scorer(gpu_ctx, ss, inp, orc)
    em.close(); ss.close()


UPDATE_PAIRS = [(r, f) for r in regimes.UPDATE_REGIMES for f in regimes.BASE_FLAVOURS]


@pytest.mark.parametrize("regime,flavour", UPDATE_PAIRS, ids=[f"{r}-{f}" for r, f in UPDATE_PAIRS])
def test_both_update_entries_read_the_same_alpha(regime, flavour, gpu_ctx, orc):
    """Two passes stepwise (every update a launch of its own) and as iterate(2) (where the handle allows it, the first
    update runs in the second pass's block prologue): the same integers through the same device function, so the same
    bits -- as tests/test_fused_update_gpu.py asserts for an alpha that is constant over the columns."""
    inp, _ = regimes.case(orc, regime, flavour)
    em, ss = open_em(gpu_ctx, inp, flavour)
    for _ in range(2):
        em.EStep(); em.MStep()
    twin, _ = open_em(gpu_ctx, inp, flavour, ss=ss)
    twin.iterate(2)
    assert np.array_equal(em.getV().view(np.uint32), twin.getV().view(np.uint32))
    assert np.array_equal(em.getCounts().view(np.uint32), twin.getCounts().view(np.uint32))
    assert np.array_equal(em.getS().view(np.uint32), twin.getS().view(np.uint32))
    em.close(); twin.close(); ss.close()


@pytest.mark.parametrize("flavour", ["grouped_6mer", "per_column"])
def test_non_finite_statistics_are_flagged_and_poison_nothing(flavour, gpu_ctx, orc):
    """q = 1 with sequences whose every window meets a zero of the model: Z = 0 for them, log Z = -inf, r = 0 / 0.  The
    statistics word carries the flag (csrc/device_utils.h: kStatBadUnit) and the update turns it into a NaN llh, as the
    reference's float sum would hold; every other sequence is computed as usual, and a handle created afterwards on the
    same context and set is not affected.

    Read before this test was written: nothing the sequence kernels derive from r, Z or the odds is an address or an
    unbounded loop count.  Table rows and count cells come from the sequence record (k-mers, lengths, N exceptions).  What
    does depend on r is WHICH lanes add (ballots of `addend != 0`) and how many entries a sequence's compacted list gets
    (kernels.hip: `at = nnz + mbcnt`, `ecnt = (nnz + 63) >> 6`; grouped_kernel.h / mixed_kernel.h: `nlog + rank`): counts
    of set ballot bits, at most one per window (or per fix lane) of the sequence, the size the lists are laid out for
    whatever r is.  A NaN r converts to the addend 0 (to_fixed40) and fails `>= 2^-40`, so such lanes sit out."""
    inp, _ = regimes.case(orc, "R3_zeros", flavour)
    off = inp.off.astype(np.int64)
    before, ss = open_em(gpu_ctx, inp, flavour)
    before.iterate(1)
    want = (before.getV(), before.getCounts(), before.getR(), before.getLLH())
    before.close()

    bad, _ = open_em(gpu_ctx, inp, flavour, ss=ss, q=1.0)
    bad.EStep()
    assert not np.isfinite(bad.getLLH())
    r = bad.getR()
    bad.iterate(1)
    assert not np.isfinite(bad.trace()[0][-1]) and not np.isfinite(bad.getLLH())
    degenerate = regimes.Inputs(inp.case, inp.kmer, inp.off, inp.v, 1.0, inp.A, inp.vbg, inp.zero_seqs)
    with np.errstate(invalid="ignore", divide="ignore"):
        r64, Z, *_ = regimes.estep_f64(degenerate)
    assert set(np.flatnonzero(Z == 0)) >= set(inp.zero_seqs)
    ok = np.concatenate([np.arange(off[n], off[n + 1]) for n in range(inp.N) if Z[n] > 0])
    margins.check(f"R3_zeros q=1 {inp.case.name}", flavour, "r, finite seqs", r[ok], r64[ok],
                  regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL, against="fp64")
    bad.close()

    after, _ = open_em(gpu_ctx, inp, flavour, ss=ss)
    after.iterate(1)
    got = (after.getV(), after.getCounts(), after.getR(), after.getLLH())
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert got[3] == want[3] and np.isfinite(got[3])
    after.close(); ss.close()
