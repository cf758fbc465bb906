"""The model update alone, bit for bit against tests/update_script.py::expected_update, in all of its forms.

The update turns the all-reduced int64 accumulator into n of all orders, v, the odds table s, q, llh and v_diff.  It
exists as model_update_lds in k_update<true> (form 0), the same function in the prologue of the next pass's grouped or
mixed kernel (the fused update), k_update<false> (form 1) and the k_update_counts bands + k_update_model (form 2); the
older tests compare form with form on real data, where a mistake the forms share (count_tree, v_off, the statistics
decode) cannot show, and reach the oracle only as the tail of a whole pass at 1e-5.  Here an all-reduce callback
overwrites the pass's sums with a script, so the update is a pure function of integers the test chose, and n, v and s
must be the oracle's bits (orc.update_v, orc.linear_s on numpy's float32 chain of EM.cpp:247-254), llh the decoded word
(NaN under the flag), v_diff within one float32 ulp of the fsum, q within 2^-22 of the fp64 value of EM.cpp:515.  Every
case asserts EM.plan_update() first: a case cannot silently run another form.

Every case drives one handle through accumulate() + update() (no all-reduce: the row is written into reduce_buffer()),
EStep() (k_stat_only) + MStep(), and iterate(2): four updates, three entry points, inside and outside the q window.

Shapes that had never run before this file: the LDS form at K = 4 -- (4,1) and (4,2), the only widths it exists for,
through count_tree<4>, the `default:` branch of the depth switch; the form's boundary 4^(K+1) W = 2048 exactly -- (2,32),
(3,8), (4,2): two cells per thread in vo0 / vo1 -- and one cell past it -- (2,33), (3,9), (4,3), (5,1) -- in both global
forms; W <= K, where every column of the top orders is the `j < k` copy -- (2,1), (2,2), (4,1), (4,2), (4,3), (5,1),
K = 3..7 at W = 3; bands of every parity (K = 3 at W = 9, K = 4..7 at W = 3: (3,3) has 768 cells, which launch_update
keeps in the LDS form whatever the tuning, so that case asserts form 0); (7,5), whose 327 680 cells make
k_update_model's grid-stride loop run twice.

Mutation check (each mistake built for gfx950, this file and tests/test_optimize_script_gpu.py run, reverted):
  * `opt_iteration > 10u` -> `>= 10u` in model_update_lds only (stop_fires and the host keep `> 10`):
    test_optimize_script_gpu.py::test_llh_decrease_fires_only_past_iteration_10[plain], [fused_mixed] and
    [fused_grouped] fail -- the device stops at the drop of pass 10, the host goes on and reports "optimize(): pass 11
    ended without reporting its status" (an error, no hang); [bands] passes (k_update_model calls stop_fires), as do the
    other 98 cases.
  * count_tree<4> in the `default:` branch of model_update_lds replaced by count_tree<3>:
    test_random_sums_in_every_form_and_shape[K4_W1_form0] and [K4_W2_form0] fail at the counts of update(); the other
    99 cases of the two files pass (no other case runs K = 4 in the LDS form).
"""
import numpy as np
import pytest

from tests import coarse_unit as cu
from tests import update_script as us
from tests.test_regimes_gpu import open_em

pytestmark = pytest.mark.gpu

CAP = 8                                                      # max_iterations: the trace's capacity


def chain(orc, inp, rows, shift, v0, q0, windows, gsg=0):
    """expected_update of consecutive passes: rows[i] with the previous expectation's v and float32 q"""
    out, v, q = [], v0, q0
    for r, win in zip(rows, windows):
        e = us.expected_update(r, shift, inp.K, inp.W, min(inp.bg_order, inp.K), inp.A, inp.vbg, v, q, win, gsg, orc)
        out.append(e)
        v, q = e[1], float(np.float32(e[3]))
    return out


def assert_trace(em, exps, windows, first=0):
    llh, vd, q = em.trace()
    assert len(llh) == first + len(exps)
    for i, (e, win) in enumerate(zip(exps, windows)):
        p = first + i
        assert us.same_float(llh[p], e[4]), (p, llh[p], e[4])
        assert us.vdiff_ok(vd[p], e[7]), (p, vd[p], e[7])
        if win is None:                                      # an earlier call's pass: its q was checked then
            continue
        if win:
            assert us.q_ok(q[p], e[3]), (p, q[p], e[3])
        else:
            assert q[p] == np.float32(e[3]), (p, q[p], e[3])          # untouched: the bits it had


def assert_model(em, e, window, what):
    n, v, s, q, llh, _, _, d64 = e
    assert np.array_equal(us.bits(em.getCounts()), us.bits(n)), what
    assert np.array_equal(us.bits(em.getV()), us.bits(v)), what
    assert np.array_equal(us.bits(em.getS()), us.bits(s)), what
    assert us.same_float(em.getLLH(), llh), (what, em.getLLH(), llh)
    assert us.vdiff_ok(em.getVdiff(), d64), (what, em.getVdiff(), d64)
    assert (us.q_ok(em.getQ(), q) if window else em.getQ() == float(np.float32(q))), (what, em.getQ(), q)


def drive(ctx, orc, em, inp, rows, shift, optimize_q=True, gsg=0):
    """rows[0]: accumulate() + update(); rows[1] (statistics only): EStep(); rows[2]: MStep(); rows[3], rows[4]: iterate(2)"""
    e0 = chain(orc, inp, rows[:1], shift, em.getV(), em.getQ(), [optimize_q], gsg)[0]
    em.accumulate()
    us.poke(ctx, em, rows[0])
    em.update()                                              # the handle's first update: inside the q window
    assert_model(em, e0, optimize_q, "update()")
    sc = us.Scripted(ctx, em, rows[1:])
    try:
        q_before = em.getQ()
        em.EStep()
        llh_e, _, _ = us.decode_stats(rows[1][-3:])
        assert us.same_float(em.getLLH(), llh_e)
        assert not us.peek(ctx, em)[-3:].any()               # k_stat_only cleared its words
        assert em.getQ() == q_before
        e1 = chain(orc, inp, rows[2:3], shift, em.getV(), em.getQ(), [False], gsg)[0]
        em.MStep()                                           # EM::MStep never touches q
        assert_model(em, e1, False, "MStep()")
        e23 = chain(orc, inp, rows[3:5], shift, em.getV(), em.getQ(), [optimize_q] * 2, gsg)
        em.iterate(2)
        assert sc.calls == 4 and em.iteration() == 4
        assert_model(em, e23[1], optimize_q, "iterate(2)")
        assert_trace(em, [e0, e1] + e23, [optimize_q, False, optimize_q, optimize_q])
    finally:
        sc.close(ctx)


def five_rows(kind, seed, inp):
    rows = us.script(kind, seed, inp.K, inp.W, 5, inp.N)
    rows[1][:-3] = 0                                         # an E-only pass adds no counts
    return rows


# (K, W, tuning while the handle is created, the form plan_update() must report)
def _c(K, W, form, **tuning):
    return (K, W, dict(fused_update=0, **tuning), form)


SHAPE_CASES = (
    [_c(K, W, us.LDS) for K, W in [(0, 1), (0, 6), (1, 7), (2, 1), (2, 2), (2, 8), (3, 5), (4, 1)]] +
    [_c(K, W, us.LDS) for K, W in [(2, 32), (3, 8), (4, 2)]] +                                   # 2048 cells exactly
    [_c(K, W, f, update_blocks=b) for K, W in [(2, 33), (3, 9), (4, 3), (5, 1)] for f, b in ((us.ONE_BLOCK, 0), (us.BANDS, 1))] +
    [_c(3, 3, us.LDS, update_blocks=1)] +                  # 768 cells: launch_update keeps K = 3 at W = 3 in LDS; its bands run at (3,9)
    [_c(K, 3, us.BANDS, update_blocks=1) for K in (4, 5, 6, 7)] +                                # bands of every parity
    [_c(K, 3, us.ONE_BLOCK, update_blocks=0) for K in (6, 7)] +
    [_c(7, 5, us.BANDS, update_blocks=1)]                                                        # the grid-stride loop runs twice
)
ONE_PER_FORM = [_c(2, 8, us.LDS), _c(3, 9, us.ONE_BLOCK, update_blocks=0), _c(3, 9, us.BANDS, update_blocks=1)]


def case_id(c):
    return f"K{c[0]}_W{c[1]}_form{c[3]}"


def run_case(ctx, orc, case, kind="random", regime=None, bound=0, gsg=0, seed=1):
    K, W, tuning, form = case
    inp = us.tiny_inputs(orc, K, W, regime=regime)
    em, ss = us.open_tiny(ctx, inp, tuning, optimizeQ=True, max_iterations=CAP, n_seqs_bound=bound, n_seqs_global=gsg)
    try:
        assert em.plan_update() == (form, False), (em.plan_update(), case)
        shift = cu.fix_shift_of(bound or gsg or inp.N)
        drive(ctx, orc, em, inp, five_rows(kind, seed + 31 * K + W, inp), shift, gsg=gsg)
    finally:
        em.close(); ss.close()


@pytest.mark.parametrize("case", SHAPE_CASES, ids=case_id)
def test_random_sums_in_every_form_and_shape(case, gpu_ctx, orc):
    run_case(gpu_ctx, orc, case)


@pytest.mark.parametrize("kind", ["zero", "sparse", "wide"])
@pytest.mark.parametrize("case", ONE_PER_FORM, ids=case_id)
def test_zero_sparse_and_wide_sums(case, kind, gpu_ctx, orc):
    run_case(gpu_ctx, orc, case, kind=kind)


@pytest.mark.parametrize("shift", [32, 24])
@pytest.mark.parametrize("case", ONE_PER_FORM, ids=case_id)
def test_coarse_units_scale_the_counts(case, shift, gpu_ctx, orc):
    assert cu.fix_shift_of(cu.BOUNDS[shift]) == shift
    run_case(gpu_ctx, orc, case, bound=cu.BOUNDS[shift])


@pytest.mark.parametrize("regime", us.ALPHA_REGIMES)
@pytest.mark.parametrize("case", ONE_PER_FORM, ids=case_id)
def test_alpha_regimes(case, regime, gpu_ctx, orc):
    run_case(gpu_ctx, orc, case, regime=regime)


@pytest.mark.parametrize("case", ONE_PER_FORM, ids=case_id)
def test_n_seqs_global_replaces_the_count_word(case, gpu_ctx, orc):
    run_case(gpu_ctx, orc, case, gsg=1000)


# llh word positive / negative / zero; sum_r = 0, about N, beyond N + 1 (a negative q, as the formula gives it); the flag
# over a plausible count
STATS = {
    "llh_pos_sumr_0": lambda N: us.stats(12345.0 / us.LLH_UNIT + 3.0, 0.0, N),
    "llh_neg_sumr_N": lambda N: us.stats(-7.0 - 1.0 / us.LLH_UNIT, N - 3.0 / us.SUMR_UNIT, N),
    "llh_0_sumr_past_N": lambda N: us.stats(0.0, N + 1.5, N),
    "bad_flag": lambda N: us.stats(2.5, 1.25, N, bad=3),
}


@pytest.mark.parametrize("name", sorted(STATS))
@pytest.mark.parametrize("case", ONE_PER_FORM, ids=case_id)
def test_statistics_words(case, name, gpu_ctx, orc):
    """one update on sums whose statistics words are the case's; the sequence kernels never see the q it leaves"""
    K, W, tuning, form = case
    inp = us.tiny_inputs(orc, K, W)
    em, ss = us.open_tiny(gpu_ctx, inp, tuning, optimizeQ=True, max_iterations=CAP)
    try:
        assert em.plan_update() == (form, False)
        r = us.row(us.counts_random(np.random.RandomState(5), K, W), STATS[name](inp.N))
        e = chain(orc, inp, [r], 40, em.getV(), em.getQ(), [True])[0]
        em.accumulate()
        us.poke(gpu_ctx, em, r)
        em.update()
        assert_model(em, e, True, name)
        assert_trace(em, [e], [True])
        if name == "llh_0_sumr_past_N":
            assert em.getQ() < 0 and em.getLLH() == 0.0
        if name == "bad_flag":
            assert np.isnan(em.getLLH()) and np.isnan(em.trace()[0][0]) and us.q_ok(em.getQ(), (inp.N - 1.25 + 1) / (inp.N + 2))
        assert not us.peek(gpu_ctx, em).any()                # consumed and zeroed
    finally:
        em.close(); ss.close()


def test_estep_alone_reports_nan_under_the_flag(gpu_ctx, orc):
    inp = us.tiny_inputs(orc, 1, 7)
    em, ss = us.open_tiny(gpu_ctx, inp, dict(fused_update=0), max_iterations=CAP)
    zeros = np.zeros(us.cells_of(1, 7), np.int64)
    sc = us.Scripted(gpu_ctx, em, [us.row(zeros, us.stats(2.5, 1.25, inp.N, bad=1)), us.row(zeros, us.stats(-2.5, 1.25, inp.N))])
    try:
        em.EStep()
        assert np.isnan(em.getLLH()) and not us.peek(gpu_ctx, em).any()
        em.EStep()
        assert em.getLLH() == -2.5 and not us.peek(gpu_ctx, em).any() and em.iteration() == 0
    finally:
        sc.close(gpu_ctx); em.close(); ss.close()


# ---------------------------------------------------------------------------- the fused prologue --

FUSED_FLAVOURS = ["grouped_6mer", "grouped_g5", "layout0_k1_ss", "mixed_a1", "mixed_w20"]


def run_fused(ctx, orc, flavour, kind="random", regime="base", bound=0):
    """iterate(4) on a four-row script: the updates of passes 1-3 run in the prologue of passes 2-4, the last one is
    k_update<true>; every intermediate model through the trace, the final one in full -- and the same bits from a twin
    created under fused_update = 0"""
    inp = us.flavour_inputs(orc, flavour, regime)
    rows = us.script(kind, 77, inp.K, inp.W, 4, inp.N)
    shift = cu.fix_shift_of(bound or inp.N)
    outs = []
    for fused in (True, False):
        ctx.set_tuning(fused_update=int(fused))
        try:
            em, ss = open_em(ctx, inp, flavour, optimizeQ=True, max_iterations=CAP, n_seqs_bound=bound)
        finally:
            ctx.set_tuning(fused_update=1)
        sc = us.Scripted(ctx, em, rows)
        try:
            assert em.plan_update() == (us.LDS, fused), (flavour, em.plan_update())
            exps = chain(orc, inp, rows, shift, em.getV(), em.getQ(), [True] * 4)
            em.iterate(4)
            assert sc.calls == 4 and em.iteration() == 4
            assert_model(em, exps[3], True, (flavour, fused))
            assert_trace(em, exps, [True] * 4)
            outs.append((em.getV(), em.getCounts(), em.getS(), em.getQ(), em.trace()[0], em.trace()[2]))
        finally:
            sc.close(ctx); em.close(); ss.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("flavour", FUSED_FLAVOURS)
def test_fused_prologue_random_sums(flavour, gpu_ctx, orc):
    run_fused(gpu_ctx, orc, flavour)


@pytest.mark.parametrize("kind", ["zero", "sparse", "wide"])
def test_fused_prologue_zero_sparse_and_wide_sums(kind, gpu_ctx, orc):
    run_fused(gpu_ctx, orc, "mixed_w20", kind=kind)


@pytest.mark.parametrize("shift", [32, 24])
def test_fused_prologue_coarse_units(shift, gpu_ctx, orc):
    run_fused(gpu_ctx, orc, "mixed_w20", bound=cu.BOUNDS[shift])


@pytest.mark.parametrize("regime", us.ALPHA_REGIMES)
def test_fused_prologue_alpha_regimes(regime, gpu_ctx, orc):
    run_fused(gpu_ctx, orc, "mixed_w20", regime=regime)
