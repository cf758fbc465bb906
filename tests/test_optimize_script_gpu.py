"""optimize()'s loop control on scripted sums (tests/update_script.py): the stop rule's branches, one float either side.

The device evaluates EM.cpp:117-118 in stop_fires / model_update_lds (csrc/update_kernel.h); the host, running one or two
units ahead, evaluates a copy in bamm_em_optimize (csrc/em.cpp).  If the two disagree the host waits for a pass that did
nothing.  Real data never placed v_diff beside epsilon, never made `llh decreased && iteration > 10` fire or not fire at
will, never fed the rule a NaN llh and never ran the q window (EM.cpp:99) to its edge.  Here every pass's sums are a row
of a script: v after a pass is a function of that pass's counts alone, so a script that alternates two rows has
v_diff = D in every pass but the first (D1 > D: tests/test_update_script_cpu.py), one that repeats a row has v_diff = 0,
and llh / sum_r are whatever the row's words say.

Every case runs on a plain handle (per_column: k_update<true> per pass), two fused handles (mixed_w20, grouped_6mer: the
rule inside the next pass's prologue, status one unit late) and a band-form handle ((3,9), update_blocks = 1: stop_fires in
k_update_model), each asserted through plan_update().  A script has exactly as many rows as passes expected: the
look-ahead units behind the raised flag find no row, as a real all-reduce would sum untouched zeros.  After every stop at
pass s: iteration() == s, the trace has s rows equal to expected_update's, the model is pass s's bits, the callback was
called at most s + 2 times, and iterate(1) without the callback gives the bits a fresh handle created from (getV(),
getQ()) gives -- the look-ahead left nothing in the accumulator or its ring.

Mutation check: see tests/test_update_exact_gpu.py.
"""
import copy

import numpy as np
import pytest

from tests import update_script as us
from tests.test_regimes_gpu import open_em
from tests.test_update_exact_gpu import assert_model, assert_trace, chain

pytestmark = pytest.mark.gpu

KINDS = sorted(us.LOOP_KINDS)


def open_kind(ctx, orc, kind, v=None, q=None, **kw):
    d, inp = us.LOOP_KINDS[kind], us.loop_inputs(orc, kind)
    if "flavour" in d:
        if v is not None:
            inp = copy.copy(inp)
            inp.v = np.ascontiguousarray(v, np.float32)
        em, ss = open_em(ctx, inp, d["flavour"], q=q, **kw)
    else:
        em, ss = us.open_tiny(ctx, inp, d["tuning"], v=v, q=q, **kw)
    assert em.plan_update() == (d["form"], d["fusable"]), (kind, em.plan_update())
    return em, ss, inp


def rising(n, start=1.0):
    return [start + p for p in range(n)]


def run_optimize(ctx, orc, em, inp, rows, windows, expect_passes, first=0, history=()):
    """optimize() on the script: returns after `expect_passes`, having left exactly those passes' trace and the last
    one's model; returns every expectation so far (history + this call's)"""
    sc = us.Scripted(ctx, em, rows)
    try:
        exps = chain(orc, inp, rows[:expect_passes], 40, em.getV(), em.getQ(), windows[:expect_passes])
        done = em.optimize()
        assert done == expect_passes, (done, expect_passes)
        assert em.iteration() == first + expect_passes
        assert sc.calls <= expect_passes + 2, sc.calls
        assert_model(em, exps[-1], windows[expect_passes - 1], "optimize()")
        assert_trace(em, list(history) + exps, [None] * len(history) + list(windows[:expect_passes]))
    finally:
        sc.close(ctx)
    return list(history) + exps


def nothing_left_behind(ctx, orc, kind, em, **kw):
    """with the callback removed, one more pass equals a fresh handle's first pass from the same model: the real kernels'
    integer sums, so the same bits -- unless the look-ahead units left something in the accumulator or its ring"""
    v, q = em.getV(), em.getQ()
    em.iterate(1)
    fresh, ss2, _ = open_kind(ctx, orc, kind, v=v, q=q, **kw)
    try:
        fresh.iterate(1)
        for a, b in ((em.getV(), fresh.getV()), (em.getCounts(), fresh.getCounts()), (em.getS(), fresh.getS())):
            assert np.array_equal(us.bits(a), us.bits(b))
        assert us.same_float(em.getLLH(), fresh.getLLH()) and em.getQ() == fresh.getQ()
    finally:
        fresh.close(); ss2.close()


def assert_trace_q_frozen(em, first, last, like):
    q = em.trace()[2]
    assert all(q[p] == q[like] for p in range(first, last)), (q[like], q[first:last])


@pytest.mark.parametrize("kind", KINDS)
def test_v_diff_below_epsilon_is_strict(kind, gpu_ctx, orc):
    _, D = us.knife_edge(orc, kind)
    Df = np.float32(D)
    c0, c1 = us.two_rows(kind, us.loop_inputs(orc, kind))
    for eps, passes in ((Df, 4), (np.nextafter(Df, np.float32(np.inf)), 2)):
        kw = dict(epsilon=float(eps), max_iterations=4)
        em, ss, inp = open_kind(gpu_ctx, orc, kind, **kw)
        try:
            rows = us.loop_rows([c0, c1], rising(passes), [0.0] * passes, inp.N)
            exps = run_optimize(gpu_ctx, orc, em, inp, rows, [False] * passes, passes)
            assert np.float32(em.trace()[1][1]) == Df           # pass 2 sat exactly on float32(D)
            assert np.float32(exps[1][7]) == Df
            nothing_left_behind(gpu_ctx, orc, kind, em, **kw)
        finally:
            em.close(); ss.close()


@pytest.mark.parametrize("kind", KINDS)
def test_identical_rows_stop_at_pass_2_unless_epsilon_is_zero(kind, gpu_ctx, orc):
    c0, _ = us.two_rows(kind, us.loop_inputs(orc, kind))
    for eps, passes in ((2e-38, 2), (0.0, 6)):               # any epsilon > 0; 0 < 0 never holds: on to max_iterations
        kw = dict(epsilon=eps, max_iterations=6)
        em, ss, inp = open_kind(gpu_ctx, orc, kind, **kw)
        try:
            rows = us.loop_rows([c0], rising(passes), [0.0] * passes, inp.N)
            run_optimize(gpu_ctx, orc, em, inp, rows, [False] * passes, passes)
            assert (em.trace()[1][1:] == 0.0).all() and em.trace()[1][0] > 0
            nothing_left_behind(gpu_ctx, orc, kind, em, **kw)
        finally:
            em.close(); ss.close()


# passes 1..11: drops at 5 and 10, an equal value at 8 -- none stops; the drop at 11 does
LLH_FIRST = [1.0, 2.0, 3.0, 4.0, 3.5, 5.0, 6.0, 6.0, 7.0, 6.5, 6.25]
# a second call counts from 1 again and compares its first pass with 6.25: drops at 1, 7 and 10 pass, the one at 11 stops
LLH_SECOND = [6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 10.5, 12.0, 13.0, 12.5, 12.25]


@pytest.mark.parametrize("kind", KINDS)
def test_llh_decrease_fires_only_past_iteration_10(kind, gpu_ctx, orc):
    kw = dict(epsilon=0.0, max_iterations=24)
    em, ss, inp = open_kind(gpu_ctx, orc, kind, **kw)
    c = us.two_rows(kind, inp)
    try:
        rows = us.loop_rows(c, LLH_FIRST, [0.0] * 11, inp.N)
        hist = run_optimize(gpu_ctx, orc, em, inp, rows, [False] * 11, 11)
        rows = us.loop_rows(c[::-1], LLH_SECOND, [0.0] * 11, inp.N)
        run_optimize(gpu_ctx, orc, em, inp, rows, [False] * 11, 11, first=11, history=hist)
        nothing_left_behind(gpu_ctx, orc, kind, em, **kw)
    finally:
        em.close(); ss.close()


@pytest.mark.parametrize("kind", KINDS)
def test_nan_llh_does_not_stop_and_neither_does_the_pass_after_it(kind, gpu_ctx, orc):
    """the bad flag at pass 12: NaN - x < 0 and, a pass later, x - NaN < 0 are both false; the next real drop stops"""
    kw = dict(epsilon=0.0, max_iterations=24)
    em, ss, inp = open_kind(gpu_ctx, orc, kind, **kw)
    try:
        llh = rising(11) + [99.0, 0.5, 0.25]                # 12: flagged (the word's 99 is never seen); 13: far below 11's; 14: a drop
        rows = us.loop_rows(us.two_rows(kind, inp), llh, [0.0] * 14, inp.N, bad=(12,))
        run_optimize(gpu_ctx, orc, em, inp, rows, [False] * 14, 14)
        t = em.trace()[0]
        assert np.isnan(t[11]) and t[12] == 0.5 and t[13] == 0.25
        nothing_left_behind(gpu_ctx, orc, kind, em, **kw)
    finally:
        em.close(); ss.close()


@pytest.mark.parametrize("kind", KINDS)
def test_q_window_closes_after_pass_5_and_reopens_with_the_next_call(kind, gpu_ctx, orc):
    """EM.cpp:99: q follows the script's sum_r in passes 1-5 of iterate(7) and of each optimize(), and keeps its bits from
    pass 6 on"""
    kw = dict(epsilon=0.0, max_iterations=32, optimizeQ=True)
    em, ss, inp = open_kind(gpu_ctx, orc, kind, **kw)
    c = us.two_rows(kind, inp)
    sum_r = lambda n, base: [base + 0.5 * p + 1.0 / us.SUMR_UNIT for p in range(n)]      # every pass another q
    try:
        rows = us.loop_rows(c, rising(7), sum_r(7, 0.25), inp.N)
        sc = us.Scripted(gpu_ctx, em, rows)
        try:
            win = [True] * 5 + [False] * 2
            hist = chain(orc, inp, rows, 40, em.getV(), em.getQ(), win)
            em.iterate(7)
            assert sc.calls == 7
            assert_trace(em, hist, win)
        finally:
            sc.close(gpu_ctx)
        assert_trace_q_frozen(em, 5, 7, like=4)
        win = [True] * 5 + [False] * 6
        for call, base in enumerate((1.0, 2.125)):
            llh = rising(10, 10.0 + 20.0 * call) + [0.0]     # the drop at pass 11 ends the call
            first = 7 + 11 * call
            hist = run_optimize(gpu_ctx, orc, em, inp, us.loop_rows(c, llh, sum_r(11, base), inp.N), win, 11, first=first, history=hist)
            assert_trace_q_frozen(em, first + 5, first + 11, like=first + 4)
            q = em.trace()[2]
            assert len({float(x) for x in q[first:first + 5]} | {float(q[first - 1])}) == 6     # the window moved q in each of its passes
        nothing_left_behind(gpu_ctx, orc, kind, em, **kw)
    finally:
        em.close(); ss.close()


def test_hand_driven_updates_have_the_handles_first_five_in_the_window(gpu_ctx, orc):
    """bamm_em_update: hand-driven passes have no optimize() call to be local to -- the handle's first five updates"""
    kind = "plain"
    em, ss, inp = open_kind(gpu_ctx, orc, kind, optimizeQ=True, max_iterations=8)
    c = us.two_rows(kind, inp)
    try:
        rows = us.loop_rows(c, rising(6), [0.5 * (p + 1) for p in range(6)], inp.N)
        win = [True] * 5 + [False]
        exps = chain(orc, inp, rows, 40, em.getV(), em.getQ(), win)
        for r in rows:
            em.accumulate()
            us.poke(gpu_ctx, em, r)
            em.update()
        assert_model(em, exps[-1], False, "sixth update()")
        assert_trace(em, exps, win)
        assert_trace_q_frozen(em, 5, 6, like=4)
    finally:
        em.close(); ss.close()
