"""The model update fused into the next pass's kernel (csrc/update_kernel.h) against the k_update launch.

Inside iterate() / optimize() a fusable handle (K <= 2-sized tables, first launch a grouped kernel) runs
update(p) in the block prologue of pass p+1's first kernel: the same device function k_update<true> runs, on the
same integers, so the models, counts, q and the log-likelihood trace must be IDENTICAL bits; v_diff is a block
reduction whose grouping follows the block size (fp64 partials: equal to the last float bit except on ties).
Reference lines the update restates: EM.cpp:247-254, Motif.h:95-136, EM.cpp:515, EM.cpp:102-118.
"""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import synth

pytestmark = pytest.mark.gpu


def build(ctx, N, L0, W, K, ss=False, n_frac=0.0, ragged=0, seed=5, fused=True, mask=None, **kw):
    pwm = synth.make_pwm(W, seed)
    codes, in_off = synth.make_sequences(N, L0, pwm, seed, 0.5, n_frac, ragged)
    packed = bm.PackedSeqs.from_codes(codes, in_off, ss, seed=42)
    A = synth.alpha_matrix(synth.default_alpha(K), W)
    vbg = packed.bg_model(2, np.array([1.0, 10.0, 10.0], np.float32))
    v0 = synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K)
    ctx.set_tuning(fused_update=int(fused))
    try:
        seqs = bm.SeqSet(ctx, packed)
        em = bm.EM(ctx, seqs, K, W, vbg, A, v0, 0.3, mask=mask, **kw)
    finally:
        ctx.set_tuning(fused_update=1)
    assert em.plan_update() == (0, fused)                    # a shape the planner declines to fuse compares nothing
    return em, seqs


def same_trace(a, b):
    (la, va, qa), (lb, vb, qb) = a, b
    assert np.array_equal(la, lb) and np.array_equal(qa, qb)
    np.testing.assert_allclose(va, vb, rtol=3e-7, atol=0)


SHAPES = [
    dict(N=3000, L0=200, W=20, K=2),                       # both strands: mixed rows when large enough, else uniform rows
    dict(N=2000, L0=120, W=12, K=2, n_frac=0.01, ragged=30),   # N exceptions: a per-column launch follows the fused one
    dict(N=1500, L0=130, W=9, K=1, ss=True),               # 3 positions per lane: the shortest class K = 1 has a grouped kernel for (G = 3)
    dict(N=1200, L0=150, W=15, K=0, ragged=20),
    dict(N=45000, L0=200, W=20, K=2),                      # enough work for the mixed-row kernel
]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"N{d['N']}_K{d['K']}_W{d['W']}" for d in SHAPES])
def test_iterate_fused_equals_unfused_bit_for_bit(shape, gpu_ctx):
    outs = []
    for fused in (True, False):
        em, seqs = build(gpu_ctx, fused=fused, optimizeQ=True, max_iterations=40, **shape)
        em.iterate(7)
        em.iterate(1)                                        # a one-pass call has nothing to fuse into
        em.iterate(4)
        outs.append((em.getV(), em.getCounts(), em.getQ(), em.getS(), em.trace(), em.iteration(), em.getR(0, 50), em.getLLH()))
        em.close(); seqs.close()
    a, b = outs
    assert a[5] == b[5] == 12
    for i in (0, 1, 3, 6):
        assert np.array_equal(a[i], b[i]), i
    assert a[2] == b[2] and a[7] == b[7]
    same_trace(a[4], b[4])


def test_fused_then_stepwise_calls_share_one_state(gpu_ctx):
    """iterate() leaves the handle exactly where EStep()/MStep() expect it (accumulator ring clean, s / q / v current)."""
    outs = []
    for fused in (True, False):
        em, seqs = build(gpu_ctx, N=4000, L0=200, W=20, K=2, fused=fused, optimizeQ=True, max_iterations=30)
        em.iterate(5)
        em.EStep(); em.MStep(); em.optimize_q()
        em.iterate(3)
        em.accumulate(); em.update()
        outs.append((em.getV(), em.getCounts(), em.getQ(), em.trace()))
        em.close(); seqs.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    same_trace(outs[0][3], outs[1][3])


@pytest.mark.parametrize("shape", SHAPES[:3] + SHAPES[4:], ids=[f"N{d['N']}_K{d['K']}_W{d['W']}" for d in SHAPES[:3] + SHAPES[4:]])
def test_optimize_fused_stops_where_unfused_stops(shape, gpu_ctx):
    """The stop rule (EM.cpp:117-118) evaluated inside the fused prologue by every block: same pass count, same
    model, same responsibilities afterwards (EM::getR sees the E-step of the LAST pass), and the handle keeps working."""
    outs = []
    for fused in (True, False):
        em, seqs = build(gpu_ctx, fused=fused, optimizeQ=True, max_iterations=200, epsilon=0.01, **shape)
        it = em.optimize()
        first = (it, em.getV(), em.getCounts(), em.getQ(), em.getR(0, 40), em.trace(), em.getLLH(), em.getVdiff(), em.iteration())
        it2 = em.optimize()                                  # a second call starts from the first one's model
        outs.append(first + (it2, em.getV(), em.iteration()))
        em.close(); seqs.close()
    a, b = outs
    assert a[0] == b[0] and a[8] == b[8] == a[0], (a[0], b[0])
    assert 1 < a[0] < 200
    for i in (1, 2, 4, 10):
        assert np.array_equal(a[i], b[i]), i
    assert a[3] == b[3] and a[6] == b[6] and a[9] == b[9] and a[11] == b[11]
    same_trace(a[5], b[5])


def test_optimize_budget_ends_without_the_rule(gpu_ctx):
    """max_iterations reached: the last pass's update is the k_update launch; nothing is rolled back."""
    outs = []
    for fused in (True, False):
        em, seqs = build(gpu_ctx, N=3000, L0=200, W=20, K=2, fused=fused, max_iterations=6, epsilon=0.0)
        assert em.optimize() == 6
        outs.append((em.getV(), em.getCounts(), em.trace(), em.getR(0, 30)))
        em.iterate(2)                                        # the ring is clean
        outs[-1] += (em.getV(),)
        em.close(); seqs.close()
    for i in (0, 1, 3, 4):
        assert np.array_equal(outs[0][i], outs[1][i]), i
    same_trace(outs[0][2], outs[1][2])


def test_fused_with_fold_mask_and_two_handles(gpu_ctx):
    """CV folds: several handles over one resident set, each with its own ring and per-block tables."""
    N = 3000
    mask = (np.arange(N) % 5 != 2).astype(np.uint8)
    outs = []
    for fused in (True, False):
        em1, seqs = build(gpu_ctx, N=N, L0=200, W=20, K=2, fused=fused, mask=mask, max_iterations=20)
        gpu_ctx.set_tuning(fused_update=int(fused))
        em2 = bm.EM(gpu_ctx, seqs, em1.K, em1.W, *_model_of(em1), 0.3, max_iterations=20)
        gpu_ctx.set_tuning(fused_update=1)
        em1.iterate(3); em2.iterate(2); em1.iterate(2); em2.iterate(3)
        outs.append((em1.getV(), em2.getV()))
        em1.close(); em2.close(); seqs.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert not np.array_equal(outs[0][0], outs[0][1])


def _model_of(em):
    """(vbg, A, v) a second handle over the same set can start from."""
    K, W = em.K, em.W
    A = synth.alpha_matrix(synth.default_alpha(K), W)
    vbg = np.full(bm.bg_size(2), 0.25, np.float32)
    return vbg, A, em.getV()
