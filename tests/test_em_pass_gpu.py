"""What a pass is described by (csrc/handles.h: EmPass), seen from outside: the E pass that getR() / sites() replay on a
sliced handle runs without the fold mask and outside the call's kernel timing and leaves mask, timing samples and the
model's trajectory as they were; a handle's `optimize_q` reaches the model update only inside the q window of iterate()
/ optimize().  Bit equality throughout (the same kernels on the same inputs), tests/test_sites_gpu.py's small shapes."""
import numpy as np
import pytest

from tests.test_parity_gpu import make_em
from tests.test_sites_gpu import bench_shape, long_mixed, make, sliced_shape  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
E_FUSED = pytest.mark.parametrize("e_fused", [1, 0], ids=["e_fused", "slot_indexed"])


def fold_mask(c):
    return (np.arange(c.N) % 3 != 0).astype(np.uint8)


@pytest.mark.parametrize("every,two_passes", [(1, 2), (3, 1), (0, 0), (-1, 2)], ids=["every", "third", "none", "whole_call"])
@E_FUSED
def test_replay_leaves_timing_alone(e_fused, every, two_passes, sliced_shape, gpu_ctx):
    """kernel_time() after getR() / sites() reports what it reported before them, in every timing mode.  (Before the replay
    became an untimed pass, whole_call counted one pass more per read-out -- 6 for 4 here -- over an interval spanning it.)"""
    c = sliced_shape
    ss, em = make(gpu_ctx, c, e_fused=e_fused)
    assert em.plan_paths()[:2] == (True, bool(e_fused))
    em.set_kernel_timing(every)
    em.iterate(4)
    ms, n = em.kernel_time()
    assert n == {1: 4, 3: 2, 0: 0, -1: 4}[every]
    em.getR()
    em.sites_and_best(0.3)
    ms2, n2 = em.kernel_time()
    print(f"e_fused={e_fused} every={every}: before the read-outs ({ms!r}, {n}), after ({ms2!r}, {n2})")
    assert n2 == n
    assert np.float32(ms2).view(np.uint32) == np.float32(ms).view(np.uint32)
    em.iterate(2)
    assert em.kernel_time()[1] == two_passes
    em.close(); ss.close()


@E_FUSED
def test_replay_leaves_mask_and_trajectory_alone(e_fused, sliced_shape, gpu_ctx):
    c = sliced_shape
    mask = fold_mask(c)
    ss, em = make(gpu_ctx, c, mask=mask, e_fused=e_fused)
    _, twin = make(gpu_ctx, c, mask=mask, ss=ss, e_fused=e_fused)
    em.iterate(3); twin.iterate(3)
    em.getR()
    em.getR(5, 33)
    _, (_, _, count) = em.sites_and_best(0.0)
    assert (count[mask == 0] == ss.lengths[mask == 0] - c.W + 1).all()      # masked-out sequences list every window
    assert (count == ss.lengths - c.W + 1).all()
    em.iterate(2); twin.iterate(2)
    assert np.array_equal(em.getV().view(np.uint32), twin.getV().view(np.uint32))
    assert em.iteration() == twin.iteration() == 5
    em.close(); twin.close(); ss.close()


@pytest.mark.parametrize("shape,tune", [("sliced_shape", {"e_fused": 1}), ("sliced_shape", {"e_fused": 0}), ("bench_shape", {}), ("long_mixed", {})],
                         ids=["sliced_e_fused", "sliced_slot_indexed", "k2_planner", "long_record"])
def test_read_out_ignores_the_mask(shape, tune, request, gpu_ctx):
    """At the seed model, no pass run: getR() of a masked handle is the unmasked handle's."""
    c = request.getfixturevalue(shape)
    ss, masked = make(gpu_ctx, c, mask=fold_mask(c), **tune)
    _, plain = make(gpu_ctx, c, ss=ss, **tune)
    if shape == "long_mixed":
        assert plain.plan_paths()[2] == 1
    a, b = masked.getR(), plain.getR()
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.count_nonzero(a) > 0
    masked.close(); plain.close(); ss.close()


def test_estep_mstep_never_touch_q(bench_shape, gpu_ctx, orc):
    """EM::MStep leaves q alone whatever the handle's optimize_q says; the q window of iterate() does not."""
    c = bench_shape
    em, ss, *_ = make_em(gpu_ctx, c, orc, optimizeQ=True)
    q0 = np.float32(em.getQ())
    em.EStep(); em.MStep()
    assert np.float32(em.getQ()).view(np.uint32) == q0.view(np.uint32)
    em.iterate(1)
    assert np.float32(em.getQ()) != q0
    em.close(); ss.close()


def test_mask_with_optimize_q_keeps_the_order_0_chain(bench_shape, gpu_ctx, orc):
    """EM::mask with optimizeQ: q after the call is the order-0 pass's per-sequence chain (EM.cpp:321) and nothing the
    masked iterations did -- the reference restatement's value, bit for bit (the check of tests/test_mask_gpu.py's
    test_mask_three_passes_match_oracle[optq], on this file's shape)."""
    c = bench_shape
    em, ss, kmer, off, vbg = make_em(gpu_ctx, c, orc, optimizeQ=True, epsilon=0.0, max_iterations=3)
    assert em.mask(0.05) == 3
    res = orc.mask(kmer, off, c.K, c.W, c.bg_order, vbg, c.A, c.v0, c.q, optimizeQ=True, f=0.05, epsilon=0.0, max_iter=3)
    q = np.float32(em.getQ())
    print(f"q after mask(0.05): {q!r} (bits {q.view(np.uint32):#010x}), restatement {np.float32(res['q'])!r}")
    assert q.view(np.uint32) == np.float32(res["q"]).view(np.uint32)
    assert q != np.float32(c.q)
    em.close(); ss.close()
