"""Every device block a sequence set or an EM handle allocates is back with the library once both are destroyed.

bamm_device_blocks_live counts the blocks handed to an owner and not yet returned (idle blocks of a context's scratch
pool do not count).  Each flavour below takes one path through the allocations of bamm_em / bamm_seqs (csrc/handles.h),
checks through the plan read-outs that it really took it, and runs its create / use / destroy cycle twice: the count
must be where it started after each, so neither a forgotten block nor a once-only allocation hides a per-cycle leak."""
import threading

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi, synth

pytestmark = pytest.mark.gpu


def _two_classes_with_n_runs():
    """96 sequences of 40-60 and 100-120 bp (two length classes on both strands); six carry a run of 15 N, more than the
    grouped kernel's virtual rows take, so those go one column at a time."""
    pwm = synth.make_pwm(12, 11)
    c1, o1 = synth.make_sequences(48, 50, pwm, 11, ragged=10)
    c2, o2 = synth.make_sequences(48, 110, pwm, 12, ragged=10)
    codes, off = np.concatenate([c1, c2]), np.concatenate([o1, o1[-1] + o2[1:]])
    for i in (0, 9, 20, 50, 61, 90):
        codes[int(off[i]) + 10:int(off[i]) + 25] = 0
    return codes, off


def _ragged(N, lo, hi, seed):
    return synth.make_sequences(N, (lo + hi) // 2, synth.make_pwm(20, seed), seed, ragged=(hi - lo) // 2)


@pytest.fixture(scope="module")
def packed():
    """The packed sets of the flavours, made once (host memory only)."""
    sets = dict(first=_two_classes_with_n_runs(), mixed=_ragged(64, 100, 150, 21), one_class=_ragged(64, 100, 124, 22),
                sliced=synth.make_sequences(48, 200, synth.make_pwm(30, 23), 23), large=_ragged(20000, 100, 150, 24))
    return {k: bm.PackedSeqs.from_codes(codes, off, False, seed=42) for k, (codes, off) in sets.items()}


@pytest.fixture()
def ctx(lib):
    c = bm.Context(0)
    c.set_tuning(scratch_poison=1)
    yield c
    c.close()


def _model(pk, K, W, seed=5):
    pwm = synth.make_pwm(W, seed)
    return (pk.bg_model(2, np.array([1, 10, 10], np.float32)), synth.alpha_matrix(synth.default_alpha(K), W),
            synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K))


def _em(ctx, ss, pk, K, W, **kw):
    vbg, A, v0 = _model(pk, K, W)
    return bm.EM(ctx, ss, K, W, vbg, A, v0, 0.3, **kw)


def _twice(cycle):
    start = bm.device_blocks_live()
    for _ in range(2):
        cycle(start)
        assert bm.device_blocks_live() == start


def _one_handle(ctx, pk, K, W, use, check_plan, tuning=None, **kw):
    """cycle(start): set + handle on `ctx` (the test's own, under `tuning`), check_plan(em), use(em), destroy both."""
    ctx.set_tuning(**(tuning or {}))

    def cycle(start):
        ss = bm.SeqSet(ctx, pk)
        em = _em(ctx, ss, pk, K, W, **kw)
        assert bm.device_blocks_live() > start
        check_plan(em)
        use(em)
        ctx.sync()
        em.close(); ss.close()
    return cycle


def _grouped_and_percolumn(em):
    g, o, _ = em.plan()
    assert g > 0 and o > 0                                   # both index lists exist


def test_grouped_and_percolumn_lists_optimize(ctx, packed):
    _twice(_one_handle(ctx, packed["first"], 2, 12, lambda em: em.optimize(), _grouped_and_percolumn, max_iterations=8))


def test_fold_mask(ctx, packed):
    mask = (np.arange(96) % 4 != 0).astype(np.uint8)
    _twice(_one_handle(ctx, packed["first"], 2, 12, lambda em: em.iterate(2), _grouped_and_percolumn, mask=mask))


def test_mixed_rows(ctx, packed):
    def mixed(em):
        assert em.plan_mixed() > 0                           # lane records, the fix lanes' log
    _twice(_one_handle(ctx, packed["mixed"], 2, 20, lambda em: em.iterate(2), mixed, tuning=dict(group_layout=8)))


def test_order_three_through_the_grouped_kernel(ctx, packed):
    def grouped(em):
        assert em.plan()[0] > 0                              # the uniform-row kernel's fix log
    _twice(_one_handle(ctx, packed["first"], 3, 12, lambda em: em.iterate(2), grouped))


@pytest.mark.parametrize("e_fused", [1, 0])
def test_sliced(e_fused, ctx, packed):
    def sliced(em):
        assert em.plan_paths()[:2] == (True, bool(e_fused))  # lists, d_nnz, d_state, the update over blocks
    _twice(_one_handle(ctx, packed["sliced"], 4, 30, lambda em: em.iterate(3), sliced, tuning=dict(e_fused=e_fused)))


@pytest.mark.parametrize("optimize_q", [False, True])
def test_mask(optimize_q, ctx, packed):
    def use(em):
        assert em.mask(0.3) >= 1 and em.last_mask["listed"] > 0
    _twice(_one_handle(ctx, packed["first"], 2, 12, use, lambda em: None, optimizeQ=optimize_q, max_iterations=4))


def test_caller_owned_reduce_buffer(ctx, packed):
    """The accumulator ring is released when the caller's buffer takes its place; that buffer is torch's, not counted."""
    import torch

    def use(em):
        before = bm.device_blocks_live()
        _, n = em.reduce_buffer()
        red = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        em.set_reduce_buffer(red.data_ptr(), n)
        assert bm.device_blocks_live() == before - 1
        em.iterate(2)
        ctx.sync()
        em._red = red                                        # alive until the handle is closed
    _twice(_one_handle(ctx, packed["first"], 2, 12, use, lambda em: None))


@pytest.mark.parametrize("which", ["mixed", "one_class"])
def test_two_ranks_on_one_device(which, lib, packed):
    """verify_comm's words on every rank; with one length class the ranks can agree on the in-kernel all-reduce, whose words
    then exist as well (two classes are two launches per pass: the vote keeps the collective).  The mode is printed, not
    asserted: tests/test_peer_allreduce_gpu.py checks the vote."""
    pk, K, W = packed[which], 2, 20
    vbg, A, v0 = _model(pk, K, W)

    def cycle(start):
        ctxs = [bm.Context(0), bm.Context(0)]
        for x in ctxs:
            x.set_tuning(peer_allreduce=1, group_layout=8)
            x.set_launch(112, 0)                             # the ranks' kernels are resident side by side: they wait for each other
        comms = bm.Comm.init_local(ctxs, 4 ** (K + 1) * W + 3)
        sets, ems = [], []
        for r in range(2):
            b, e = pk.shard_range(W, r, 2)
            sets.append(bm.SeqSet(ctxs[r], pk, b, e))
            ems.append(bm.EM(ctxs[r], sets[r], K, W, vbg, A, v0, 0.3, n_seqs_global=pk.n_seqs, n_seqs_bound=pk.n_seqs))
            ems[r].set_comm(comms[r])
            assert ems[r].plan_mixed() > 0
        out, errs = [None, None], [None, None]

        def worker(r):
            try:
                mode = ems[r].comm_mode()
                ems[r].iterate(2)
                ctxs[r].sync()
                out[r] = mode
            except Exception as e:                           # a rank that fails alone must not leave its peer in the collective
                errs[r] = e
                for x in comms:
                    x.abort()

        th = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th)
        for x in ems + sets:
            x.close()
        live = bm.device_blocks_live()
        for x in comms + ctxs:
            x.close()
        assert errs == [None, None], [str(e) for e in errs]
        assert out[0][0] == out[1][0] and out[0][0] in (1, 2)  # whatever the vote gave: this test is about the count
        print("two ranks, %s: comm mode %d %s" % (which, out[0][0], out[0][1]))
        assert live == start

    _twice(cycle)


def test_one_set_serving_two_orders(ctx, packed):
    """Two exception tables and two record tables on one set; destroyed in the order handle, handle, set."""
    pk = packed["first"]

    def cycle(start):
        ss = bm.SeqSet(ctx, pk)
        ems = [_em(ctx, ss, pk, K, 12) for K in (0, 2)]
        for em in ems:
            assert em.plan()[0] > 0                          # grouped: the set built records for this order
            em.iterate(2)
        ctx.sync()
        ems[0].close(); ems[1].close()
        assert bm.device_blocks_live() > start               # the set's own arrays and tables
        ss.close()
    _twice(cycle)


def _four_records():
    """Single-strand records of 1, 16, 17 and 8193 bases (one beyond the length classes), one N in the 17-base record."""
    off = np.concatenate([[0], np.cumsum([1, 16, 17, 8193])]).astype(np.uint64)
    codes = np.random.RandomState(31).randint(1, 5, size=int(off[-1])).astype(np.uint8)
    codes[int(off[2]) + 5] = 0
    return codes, off


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("stride", [0, 2])
def test_sample_negatives_returns_its_temporaries(stride, resident, ctx):
    """bamm_sample_negatives (csrc/negs.cpp) with a long positive cut into segments of 16 positions.  The positives are made
    and closed inside the cycle: their order-2 exception table, built by the first sampling call, is theirs to keep."""
    codes, off = _four_records()
    ctx.set_tuning(neg_segment_positions=16)
    try:
        def cycle(start):
            pos = bm.SeqSet(ctx, bm.PackedSeqs.from_codes(codes, off, True, seed=42))
            before = bm.device_blocks_live()
            neg, res = bm.sample_negatives(ctx, pos, 2, 2, False, stride, resident=resident)
            assert neg.n_seqs == (4 if stride else 8)
            if resident:
                assert bm.device_blocks_live() > before
                res.close()
            pos.close()
        _twice(cycle)
    finally:
        ctx.set_tuning(neg_segment_positions=0)


def test_sample_negatives_declines_without_a_block(ctx):
    """s_order = 1: the library's "unsupported" code (the CLI samples on the host on exactly that), nothing left behind."""
    codes, off = _four_records()
    pos = bm.SeqSet(ctx, bm.PackedSeqs.from_codes(codes, off, True, seed=42))

    def cycle(start):
        with pytest.raises(abi.BammError) as err:
            bm.sample_negatives(ctx, pos, 1, 2, False, 0)
        assert err.value.code == abi.ERR_UNSUPPORTED
    _twice(cycle)
    pos.close()


def test_pooled_blocks_return_to_the_context(ctx, packed):
    """20 000 sequences through mixed rows: 512 bytes of lane records each, beyond the pool's 4 MB threshold.  After the
    handle the block waits in the context (which is still open here) and is nobody's."""
    pk = packed["large"]
    assert pk.n_seqs * 512 > 4 << 20

    def mixed(em):
        assert em.plan_mixed() == pk.n_seqs
    _twice(_one_handle(ctx, pk, 2, 20, lambda em: em.iterate(2), mixed, tuning=dict(group_layout=8)))
