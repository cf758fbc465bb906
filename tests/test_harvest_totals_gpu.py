"""The fix lanes' harvest in k_em_mix (csrc/mixed_kernel.h) after the M-step: a virtual count cell is never cleared, the
lane keeps the total it last saw and takes the difference; the resident bins have a dump cell per column for the code
"no bin".

What can go wrong and is tested here: a running total that is stale or carried to the wrong sequence.  The accumulator
is integers, so it must not depend on which sequences follow each other in a wave: the same set at 1, 2 and 3 blocks
(15, 8 and 5 sequences per wave) gives the same words, over three passes in one handle (the totals start at zero with
the cells in every launch).  W = 20 has two wide groups and none of their columns resident; W = 16 has one and every
column resident, so the fourth add goes to a wide group's bins.  Lengths that alternate from sequence to sequence move the
edge rows -- which lanes are fix lanes, and for which positions -- while the cells' totals carry on.  No layout lost a
resident column to the dump cells (tests/test_harvest_cpu.py), so there is no case for one.

All handles are forced onto the mixed rows (group_layout 8) with a set number of blocks, as in test_lane_records_gpu.py.
v of the third pass is held against the fp64 restatement of that pass (from the model the handle had after two) at the
bars of the mixed-row tests there and in test_grouped_gpu.py: rtol 1e-6, atol 1e-9."""
import ctypes as C

import numpy as np
import pytest

import bammmotif2_amd as bm
from tests.cases import Case
from tests.test_partition_exact_gpu import accumulator

pytestmark = pytest.mark.gpu

N = 240


def alternate(c, L_other):
    """every second sequence of the case cut to L_other bases"""
    lens = np.diff(c.in_off.astype(np.int64))
    keep = np.where(np.arange(c.N) % 2 == 1, L_other, lens)
    parts = [c.codes[int(b):int(b) + int(k)] for b, k in zip(c.in_off[:-1], keep)]
    c.codes = np.concatenate(parts)
    c.in_off = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
    return c


# (id, W, the length of every second sequence where it is not 200)
_SETS = [("W20", 20, None), ("W16", 16, None),
         ("W20_L0_180_200", 20, 180),                        # 6 and 7 positions per lane: a launch each
         ("W20_L0_193_200", 20, 193), ("W16_L0_193_200", 16, 193)]     # both 7 per lane: they alternate within every wave


class Set:
    def __init__(self, orc, W, L_other):
        c = Case(name="harvest", N=N, L0=200, W=W, K=2)
        if L_other:
            alternate(c, L_other)
        self.c = c
        self.seq, self.kmer, self.off, self.vbg = c.encode(orc)
        self.pk = bm.PackedSeqs.from_kmers(self.kmer, self.off)
        self.runs = {}

    def run(self, ctx, hip, blocks):
        """(accumulator words of the third pass, v before it, v after it) with the launches cut into `blocks` blocks"""
        if blocks not in self.runs:
            c = self.c
            ctx.set_tuning(group_layout=8)
            ctx.set_launch(blocks, 0)
            try:
                ss = bm.SeqSet(ctx, self.pk)
                em = bm.EM(ctx, ss, c.K, c.W, self.vbg, c.A, c.v0, c.q, bg_order=c.bg_order)
            finally:
                ctx.set_launch(0, 0)
                ctx.set_tuning(group_layout=-1)
            assert em.plan_mixed() == em.plan()[0] > c.N // 2
            em.iterate(2)
            v2 = em.getV()
            em.accumulate()
            ctx.sync()
            p, n = em.reduce_buffer()
            words = np.zeros(n, np.int64)
            assert hip.hipMemcpy(words.ctypes.data_as(C.c_void_p), C.c_void_p(p), n * 8, 2) == 0
            em.update()
            self.runs[blocks] = (words, v2, em.getV())
            em.close(); ss.close()
        return self.runs[blocks]


@pytest.fixture(scope="module")
def sets(orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Set(orc, *[s[1:] for s in _SETS if s[0] == name][0])
        return made[name]
    return get


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.mark.parametrize("name", [s[0] for s in _SETS])
def test_third_pass_is_the_same_integers_at_one_two_and_three_blocks(name, sets, gpu_ctx, hip):
    s = sets(name)
    cells = 4 ** (s.c.K + 1) * s.c.W
    one = s.run(gpu_ctx, hip, 1)
    assert one[0][cells + 2] == N and one[0][cells] != 0 and np.count_nonzero(one[0][:cells]) > cells // 2
    for blocks in (2, 3):
        other = s.run(gpu_ctx, hip, blocks)
        assert np.array_equal(other[0], one[0]), blocks
        assert np.array_equal(other[1], one[1]) and np.array_equal(other[2], one[2]), blocks


@pytest.mark.parametrize("name", [s[0] for s in _SETS])
def test_third_pass_against_exact_arithmetic(name, sets, gpu_ctx, hip, orc):
    s = sets(name)
    c = s.c
    _, v2, v3 = s.run(gpu_ctx, hip, 2)
    v64, *_ = orc.em_step_f64(s.kmer, s.off, c.K, c.W, c.bg_order, s.vbg, c.A, v2, c.q)
    np.testing.assert_allclose(v3, v64, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("name", ["W20", "W16"])
def test_first_pass_accumulator_at_one_two_and_three_blocks(name, sets, gpu_ctx, hip):
    """tests.test_partition_exact_gpu.accumulator: a fresh handle's first pass, read before any update."""
    s = sets(name)
    c = s.c
    shape = dict(N=c.N, K=c.K, W=c.W, tune=dict(group_layout=8))
    words = [accumulator(gpu_ctx, hip, s.pk, 0, c.N, shape, s.vbg, c.A, c.v0, (blocks, 0)) for blocks in (1, 2, 3)]
    cells = 4 ** (c.K + 1) * c.W
    assert words[0][cells + 2] == c.N and words[0][cells] != 0
    assert np.array_equal(words[1], words[0]) and np.array_equal(words[2], words[0])
