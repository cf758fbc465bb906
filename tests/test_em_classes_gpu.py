"""k_em_seq, k_e_slice, k_m_slice and k_m_list (csrc/kernels.hip) in every one of their 23 positions-per-lane classes.

tests/em_classes.py builds one record set per class -- the class's shortest and longest record, 64 M - 1 and a length that
is a multiple of neither 4 nor M, with N at the record's ends, around the first lane's last position and in a run across
the lane boundary in the middle of the wave; a record without exceptions, one with fewer than the six that travel with a
prefetched record, one with more; enough records for every wave of a one-block launch to walk three -- and two models, a
blurred one (every window adds: the dense walks, lists beyond the prefetched batches) and a sharp one (a handful of windows
add: the sparse M-step, one-batch lists).  tests/test_em_classes_cpu.py pins all of that without a GPU.

Flavour P is K = 2, W = 20 under grouped=0: every record through k_em_seq.  Flavour S is K = 4, W = 30: the sliced path in
the six tunings of test_parity_gpu.py::test_sliced_paths_agree_bit_for_bit.  Flavour L is K = 4, W = 20 in the classes of 40
positions per lane and more, where flavour S cannot reach k_m_list.  r, llh, counts and v are held to fp64
(regimes.estep_f64, orc.em_step_f64) at tests/regimes.py's bars; what adds the same integers is held bit for bit.  The
observed margins land in the session's parity-margin table (profiles/em_classes_margins.txt).

Three deliberate mistakes were tried against this file, one at a time (HISTORY.md has the details).  decode_raw without its
tail loop over the exceptions beyond the first six: all 46 cases of P and S fail at r against fp64.  k_em_seq's sparse walk
without its last batch: P1..P16 fail at the counts -- the twelve classes that have a sparse M-step -- and nothing else.
k_m_list ignoring list entries from index 256 on: S5..S32 fail at the counts under the blurred model; S40..S128 did not,
which is how flavour L came to be.
"""
import numpy as np
import pytest

import bammmotif2_amd as bm
from tests import em_classes, margins
from tests.em_classes import M_CLASSES, MODELS

pytestmark = pytest.mark.gpu

SLICED_TUNINGS = (("list", dict(adaptive_lists=0)), ("adaptive", {}), ("never_lists", dict(list_threshold_pct=0)),
                  ("lists_from_pass_2", dict(list_threshold_pct=100)), ("dense", dict(e_list=0)), ("e_sliced", dict(e_fused=0)))
SLICED_DEFAULTS = dict(e_list=1, e_fused=1, adaptive_lists=1, list_threshold_pct=45)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    bad = np.flatnonzero(a != b)
    assert a.shape == b.shape and bad.size == 0, f"{what}: {bad.size} of {a.size} words differ, first at {bad[:8]}"


class Handles:
    """The handles and resident sets a test opened, closed whatever happens."""

    def __init__(self, ctx):
        self.ctx, self.open, self.ems = ctx, [], []

    def seqs(self, kmer, off):
        ss = bm.SeqSet(self.ctx, bm.PackedSeqs.from_kmers(kmer, off))
        self.open.append(ss)
        return ss

    def em(self, ss, inp, tuning, blocks=0, **kw):
        """An EM handle created under `tuning` (and a launch of `blocks` blocks); the context is back at its defaults afterwards."""
        self.ctx.set_tuning(**tuning)
        self.ctx.set_launch(blocks, 0)
        try:
            em = bm.EM(self.ctx, ss, inp.K, inp.W, inp.vbg, inp.A, inp.v, inp.q, bg_order=inp.bg_order, **kw)
        finally:
            restore(self.ctx)
        self.ems.append(em)
        return em

    def close_ems(self):
        for em in self.ems:
            em.close()
        self.ems = []

    def close(self):
        self.close_ems()
        for ss in self.open:
            ss.close()
        self.open = []


def restore(ctx):
    ctx.set_tuning(grouped=1, sparse=1, **SLICED_DEFAULTS)
    ctx.set_launch(0, 0)


def check_against_fp64(name, flavour, model, tag, inp, want, r=None, llh=None, counts=None, v=None):
    """Each given quantity against fp64 at the pair's bars, through margins.check."""
    bars = em_classes.bars(flavour, model, inp)
    for k, got in (("r", r), ("llh", llh), ("counts", counts), ("v", v)):
        if got is not None:
            margins.check(name, tag, k, got, want[k], *bars[k], against="fp64")


def fp64_of(ref):
    return {"r": ref.r64, "llh": ref.llh64, "counts": ref.n64, "v": ref.v64}


@pytest.mark.parametrize("M", M_CLASSES)
def test_per_column_kernel_in_every_class(M, gpu_ctx, orc):
    cs = em_classes.class_set(orc, "P", M)
    hs = Handles(gpu_ctx)
    try:
        ss = hs.seqs(cs.kmer, cs.off)
        mask = em_classes.fold_mask(cs.N)
        keep = np.flatnonzero(mask)
        sub = hs.seqs(*em_classes.subset(cs.kmer, cs.off, keep))
        for model in MODELS:
            inp, ref = em_classes.case(orc, "P", model, M)
            name, want = f"{cs.name} {model}", fp64_of(ref)
            per_column = dict(grouped=0, sparse=1)

            step = hs.em(ss, inp, per_column)                                    # EStep, getR, MStep one after the other
            grouped, other, _ = step.plan()
            sliced, _, long_seqs = step.plan_paths()
            assert grouped == 0 and other == cs.N and not sliced and long_seqs == 0, (grouped, other, sliced, long_seqs)
            step.EStep()
            r, llh = step.getR(), step.getLLH()
            check_against_fp64(name, "P", model, "k_em_seq E", inp, want, r=r, llh=llh)
            if model == "blurred":                                               # zero in the last W - 1 slots and nowhere else
                assert np.array_equal(r == 0, ref.r32 == 0)
            b, e = cs.N // 3, cs.N - cs.N // 3                                   # a middle range of getR is a slice of the whole
            off = inp.off.astype(np.int64)
            same_bits(step.getR(b, e), r[off[b]:off[e]], f"{name}: getR({b}, {e})")
            step.MStep()
            counts = step.getCounts()
            check_against_fp64(name, "P", model, "k_em_seq E, M", inp, want, counts=counts)

            one = hs.em(ss, inp, per_column)                                     # the fused pass
            one.iterate(1)
            check_against_fp64(name, "P", model, "k_em_seq pass", inp, want, llh=one.trace()[0][-1], counts=one.getCounts(), v=one.getV())

            dense = hs.em(ss, inp, dict(grouped=0, sparse=0))                    # the sparse M-step adds the dense one's integers
            assert dense.plan()[:2] == (0, cs.N)
            dense.iterate(1)
            same_bits(dense.getCounts(), one.getCounts(), f"{name}: counts, sparse=0 against sparse=1")
            same_bits(dense.getV(), one.getV(), f"{name}: v, sparse=0 against sparse=1")
            same_bits(dense.trace()[0], one.trace()[0], f"{name}: llh, sparse=0 against sparse=1")

            single = hs.em(ss, inp, per_column, blocks=1)                        # one block: every wave walks three records or more
            single.EStep()
            same_bits(single.getR(), r, f"{name}: r, blocks=1 against the default launch")
            single.MStep()
            same_bits(single.getCounts(), counts, f"{name}: counts, blocks=1 against the default launch")

            fold = hs.em(ss, inp, per_column, mask=mask)                         # a fold's mask against the kept records alone
            alone = hs.em(sub, inp, per_column)
            assert fold.plan()[0] == 0 and alone.plan()[:2] == (0, len(keep))
            fold.iterate(1); alone.iterate(1)
            same_bits(fold.getCounts(), alone.getCounts(), f"{name}: counts, mask against subset")
            sub_inp = cs.inputs(model, keep)
            v64, n64, llh64, _ = orc.em_step_f64(sub_inp.kmer, sub_inp.off, sub_inp.K, sub_inp.W, sub_inp.bg_order, sub_inp.vbg, sub_inp.A,
                                                 sub_inp.v, sub_inp.q)
            check_against_fp64(name, "P", model, "k_em_seq mask", sub_inp, {"llh": llh64, "counts": n64, "v": v64},
                               llh=fold.trace()[0][-1], counts=fold.getCounts(), v=fold.getV())
            hs.close_ems()
    finally:
        restore(gpu_ctx)
        hs.close()


@pytest.mark.parametrize("M", M_CLASSES)
def test_sliced_kernels_in_every_class(M, gpu_ctx, orc):
    cs = em_classes.class_set(orc, "S", M)
    hs = Handles(gpu_ctx)
    try:
        ss = hs.seqs(cs.kmer, cs.off)
        for model in MODELS:
            inp, ref = em_classes.case(orc, "S", model, M)
            name, want = f"{cs.name} {model}", fp64_of(ref)
            tunings = dict(SLICED_TUNINGS)

            # one step of a fresh handle: k_em_seq<WRITE_R> with lists and k_m_list; dense r and k_m_slice
            for tag in ("list", "dense"):
                em = hs.em(ss, inp, tunings[tag])
                sliced, e_fused, long_seqs = em.plan_paths()
                assert sliced and e_fused and long_seqs == 0 and em.plan()[0] == 0, (tag, sliced, e_fused, long_seqs, em.plan())
                em.iterate(1)
                r = em.getR()
                check_against_fp64(name, "S", model, f"sliced {tag}", inp, want, r=r, llh=em.trace()[0][-1], counts=em.getCounts(), v=em.getV())
                if model == "blurred":
                    assert np.array_equal(r == 0, ref.r32 == 0)

            res = {}
            for tag, tune in SLICED_TUNINGS:
                em = hs.em(ss, inp, tune, optimizeQ=True)
                sliced, e_fused, long_seqs = em.plan_paths()
                assert sliced and long_seqs == 0 and e_fused == (tag != "e_sliced"), (tag, sliced, e_fused, long_seqs)
                em.iterate(3)
                res[tag] = (em.getCounts(), em.getV(), np.float32(em.getQ()), em.trace()[0], em.getR())
            for tag in ("dense", "adaptive", "never_lists", "lists_from_pass_2"):
                for k, what in enumerate(("counts", "v", "q", "llh trace", "r")):
                    same_bits(res[tag][k], res["list"][k], f"{name}: {what} after three passes, {tag} against list")
            np.testing.assert_allclose(res["list"][1], res["e_sliced"][1], rtol=2e-6, atol=1e-10)
            np.testing.assert_allclose(res["list"][4], res["e_sliced"][4], rtol=1e-5, atol=1e-12)

            for tag in ("list", "dense"):                                        # one block: every wave walks three records or more
                em = hs.em(ss, inp, tunings[tag], blocks=1, optimizeQ=True)
                em.iterate(3)
                got = (em.getCounts(), em.getV(), np.float32(em.getQ()), em.trace()[0], em.getR())
                for k, what in enumerate(("counts", "v", "q", "llh trace", "r")):
                    same_bits(got[k], res[tag][k], f"{name}: {what} after three passes, {tag} at blocks=1 against the default launch")
            hs.close_ems()
    finally:
        restore(gpu_ctx)
        hs.close()


@pytest.mark.parametrize("M", em_classes.classes_of("L"))
def test_list_walk_in_the_long_classes(M, gpu_ctx, orc):
    """From 40 positions per lane on, flavour S never reaches k_m_list: beside a slice of 15 columns a block's copies of the
    decoded records do not fit, and the planner walks dense r under every tuning (tests/em_classes.py: FLAVOURS).  K = 4,
    W = 20 cuts the table into slices of 10 columns, where they fit in every class: the `list` tuning against fp64, against
    the dense walk and at one block."""
    cs = em_classes.class_set(orc, "L", M)
    hs = Handles(gpu_ctx)
    tunings = dict(SLICED_TUNINGS)
    try:
        ss = hs.seqs(cs.kmer, cs.off)
        for model in MODELS:
            inp, ref = em_classes.case(orc, "L", model, M)
            name, want = f"{cs.name} {model}", fp64_of(ref)
            em = hs.em(ss, inp, tunings["list"])
            sliced, e_fused, long_seqs = em.plan_paths()
            assert sliced and e_fused and long_seqs == 0 and em.plan()[0] == 0, (sliced, e_fused, long_seqs, em.plan())
            em.iterate(1)
            r = em.getR()
            check_against_fp64(name, "L", model, "sliced list", inp, want, r=r, llh=em.trace()[0][-1], counts=em.getCounts(), v=em.getV())
            if model == "blurred":
                assert np.array_equal(r == 0, ref.r32 == 0)
            res = {}
            for tag, blocks in (("list", 0), ("dense", 0), ("list", 1)):
                em = hs.em(ss, inp, tunings[tag], blocks=blocks, optimizeQ=True)
                em.iterate(3)
                res[tag, blocks] = (em.getCounts(), em.getV(), np.float32(em.getQ()), em.trace()[0], em.getR())
            for k, what in enumerate(("counts", "v", "q", "llh trace", "r")):
                same_bits(res["dense", 0][k], res["list", 0][k], f"{name}: {what} after three passes, dense against list")
                same_bits(res["list", 1][k], res["list", 0][k], f"{name}: {what} after three passes, list at blocks=1 against the default launch")
            hs.close_ems()
    finally:
        restore(gpu_ctx)
        hs.close()
