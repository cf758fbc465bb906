"""The fused model update (csrc/update_kernel.h in the block prologue of k_em_grp and k_em_mix / k_em_mix1) in every length
class that carries it, and the pass that runs behind it.

tests/test_update_exact_gpu.py and test_optimize_script_gpu.py pin the update as a function of scripted sums; here the sums
are the pass's own, on one record set per (family, class) of tests/fused_classes.py -- the class's shortest and longest
records, enough of them for two blocks whose waves walk two records and one a third -- so that what follows the prologue is
checked too: the count table zeroed over the update's scratch, the grouped odds built from the table the update left in
LDS, the fix lanes reading their block's copy of it, q from the update's return instead of the published one.

Per case, P = 4 passes with optimizeQ (q changes in every pass, so a stale q shows):
  plan     plan_update() == (0, fused), plan() == (N, 0, 1) and the launch's class / mixed / anchored, asserted before anything
           runs: a case whose planner declined to fuse fails here instead of comparing an unfused run with itself
  bits     iterate(P) of a handle created under fused_update = 1 against iterate(P - 1), iterate(1) of one created under 0:
           v, counts, s, q, llh, iteration, r and the llh / q columns of the trace are the same words; v_diff within 3e-7
           (tests/test_fused_update_gpu.py::same_trace: the fp64 block reduction groups by block size)
  fp64     both handles share one binary, so the FUSED handle's r, llh, counts and v of pass P are also held to
           regimes.estep_f64 / orc.em_step_f64 on the twin's (v, q) from before that pass, at tests/regimes.py's bars,
           through margins.check (the observed margins land in the session's parity table; profiles/fused_classes_margins.txt)
  optimize a third handle, fused, with epsilon = 0 and max_iterations = P leaves iterate(P)'s bits (the look-ahead units,
           the `stop` argument, the prologue's old-v read); on three cases both tunings also run to the stop rule
           (epsilon = 0.01): same pass count strictly between 1 and 200, same bits, same r, and the same after iterate(2)

No entry of regimes.PAIR_BARS was needed: every case keeps the bars as they stand (tests/test_fused_classes_cpu.py prints the
reference's own fp32 figures per case).

The width boundaries (plan_fused_update's first line, update_fits_lds: 4^(K+1) W <= 2048): W = 32 is fusable, W = 33 leaves
the LDS form (form 2, not fusable) and is kept as a pin with the bit comparison; W = 1 and W = 3 are fusable.

Two sets of several launches: classes 5, 7 and 20 with six scattered-N records and a fold mask (the class-7 launch, the
largest of the fused classes, is moved to the front and carries the update; the others read the model block 0 published), and
classes 20 and 24 alone (nothing to fuse into: (0, False), equal bits all the same).

Two deliberate mistakes were tried against this file, one at a time, each built, run once and reverted; both make numbers
stale and touch no address.
  grouped_kernel.h, `const float q = fused_now ? q_fused : *a.q` reading `*a.q`: 44 of the 69 ids fail, every one at the
  first comparison (v, fused against unfused: all words differ) -- the 43 fusable uniform-row cases (u_*, g2_*, k1_*, k0_*,
  layout*, width_w32 / w1 / w3) and three_classes; the 23 mix_* cases, width_w33_m7 and classes_20_24 pass.
  mixed_kernel.h, `if (!staged)` in front of the copy of a.s made unconditional (the table the update staged is overwritten
  by the previous model's): the 23 mix_* cases fail, the other 46 ids pass.
Neither passed anywhere it should have failed.
"""
import numpy as np
import pytest

import bammmotif2_amd as bm
from tests import fused_classes as fc, margins, regimes
from tests.test_em_classes_gpu import same_bits

pytestmark = pytest.mark.gpu

P = fc.P
DEFAULTS = dict(fused_update=1, group_size=0, group_layout=-1, mix_anchor=1)


class Handles:
    """The handles and the resident set of one case, closed whatever happens."""

    def __init__(self, ctx, fs, tuning, blocks, mask=None):
        self.ctx, self.fs, self.tuning, self.blocks, self.mask = ctx, fs, tuning, blocks, mask
        self.ems = []
        self.ss = bm.SeqSet(ctx, bm.PackedSeqs.from_kmers(fs.kmer, fs.off))

    def em(self, fused, **kw):
        """A handle created under the case's tuning, `fused_update` and the launch of `blocks` blocks; the context is back at
        its defaults afterwards."""
        fs = self.fs
        try:
            self.ctx.set_tuning(fused_update=int(fused), **self.tuning)
            self.ctx.set_launch(self.blocks, 0)
            em = bm.EM(self.ctx, self.ss, fs.K, fs.W, fs.vbg, fs.A, fs.v0, fs.q0, bg_order=fs.bg_order, optimizeQ=True, mask=self.mask, **kw)
        finally:
            self.ctx.set_tuning(**DEFAULTS)
            self.ctx.set_launch(0, 0)
        self.ems.append(em)
        return em

    def close(self):
        for em in self.ems:
            em.close()
        self.ss.close()


def state(em):
    return dict(v=em.getV(), counts=em.getCounts(), s=em.getS(), q=np.float32(em.getQ()), llh=np.float32(em.getLLH()),
                iteration=em.iteration(), trace=em.trace())


def same_state(a, b, what, keys=("v", "counts", "s", "q", "llh")):
    for k in keys:
        same_bits(a[k], b[k], f"{what}: {k}")
    assert a["iteration"] == b["iteration"], what
    (la, va, qa), (lb, vb, qb) = a["trace"], b["trace"]
    same_bits(la, lb, f"{what}: llh column of the trace")
    same_bits(qa, qb, f"{what}: q column of the trace")
    np.testing.assert_allclose(va, vb, rtol=3e-7, atol=0, err_msg=f"{what}: v_diff column of the trace")


def fused_against_unfused_and_fp64(hs, orc, name, expect_fused, tag, keep=None):
    """The bit comparison of iterate(P), the fp64 anchor of pass P (fused handles) and optimize() at epsilon = 0.  Returns
    (fused handle's state, its r)."""
    fs = hs.fs
    fused, twin = hs.em(True), hs.em(False)
    assert fused.plan_update() == (0, expect_fused) and twin.plan_update() == (0, False)
    assert fused.plan() == twin.plan()
    twin.iterate(P - 1)
    v, q = twin.getV(), twin.getQ()
    twin.iterate(1)
    fused.iterate(P)
    a, b = state(fused), state(twin)
    assert a["iteration"] == P
    same_state(a, b, f"{name}: iterate({P}), fused against unfused")
    r = fused.getR()
    same_bits(r, twin.getR(), f"{name}: r, fused against unfused")
    # pass P against fp64, from the model the twin held before it
    inp = fs.inputs(v, q)
    r64, *_ = regimes.estep_f64(inp)
    sub = inp if keep is None else fs.inputs(v, q, keep)
    v64, n64, llh64, _ = orc.em_step_f64(sub.kmer, sub.off, sub.K, sub.W, sub.bg_order, sub.vbg, sub.A, sub.v, sub.q)
    bars = fc.bars(name, inp)
    margins.check(name, tag, "r", r, r64, *bars["r"], against="fp64")        # every record, masked out or not
    margins.check(name, tag, "llh", a["trace"][0][-1], llh64, bars["llh"][0], regimes.llh_atol(sub.N), against="fp64")
    margins.check(name, tag, "counts", a["counts"], n64, *bars["counts"], against="fp64")
    margins.check(name, tag, "v", a["v"], v64, *bars["v"], against="fp64")
    # optimize() with the rule off: the same passes through the look-ahead units
    opt = hs.em(expect_fused, epsilon=0.0, max_iterations=P)
    assert opt.plan_update() == (0, expect_fused)
    assert opt.optimize() == P
    same_state(state(opt), a, f"{name}: optimize() at epsilon = 0 against iterate({P})")
    same_bits(opt.getR(), r, f"{name}: r, optimize() against iterate({P})")
    return a, r


def stop_rule(hs, name):
    """optimize() to its stop rule under both tunings: the `fired` return of the prologue."""
    outs = []
    for fused in (True, False):
        em = hs.em(fused, epsilon=0.01, max_iterations=200)
        assert em.plan_update() == (0, fused)
        it = em.optimize()
        first = (it, state(em), em.getR())
        em.iterate(2)
        outs.append(first + (state(em),))
    (ia, sa, ra, na), (ib, sb, rb, nb) = outs
    assert ia == ib and 1 < ia < 200 and sa["iteration"] == ia, (ia, ib)
    same_state(sa, sb, f"{name}: optimize() to the stop rule after {ia} passes, fused against unfused")
    same_bits(ra, rb, f"{name}: r after the stop rule")
    same_state(na, nb, f"{name}: iterate(2) after the stop rule")


@pytest.mark.parametrize("name", [s.name for s in fc.SPECS])
def test_fused_pass_in_its_class(name, gpu_ctx, orc):
    spec = fc.SPEC_BY_NAME[name]
    fs = fc.case_set(orc, name)
    hs = Handles(gpu_ctx, fs, spec.tuning, blocks=2)
    try:
        if not spec.fusable:                                 # a pin of the planner's boundary, and the bit comparison
            a, b = hs.em(True), hs.em(False)
            assert a.plan_update() == b.plan_update() == (spec.form, False), spec.why
            assert a.plan() == b.plan() == spec.plan, spec.why
            a.iterate(P); b.iterate(P - 1); b.iterate(1)
            same_state(state(a), state(b), f"{name}: iterate({P}) under fused_update = 1 and 0")
            same_bits(a.getR(), b.getR(), f"{name}: r")
            return
        probe = hs.em(True)
        assert probe.plan_update() == (0, True), spec.why
        assert probe.plan() == (fs.N, 0, 1)
        assert probe.plan_launches() == [dict(count=fs.N, positions_per_lane=spec.M, mixed=spec.mixed, anchored=spec.anchored)]
        assert probe.plan_mixed() == (fs.N if spec.mixed else 0)
        fused_against_unfused_and_fp64(hs, orc, name, True, "k_em_mix fused" if spec.mixed else "k_em_grp fused")
        if spec.stop:
            stop_rule(hs, name)
    finally:
        gpu_ctx.set_tuning(**DEFAULTS)
        gpu_ctx.set_launch(0, 0)
        hs.close()


# plan_launches() of the two sets, as the planner gives them (pinned): the buckets in the order of their classes, a class's
# grouped launch before its k_em_seq one, then plan_fused_update's swap of the largest fused class to the front
def _launch(count, M):
    return dict(count=count, positions_per_lane=M, mixed=False, anchored=False)


MULTI_PLANS = {
    "three_classes": dict(update=(0, True), plan=(60, 6, 4), launches=[_launch(40, 7), _launch(8, 5), _launch(6, 7), _launch(12, 20)]),
    "classes_20_24": dict(update=(0, False), plan=(20, 0, 2), launches=[_launch(10, 20), _launch(10, 24)]),
}


@pytest.mark.parametrize("name", sorted(fc.MULTI))
def test_sets_of_several_launches(name, gpu_ctx, orc):
    fs, cls, mask = fc.multi_set(orc, name)
    want = MULTI_PLANS[name]
    hs = Handles(gpu_ctx, fs, {}, blocks=0, mask=mask)
    try:
        probe, plain = hs.em(True), hs.em(False)
        assert probe.plan_update() == want["update"] and plain.plan_update() == (0, False)
        assert probe.plan() == want["plan"]
        launches = probe.plan_launches()
        assert launches == want["launches"]
        if want["update"][1]:                                # the largest fused class first; class 20 carries no update
            assert launches[0]["positions_per_lane"] == 7 and launches[0]["count"] == max(l["count"] for l in launches)
            assert sorted(map(str, plain.plan_launches())) == sorted(map(str, launches))
        keep = None if mask is None else np.flatnonzero(mask)
        fused_against_unfused_and_fp64(hs, orc, name, want["update"][1], "fused, 4 launches" if want["update"][1] else "classes 20, 24", keep)
    finally:
        gpu_ctx.set_tuning(**DEFAULTS)
        gpu_ctx.set_launch(0, 0)
        hs.close()
