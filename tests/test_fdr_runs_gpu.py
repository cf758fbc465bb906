"""bamm_fdr_seal / bamm_fdr_absorb (csrc/fdr_stats.cpp) and the merge of sorted runs (csrc/fdr.hip: k_fdr_merge): scores
collected on several handles, on one to three contexts, sealed where they lie, absorbed by one handle and merged there must
give what ONE handle reports that was given the concatenation through the path that sorts it whole -- info, every row, every
p-value, the same bits (a NaN must be a NaN in the same place, as in tests/test_fdr_mops_gpu.py)."""
import os

import numpy as np
import pytest

import bammmotif2_amd as bm
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

F32 = np.float32


def same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))


@pytest.fixture(scope="module")
def ctxs(gpu_ctx):
    """Three contexts of device 0, the session's first; every one hands out poisoned scratch blocks."""
    more = [bm.Context(0), bm.Context(0)]
    for c in more:
        c.set_tuning(scratch_poison=1)
    yield [gpu_ctx] + more
    for c in more:
        c.close()


def outputs(f, posN, negN):
    f.statistics(posN, negN, True)
    info = f.info()
    return dict(info=info, rows=f.rows(), p=f.pvalues())


def assert_same(got, want, what):
    for k in ("n_pos", "n_neg", "n_rows"):
        assert got["info"][k] == want["info"][k], (what, k, got["info"][k], want["info"][k])
    for k in ("e_tp", "occ_mult"):
        assert same_bits([got["info"][k]], [want["info"][k]]), (what, k, got["info"][k], want["info"][k])
    for k in ("tp", "fp", "fdr", "rec"):
        assert same_bits(got["rows"][k], want["rows"][k]), (what, k)
    assert same_bits(got["p"], want["p"]), (what, "pvalues")


def expected(ctx, pos_parts, neg_parts, posN, negN):
    """One handle, the concatenation, the existing path: one sort per list, no run, no merge."""
    f = bm.FdrMops(ctx)
    try:
        f.add_scores(False, np.concatenate(pos_parts).astype(F32))
        f.add_scores(True, np.concatenate(neg_parts).astype(F32))
        return outputs(f, posN, negN)
    finally:
        f.close()


def sealed_handle(ctx, pos, neg):
    f = bm.FdrMops(ctx)
    f.add_scores(False, pos)
    f.add_scores(True, neg)
    f.seal()
    return f


def merged(ctxs, n_ctx, pos_parts, neg_parts, posN, negN):
    """Part i on a handle of context i mod n_ctx, sealed there; all absorbed in order by a fresh handle of context 0."""
    parts = [sealed_handle(ctxs[i % n_ctx], p, q) for i, (p, q) in enumerate(zip(pos_parts, neg_parts))]
    owner = bm.FdrMops(ctxs[0])
    try:
        for f in parts:
            owner.absorb(f)
            assert f.info()["n_pos"] == 0 and f.info()["n_neg"] == 0
        return outputs(owner, posN, negN)
    finally:
        owner.close()
        for f in parts:
            f.close()


PLANS = [(2, 1), (3, 2), (5, 3)]                             # (sealed handles, contexts of device 0)


def run_lengths():
    spt, spb = bm.fdr_geometry()
    return [0, 1, spt - 1, spt, spt + 1, spb - 1, spb, spb + 1, 3 * spb + 7]


def draw_lengths(n_handles, shift):
    """Lengths of the positive and the negative run of every handle, walking the set from two different starts: over the
    three plans and the shifts the cases use, every length meets every position."""
    L = run_lengths()
    return ([L[(i + shift) % len(L)] for i in range(n_handles)], [L[(2 * i + shift + 4) % len(L)] for i in range(n_handles)])


def check(ctxs, pos_parts, neg_parts, what, counts=None):
    pos_parts = [np.ascontiguousarray(p, F32) for p in pos_parts]
    neg_parts = [np.ascontiguousarray(q, F32) for q in neg_parts]
    n_pos, n_neg = sum(map(len, pos_parts)), sum(map(len, neg_parts))
    assert n_pos + n_neg > 0
    # sequence counts beyond the window counts: idx_max starts behind the walk, so every step up to the last return to the
    # running maximum is a row
    posN, negN = counts or (n_pos + 1, n_neg + 3)
    want = expected(ctxs[0], pos_parts, neg_parts, posN, negN)
    for n_handles, n_ctx in PLANS:
        if n_handles != len(pos_parts):
            continue
        assert_same(merged(ctxs, n_ctx, pos_parts, neg_parts, posN, negN), want, (what, n_handles, n_ctx))
    return want


def for_every_plan(ctxs, what, make):
    """make(n_handles, rs) -> (pos_parts, neg_parts)"""
    for k, (n_handles, _) in enumerate(PLANS):
        pos_parts, neg_parts = make(n_handles, np.random.RandomState(100 + k))
        check(ctxs, pos_parts, neg_parts, what)


# ------------------------------------------------------------------ run combinations
def test_all_runs_empty_but_one(ctxs):
    spt, spb = bm.fdr_geometry()
    for length in (1, spt + 1, 3 * spb + 7):
        def make(n, rs):
            pos = [np.zeros(0, F32) for _ in range(n)]
            neg = [np.zeros(0, F32) for _ in range(n)]
            pos[n - 1] = rs.normal(1, 1, length)                 # the last handle's positives, the first one's negatives
            neg[0] = rs.normal(0, 1, length + 2)
            return pos, neg
        for_every_plan(ctxs, "empty but one", make)

    def only_negatives(n, rs):
        return [np.zeros(0, F32) for _ in range(n)], [np.zeros(0, F32)] * (n - 1) + [rs.normal(0, 1, spb + 1)]
    for_every_plan(ctxs, "no positive at all", only_negatives)


def test_one_element_per_run(ctxs):
    for_every_plan(ctxs, "one element per run", lambda n, rs: ([rs.normal(1, 1, 1) for _ in range(n)], [rs.normal(0, 1, 1) for _ in range(n)]))


def test_every_run_ends_inside_the_same_block(ctxs):
    """Every run's largest score is among the list's last few: all runs are exhausted inside the last block of the merge."""
    def make(n, rs):
        lp, ln = draw_lengths(n, 2)
        def runs(lengths, base):
            out = []
            for i, m in enumerate(lengths):
                a = rs.uniform(0, 1, m).astype(F32)
                if m:
                    a[rs.randint(m)] = base + i / 16.0
                out.append(a)
            return out
        return runs(lp, 5.0), runs(ln, 4.0)
    for_every_plan(ctxs, "same block", make)


def test_disjoint_value_ranges(ctxs):
    """Run i lies wholly above (then: below) run i - 1: one run of every pair is exhausted before the other starts."""
    for sign in (1.0, -1.0):
        def make(n, rs):
            lp, ln = draw_lengths(n, 5)
            return ([sign * 10 * i + rs.uniform(0, 1, m) for i, m in enumerate(lp)], [sign * 10 * i + 3 + rs.uniform(0, 1, m) for i, m in enumerate(ln)])
        for_every_plan(ctxs, "disjoint %+d" % sign, make)


def deal(lengths, start):
    """The integers start, start + 1, ... dealt one at a time to the runs that still have room."""
    runs, k = [[] for _ in lengths], start
    while any(len(r) < m for r, m in zip(runs, lengths)):
        for r, m in zip(runs, lengths):
            if len(r) < m:
                r.append(k)
                k += 1
    return [np.array(r, F32) for r in runs]


def test_fully_interleaved(ctxs):
    def make(n, rs):
        lp, ln = draw_lengths(n, 7)
        return deal(lp, 0), deal(ln, 3)
    for_every_plan(ctxs, "interleaved", make)


def test_every_score_equal(ctxs):
    def make(n, rs):
        lp, ln = draw_lengths(n, 1)
        return [np.full(m, 1.25, F32) for m in lp], [np.full(m, 1.25, F32) for m in ln]
    for_every_plan(ctxs, "all equal", make)


def test_signed_zeros_over_the_runs(ctxs):
    def make(n, rs):
        lp, ln = draw_lengths(n, 3)
        pick = lambda m: rs.choice(np.array([-0.0, 0.0, 0.0, -0.0, -1.0, 1.0], F32), m)
        pos, neg = [pick(m) for m in lp], [pick(m) for m in ln]
        assert any(np.signbit(a[a == 0]).any() for a in pos + neg) and any((~np.signbit(a[a == 0])).any() for a in pos + neg)
        return pos, neg
    for_every_plan(ctxs, "signed zeros", make)


def test_values_that_differ_only_beyond_2_pow_24(ctxs):
    """Neighbouring floats at 2^24 (integers two apart) and their negatives: the keys differ in their lowest bits only."""
    def make(n, rs):
        lp, ln = draw_lengths(n, 6)
        pick = lambda m: ((2.0 ** 24 + 2.0 * rs.randint(0, 40, m)) * rs.choice([-1.0, 1.0], m)).astype(F32)
        pos, neg = [pick(m) for m in lp], [pick(m) for m in ln]
        allv = np.concatenate(pos + neg)
        assert np.all(np.abs(allv) >= 2.0 ** 24) and len(np.unique(allv)) > 40
        return pos, neg
    for_every_plan(ctxs, "beyond 2^24", make)


def test_sequence_counts_of_the_cli(ctxs):
    """idx_max starting inside the walk (sequence counts a tenth of the window counts), five runs of every length class."""
    rs = np.random.RandomState(11)
    lp, ln = draw_lengths(5, 0)
    pos, neg = [rs.normal(1, 1, m) for m in lp], [rs.normal(0, 1, m) for m in ln]
    want = check(ctxs, pos, neg, "cli counts", counts=(max(1, sum(lp) // 11), max(1, sum(ln) // 11)))
    assert 0 < want["info"]["n_rows"] < sum(lp) + sum(ln)


# ------------------------------------------------------------------ mixed and nested absorbs
def test_one_unsealed_and_two_sealed_sources(ctxs):
    spt, spb = bm.fdr_geometry()
    rs = np.random.RandomState(21)
    lens = [spb + 1, spt - 1, 3 * spb + 7, spb - 1]             # the owner's own open scores, the unsealed source, two sealed ones
    pos = [rs.normal(1, 1, m).astype(F32) for m in lens]
    neg = [rs.normal(0, 1, m + 5).astype(F32) for m in lens]
    n_pos, n_neg = sum(map(len, pos)), sum(map(len, neg))
    want = expected(ctxs[0], pos, neg, n_pos + 1, n_neg + 3)
    for order in ((1, 2, 3), (2, 1, 3), (2, 3, 1)):             # the open scores in front of, between and behind the runs
        owner = bm.FdrMops(ctxs[0])
        owner.add_scores(False, pos[0]); owner.add_scores(True, neg[0])
        src = {1: bm.FdrMops(ctxs[1]), 2: sealed_handle(ctxs[2], pos[2], neg[2]), 3: sealed_handle(ctxs[0], pos[3], neg[3])}
        src[1].add_scores(False, pos[1]); src[1].add_scores(True, neg[1])
        try:
            for k in order:
                owner.absorb(src[k])
            assert_same(outputs(owner, n_pos + 1, n_neg + 3), want, ("mixed", order))
        finally:
            owner.close()
            for f in src.values():
                f.close()


@pytest.mark.parametrize("seal_the_middle", [False, True], ids=["open_middle", "sealed_middle"])
def test_a_handle_that_absorbed_is_absorbed(seal_the_middle, ctxs):
    spt, spb = bm.fdr_geometry()
    rs = np.random.RandomState(31)
    lens = [spb, spt + 1, 1, 3 * spb + 7, spt]
    pos = [rs.normal(1, 1, m).astype(F32) for m in lens]
    neg = [rs.normal(0, 1, 2 * m + 1).astype(F32) for m in lens]
    n_pos, n_neg = sum(map(len, pos)), sum(map(len, neg))
    want = expected(ctxs[0], pos, neg, n_pos + 1, n_neg + 3)
    hs = [sealed_handle(ctxs[1], pos[0], neg[0]), bm.FdrMops(ctxs[2]), sealed_handle(ctxs[2], pos[2], neg[2]),
          sealed_handle(ctxs[0], pos[3], neg[3])]
    hs[1].add_scores(False, pos[1]); hs[1].add_scores(True, neg[1])
    middle, owner = bm.FdrMops(ctxs[1]), bm.FdrMops(ctxs[0])
    try:
        middle.add_scores(False, pos[4]); middle.add_scores(True, neg[4])
        middle.absorb(hs[0]); middle.absorb(hs[1]); middle.absorb(hs[2])
        assert middle.info()["n_pos"] == sum(lens) - lens[3]
        if seal_the_middle:                                      # sorts what is open and merges the runs it took over
            middle.seal()
            middle.seal()                                        # a second call is a no-op
        owner.absorb(hs[3])
        owner.absorb(middle)
        assert middle.info()["n_pos"] == 0
        assert_same(outputs(owner, n_pos + 1, n_neg + 3), want, "nested")
    finally:
        for f in hs + [middle, owner]:
            f.close()


def test_a_sealed_handle_runs_statistics_itself(ctxs):
    rs = np.random.RandomState(41)
    pos, neg = rs.normal(1, 1, 5000).astype(F32), rs.normal(0, 1, 9000).astype(F32)
    want = expected(ctxs[0], [pos], [neg], 500, 900)
    f = sealed_handle(ctxs[1], pos, neg)
    try:
        assert_same(outputs(f, 500, 900), want, "sealed, then statistics")
    finally:
        f.close()


# ------------------------------------------------------------------ errors leave both handles as they were
def test_errors(ctxs):
    E = bm.abi.BammError
    ones = np.ones(3, F32)
    a, b, c, d = (bm.FdrMops(ctxs[i % 2]) for i in range(4))
    try:
        for f in (a, b, c, d):
            f.add_scores(False, ones); f.add_scores(True, ones[:2])
        before = [f.info() for f in (a, b, c, d)]
        unchanged = lambda: [f.info() for f in (a, b, c, d)] == before
        with pytest.raises(E, match="cannot absorb itself"):
            a.absorb(a)
        assert unchanged()
        b.seal()
        with pytest.raises(E, match="sealed"):
            b.absorb(a)                                          # a sealed destination
        with pytest.raises(E, match="no more scores"):
            b.add_scores(False, ones)                            # scores after seal
        with pytest.raises(E, match="no more scores"):
            b.add_scores(True, ones)
        assert unchanged()
        c.statistics(3, 2, True)
        before = [f.info() for f in (a, b, c, d)]
        with pytest.raises(E, match="destination is past bamm_fdr_statistics"):
            c.absorb(a)
        with pytest.raises(E, match="source is past bamm_fdr_statistics"):
            a.absorb(c)
        with pytest.raises(E, match="past bamm_fdr_statistics"):
            c.seal()
        assert unchanged()
        a.absorb(b)                                              # what the refusals left behind still works
        assert a.info()["n_pos"] == 6 and a.info()["n_neg"] == 4 and b.info()["n_pos"] == 0
        before = [f.info() for f in (a, b, c, d)]
        for call in (lambda: a.absorb(b), lambda: b.absorb(d), b.seal):
            with pytest.raises(E, match="can only be destroyed"):
                call()                                           # an absorbed handle is neither source nor destination again
        with pytest.raises(E, match="can only be destroyed"):
            b.add_scores(False, ones)
        with pytest.raises(E, match="can only be destroyed"):
            b.statistics(3, 2)
        assert unchanged()
        a.statistics(6, 4, True)
        assert a.info()["n_rows"] > 0 and len(a.pvalues()) == 6
    finally:
        for f in (a, b, c, d):
            f.close()


# ------------------------------------------------------------------ the reference's own scores
def test_reference_scores_in_five_strided_parts(ctxs):
    g = dict(np.load(os.path.join(gu.GOLDEN_DIR, "eval_small.npz")))
    pos, neg = g["fdr_pos_all"].astype(F32), g["fdr_neg_all"].astype(F32)
    want = expected(ctxs[0], [pos], [neg], 120, 240)
    assert want["info"]["n_rows"] > 0
    got = merged(ctxs, 3, [pos[k::5] for k in range(5)], [neg[k::5] for k in range(5)], 120, 240)
    assert_same(got, want, "eval_small in five parts")
