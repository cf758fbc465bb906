"""The input side of tests/test_fused_classes_gpu.py, pinned without a GPU (tests/fused_classes.py builds the sets), so that a
failure there is a kernel's or the planner's and not the test's.

1. Every record's position count lies in the class its case names: by its length for uniform rows and for end-anchored mixed
   rows, by its span L - W + 3 + 3 (4 - B) for start-anchored mixed rows (where the length lies in the class above, all of
   a set's in the same one), with the shortest and the longest value the class admits at both ends.
2. The record counts: 4 T / 64 + 1 for the block size T of the class, T as csrc/mclass.h lists it and as grp_max_threads
   (csrc/grouped.hip) returns it -- the two agree on every class that carries the fused prologue.
3. The single-N record of a single-strand set: one N, at least K + G + 2 positions from both ends for the widest group
   (G = 4), and between 1 and K + 2 exceptions, counted from PackedSeqs.arrays() as the device's list is built (none at K = 0,
   where no k-mer reaches back to the N); every other record of such a set has none.  A set on both strands has no N but the
   junction's, in the middle of the record, with at most K exceptions.
4. The cases cover what they are there for: every class of 2..16 positions per lane, both block sizes, both group sizes at
   K = 2 and K = 1, the three layouts, mixed rows at 4..10 in both A and both flavours (10 end-anchored only).
5. The fp32 restatement of the reference against fp64 on every case's seed model, in the measure of the GPU test's bars
   (`gate ...` lines): a record, and the check of any regimes.PAIR_BARS entry listed for a case (twice its figure).
"""
import numpy as np
import pytest

import bammmotif2_amd as bm
from tests import em_classes, fused_classes as fc, margins, regimes

NAMES = [s.name for s in fc.SPECS]


def test_block_sizes_are_the_headers():
    table = dict(em_classes.mclass_table())
    grp = fc.grp_max_threads_source()
    for M in fc.FUSED_CLASSES:
        assert fc.threads_for(M) == table[M] == grp(M), M
    assert fc.FUSED_CLASSES == [2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16]
    assert [fc.n_records(M) for M in (8, 10)] == [65, 49]
    assert grp(20) == 512 and table[20] == 768               # from 20 positions per lane on the two differ: no fused class


def test_cases_cover_what_they_name():
    uni = [s for s in fc.SPECS if not s.mixed and s.fusable]
    assert {s.M for s in uni if (s.K, s.W, s.ss, s.tune) == (2, 20, False, ())} == set(fc.FUSED_CLASSES)
    assert {s.M for s in uni if s.K == 2 and s.tuning.get("group_size") == 2} == {4, 8, 12}
    assert {s.M for s in uni if (s.K, s.W) == (2, 31)} == {4, 8, 12}
    assert {(s.M, s.ss) for s in uni if (s.K, s.W, s.tune) == (1, 14, ())} == {(3, False), (7, False), (10, False), (16, False), (5, True), (14, True)}
    assert any(s.K == 1 and s.tuning.get("group_size") == 3 for s in uni)
    assert {(s.M, s.ss) for s in uni if s.K == 0} == {(6, True), (8, False), (12, True)}
    for K, W, ss in ((2, 20, False), (1, 12, True)):
        assert {(s.tuning["group_layout"], s.M) for s in uni if (s.K, s.W, s.ss) == (K, W, ss) and "group_layout" in s.tuning} == \
            {(l, M) for l in (0, 2, 3) for M in (7, 10)}
    for A in (1, 2):
        mixed = {(s.M, s.anchored) for s in fc.SPECS if s.mixed and fc.mix_groups(s.W)[0] == A}
        assert mixed == {(M, a) for M in fc.MIXED_CLASSES for a in (True, False)} - {(10, True)}
    assert all(s.tuning["group_layout"] == 8 and s.tuning["mix_anchor"] == int(s.anchored) for s in fc.SPECS if s.mixed)
    assert {s.W for s in fc.SPECS if s.name.startswith("width_")} == {32, 33, 1, 3}
    assert [s.name for s in fc.SPECS if not s.fusable] == ["width_w33_m7"]
    stops = [s for s in fc.SPECS if s.stop]
    assert len(stops) == 3 and sorted((s.mixed, fc.threads_for(s.M)) for s in stops) == [(False, 768), (False, 1024), (True, 1024)]
    assert all(s.K <= 2 and 4 ** (s.K + 1) * s.W <= 2048 for s in fc.SPECS if s.fusable)


@pytest.mark.parametrize("name", NAMES)
def test_records_are_in_the_class_claimed(name, orc, lib):
    spec = fc.SPEC_BY_NAME[name]
    fs = fc.case_set(orc, name)
    K, W, M, prev = spec.K, spec.W, spec.M, em_classes.prev_class(spec.M)
    pk = bm.PackedSeqs.from_kmers(fs.kmer, fs.off)
    arr = pk.arrays()
    lens = arr["len"].astype(np.int64)
    assert np.array_equal(lens, fs.lens) and np.array_equal(lens, [len(r) if spec.ss else 2 * len(r) + 1 for r in fs.records])
    assert fs.N == fc.n_records(M) == 4 * fc.threads_for(M) // 64 + 1 and fs.N <= 65 and lens.max() <= 1024
    assert (lens >= W).all()
    if spec.mixed:
        anchor = bool(spec.tuning["mix_anchor"])
        assert anchor == spec.anchored
        runs = {fc.run_class(int(L), W, anchor) for L in lens}
        assert runs == {M}, runs
        own = {fc.class_of(int(L)) for L in lens}
        spans = np.array([fc.mix_span(int(L), W) for L in lens])
        if spec.anchored:                                    # one bucket, the class above; the span at both ends of the class's reach
            assert own == {em_classes.M_CLASSES[em_classes.M_CLASSES.index(M) + 1]}
            c = int(lens.max()) - 64 * M                     # L - span
            assert spans.max() == 64 * M and spans.min() == 64 * M + 1 - c and lens.min() == 64 * M + 1 and 64 * prev < spans.min()
            assert fc.run_class(int(lens.max()) + 2, W, True) != M               # the next odd length leaves the class
        else:
            assert own == {M} and lens.min() == 64 * prev + 1 and lens.max() == 64 * M - 1
    else:
        assert ((64 * prev < lens) & (lens <= 64 * M)).all()
        want = [64 * prev + 1, 64 * M, 64 * M - 1] if spec.ss else [64 * prev + 1, 64 * M - 1]
        assert list(lens[:len(want)]) == want
    # the exceptions, from the packed set
    exc = em_classes.exception_counts(arr, K)
    assert np.array_equal(exc, em_classes.kmer_exception_counts(fs.kmer, fs.off, K))
    n_at = [np.flatnonzero(r == 0) for r in fs.records]
    if spec.ss:
        (single,) = [i for i, k in enumerate(fs.kinds) if k == "single"]
        assert single == fs.single and [len(a) for a in n_at] == [int(i == single) for i in range(fs.N)]
        p, L = int(n_at[single][0]), int(lens[single])
        assert min(p, L - 1 - p) >= K + 4 + 2                # K + G + 2 at the widest group; a single strand has no junction
        assert p + 8 + 4 <= L - W + 1                        # ... and clear of the rows for the LW1 edge at any B <= 8, G <= 4 (plan.cpp: capable)
        # (K = 0: the N is its random base and no k-mer reaches back to it, so the record has no exception at all)
        assert (1 if K else 0) <= exc[single] <= (K + 2 if K else 0) and not np.delete(exc, single).any()
    else:
        assert fs.single is None and "single" not in fs.kinds and not any(len(a) for a in n_at)
        assert (exc <= K).all()                              # the junction alone: at most K k-mers reach across it
    print(f"\ngate fused_classes {name}: {fs.N} records of {lens.min()}..{lens.max()} positions, encoder seed {fs.encoder_seed}, "
          f"exceptions {exc.min()}..{exc.max()}" + (f", single N {exc[fs.single]}" if spec.ss else ""))
    pk.free()


@pytest.mark.parametrize("name", sorted(fc.MULTI))
def test_sets_of_several_launches(name, orc, lib):
    fs, cls, mask = fc.multi_set(orc, name)
    d = fc.MULTI[name]
    lens = fs.lens
    for M, count in d["parts"]:
        mine = lens[cls == M]
        assert len(mine) == count and mine.min() == 64 * em_classes.prev_class(M) + 1 and mine.max() == 64 * M - 1
    exc = em_classes.kmer_exception_counts(fs.kmer, fs.off, fs.K)
    if d["scattered"]:
        M, count = d["scattered"]
        assert (cls == 0).sum() == count
        for i in np.flatnonzero(cls == 0):
            assert fc.class_of(int(lens[i])) == M and (fs.records[i] == 0).sum() >= 1
            o = fs.off.astype(np.int64)
            bad = np.flatnonzero(kmer_bad(fs.kmer[o[i]:o[i + 1]], fs.K))
            assert bad.max() - bad.min() + 1 > 8, i          # more group ends than xrec_for_group's range holds: k_em_seq
    else:
        assert not (cls == 0).any()
    assert (exc[cls != 0] <= fs.K).all()
    if d["mask"]:
        assert mask[0] == 0 and mask[-1] == 0 and not mask[::3].any()
        kept = cls[np.flatnonzero(mask)]
        assert all((kept == M).sum() >= 2 for M, _ in d["parts"]) and (kept == 0).sum() >= 1 and (cls[mask == 0] == 0).sum() >= 1
    else:
        assert mask is None
    counts = dict(d["parts"])
    if name == "three_classes":
        assert counts[7] > counts[20] > counts[5]


def kmer_bad(kmer, K):
    km = kmer.astype(np.int64)
    base = km & 3
    bad = np.zeros(len(km), bool)
    for d in range(1, K + 1):
        bad[d:] |= ((km[d:] >> (2 * d)) & 3) != base[:-d]
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_fp32_reference_against_fp64(name, orc):
    """orc.estep / orc.mstep_counts / orc.update_v (the reference's own fp32 evaluation) against fp64 on the seed model."""
    fs = fc.case_set(orc, name)
    inp = fs.inputs()
    ref = regimes.Reference(orc, inp)
    assert np.isfinite(ref.r64).all() and np.isfinite(ref.v64).all() and (ref.Z > 0).all()
    n32 = orc.mstep_counts(inp.kmer, inp.off, inp.K, inp.W, ref.r32)
    v32 = orc.update_v(n32, inp.A, inp.vbg, inp.K, inp.W)
    got = {"r": ref.r32, "llh": ref.llh32, "counts": n32, "v": v32}
    want = {"r": ref.r64, "llh": ref.llh64, "counts": ref.n64, "v": ref.v64}
    base = {"r": (regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL), "llh": (regimes.LLH_RTOL, regimes.llh_atol(inp.N)),
            "counts": (regimes.N_RTOL, regimes.N_ATOL), "v": (regimes.V_RTOL, regimes.V_ATOL)}
    dev = {k: (margins.rel(got[k], want[k], rtol, atol), rtol) for k, (rtol, atol) in base.items()}
    print("\ngate fused_classes %-26s " % name + "  ".join(f"{k} {o:.3e}/{a:.1e}" for k, (o, a) in dev.items()))
    assert all(np.isfinite(o) for o, _ in dev.values())
    for (rg, sp, k), listed in regimes.PAIR_BARS.items():                        # a widened bar is twice what is measured here
        if (rg, sp) == (fc.PAIR, name):
            observed, bar = dev[k]
            assert bar < observed and 2.0 * observed <= listed * 1.001 and listed <= 2.0 * observed * 1.01, (k, observed, listed)
    for k, (rtol, atol) in fc.bars(name, inp).items():
        assert rtol >= base[k][0] and atol >= base[k][1]


def test_builders_are_reproducible(orc):
    name = "k1_w14_m5_ss"
    a = fc.case_set(orc, name)
    fc._SETS.pop(name)
    b = fc.case_set(orc, name)
    assert a is not b and a.kmer.tobytes() == b.kmer.tobytes() and a.off.tobytes() == b.off.tobytes() and a.vbg.tobytes() == b.vbg.tobytes()
    assert a.v0.tobytes() == b.v0.tobytes() and a.encoder_seed == b.encoder_seed
