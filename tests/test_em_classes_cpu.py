"""The input side of tests/test_em_classes_gpu.py, pinned without a GPU, so that a failure there is a kernel's and not the
test's (tests/em_classes.py builds the records and the models).

1. Every record is in the class it was built for (64 prev < L <= 64 M), the four edge lengths are there, every class holds
   enough records for a wave to walk three, and the exception counts -- from PackedSeqs.arrays(), as the device's list is
   built -- are what the builder intended: none, one to six, more than six.
2. The conditions on the two models, in fp64 through regimes.estep_f64 (a window is non-zero when r * 2^40 >= 1):
     sharp    every record has fewer than 64 non-zero windows (a list is one batch), and in the classes of 4..16 positions
              per lane, where the sparse M-step's list holds 192, between 1 and 96;
     blurred  every record with more than 256 windows has more than 256 non-zero ones (the dense walk; lists beyond the four
              batches k_m_list prefetches), and r is zero in the last W - 1 slots only, in fp64 and in the fp32 restatement.
3. The fp32 restatement of the reference (orc.estep, orc.mstep_counts, orc.update_v) against fp64 per (flavour, model,
   class), on r, counts, v and llh in the measure of the GPU test's bars (`gate ...` lines, kept in
   profiles/em_classes_margins.txt).  The GPU test holds the kernels to tests/regimes.py's bars whether or not the
   restatement keeps them -- it sums a record's windows and a cell's addends one after the other in fp32, the kernels do
   not --, so the figures are a record; only an entry of regimes.PAIR_BARS widens a bar, and such an entry must be twice
   the figure measured here.
"""
import numpy as np
import pytest

import bammmotif2_amd as bm
from tests import em_classes, margins, regimes
from tests.em_classes import FLAVOURS, M_CLASSES, MODELS

CLASSES = [(f, M) for f in FLAVOURS for M in em_classes.classes_of(f)]
CLASS_IDS = [f"{f}{M}" for f, M in CLASSES]
CASES = [(f, m, M) for f in FLAVOURS for m in MODELS for M in em_classes.classes_of(f)]
CASE_IDS = [f"{f}{M}-{m}" for f, m, M in CASES]


def test_class_table_is_the_headers():
    assert em_classes.mclass_table() == [(M, em_classes.threads_for(M)) for M in M_CLASSES]
    assert len(M_CLASSES) == 23 and all(em_classes.classes_of(f) == list(M_CLASSES) for f in "PS")
    assert em_classes.classes_of("L") == [40, 48, 56, 64, 80, 96, 128]


@pytest.mark.parametrize("flavour,M", CLASSES, ids=CLASS_IDS)
def test_records_are_in_their_class_with_the_exceptions_as_built(flavour, M, orc, lib):
    cs = em_classes.class_set(orc, flavour, M)
    K, W, prev = cs.K, cs.W, cs.prev
    pk = bm.PackedSeqs.from_kmers(cs.kmer, cs.off)
    arr = pk.arrays()
    lens = arr["len"].astype(np.int64)
    assert np.array_equal(lens, [len(r) for r in cs.records]) and np.array_equal(lens, np.diff(cs.off.astype(np.int64)))
    assert ((64 * prev < lens) & (lens <= 64 * M) & (lens >= W)).all()
    edges = lens[:4]
    assert list(edges[:3]) == [max(W, 64 * prev + 1), 64 * M, 64 * M - 1] and edges[3] % 4 != 0 and (M == 1 or edges[3] % M != 0)
    assert cs.N >= 3 * em_classes.threads_for(M) // 64 + 1 and cs.N == em_classes.min_records(M)
    # N where with_n puts them, in every edge record that reaches the place
    run = 32 * M - (K + 2) // 2
    for rec in cs.records[:4]:
        want = [p for p in [0, M - 1, M, len(rec) - 1] + list(range(run, run + K + 2)) if p < len(rec)]
        assert not rec[want].any()
    assert cs.records[cs.clean].all() and (cs.records[cs.single] == 0).sum() == 1 and 0 < int(np.flatnonzero(cs.records[cs.single] == 0)[0]) < lens[cs.single] - 1
    # the three exception counts, from the packed set
    exc = em_classes.exception_counts(arr, K)
    assert np.array_equal(exc, em_classes.kmer_exception_counts(cs.kmer, cs.off, K))
    assert exc[cs.clean] == 0 and 1 <= exc[cs.single] <= em_classes.RAW_EXC and exc[cs.many] > em_classes.RAW_EXC
    assert cs.kinds[cs.many] == "edge" and lens[cs.many] >= 32 * M + K + 2            # it holds the run across the lane boundary
    print(f"\ngate em_classes {cs.name}: {cs.N} records of {lens.min()}..{lens.max()} positions, encoder seed {cs.encoder_seed}, "
          f"exceptions clean {exc[cs.clean]} single {exc[cs.single]} run {exc[cs.many]} most {exc.max()}")
    pk.free()


@pytest.mark.parametrize("flavour,model,M", CASES, ids=CASE_IDS)
def test_model_conditions_hold_in_fp64(flavour, model, M, orc):
    inp, ref = em_classes.case(orc, flavour, model, M)
    assert np.isfinite(ref.r64).all() and np.isfinite(ref.v64).all() and (ref.Z > 0).all()
    np.testing.assert_allclose(ref.llh_np, ref.llh64, rtol=1e-12, atol=1e-11 * inp.N)           # numpy's E step and the oracle's agree
    np.testing.assert_allclose(ref.n_np.astype(np.float32), ref.n64, rtol=1.2e-7, atol=1e-300)
    off = inp.off.astype(np.int64)
    windows = np.diff(off) - inp.W + 1
    nz = em_classes.nonzero_windows(inp, ref.r64)
    print(f"\ngate em_classes {inp.case.name}-{model}: non-zero windows per record {nz.min()}..{nz.max()} of {windows.min()}..{windows.max()}")
    if model == "sharp":
        assert (nz < 64).all()
        if 4 <= M <= 16:
            assert ((1 <= nz) & (nz <= 96)).all()
    else:
        big = windows > em_classes.LIST_PREFETCH
        assert (nz[big] > em_classes.LIST_PREFETCH).all()
        tail = np.zeros(len(ref.r64), bool)
        for n in range(inp.N):
            tail[off[n + 1] - inp.W + 1:off[n + 1]] = True
        assert np.array_equal(ref.r64 == 0, tail) and np.array_equal(ref.r32 == 0, tail)


@pytest.mark.parametrize("flavour,model,M", CASES, ids=CASE_IDS)
def test_fp32_reference_against_fp64(flavour, model, M, orc):
    inp, ref = em_classes.case(orc, flavour, model, M)
    n32 = orc.mstep_counts(inp.kmer, inp.off, inp.K, inp.W, ref.r32)
    v32 = orc.update_v(n32, inp.A, inp.vbg, inp.K, inp.W)
    got = {"r": ref.r32, "llh": ref.llh32, "counts": n32, "v": v32}
    want = {"r": ref.r64, "llh": ref.llh64, "counts": ref.n64, "v": ref.v64}
    base = {"r": (regimes.R_RTOL * regimes.r_len_factor(inp.off), regimes.R_ATOL), "llh": (regimes.LLH_RTOL, regimes.llh_atol(inp.N)),
            "counts": (regimes.N_RTOL, regimes.N_ATOL), "v": (regimes.V_RTOL, regimes.V_ATOL)}
    dev = {k: (margins.rel(got[k], want[k], rtol, atol), rtol) for k, (rtol, atol) in base.items()}
    print("\ngate em_classes %-14s " % f"{inp.case.name}-{model}" + "  ".join(f"{k} {o:.3e}/{a:.1e}" for k, (o, a) in dev.items()))
    assert all(np.isfinite(o) for o, _ in dev.values())
    pair = em_classes.pair_name(flavour, model)
    for (rg, sp, k), listed in regimes.PAIR_BARS.items():                        # a widened bar is twice what is measured here
        if (rg, sp) == (pair, inp.case.name):
            observed, bar = dev[k]
            assert bar < observed and 2.0 * observed <= listed * 1.001 and listed <= 2.0 * observed * 1.01, (k, observed, listed)
    for k, (rtol, atol) in em_classes.bars(flavour, model, inp).items():         # ... and no bar is below the fuzz sweep's
        assert rtol >= base[k][0] and atol >= base[k][1]


def test_builders_are_reproducible(orc):
    a, b = em_classes.ClassSet(orc, "P", 5), em_classes.ClassSet(orc, "P", 5)
    assert a.kmer.tobytes() == b.kmer.tobytes() and a.off.tobytes() == b.off.tobytes() and a.vbg.tobytes() == b.vbg.tobytes()
    assert a.model("sharp")[0].tobytes() == b.model("sharp")[0].tobytes()
    mask = em_classes.fold_mask(a.N)
    assert mask[0] == 0 and mask[-1] == 0 and not mask[::3].any() and mask.sum() >= a.N // 2
