"""bamm_fdr (csrc/fdr.hip, csrc/fdr_stats.cpp): FDR::calculatePR's MOPS branch and FDR::calculatePvalues (FDR.cpp:156-196,
:278-333) on the device -- both score lists sorted there, the ranking walk as a parallel merge, rows and p-values computed
for the range a call names -- against the host restatement (host/fdr.cpp through bh_fdr_mops_rows), which
tests/test_eval_cpu.py pins to the reference's files.  Both evaluate csrc/fdr_rows.h: every output must be the same bits
(a NaN must be a NaN in the same place: its payload is the hardware's)."""
import ctypes as C
import os

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import build, synth
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

SPT, SPB = None, None                                       # the kernels' granularities, read from the library (geometry())


@pytest.fixture(scope="module")
def host():
    build.build_host()
    h = C.CDLL(build.HOST_LIB)
    h.bh_last_error.restype = C.c_char_p
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))


def host_rows(host, pos, neg, posN, negN):
    pos, neg = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(neg, np.float32)
    n = len(pos) + len(neg)
    cols = {k: np.zeros(max(n, 1), np.float32) for k in ("tp", "fp", "fdr", "rec")}
    p = np.zeros(max(len(pos), 1), np.float32)
    n_rows, occ = C.c_uint64(), C.c_float()
    rc = host.bh_fdr_mops_rows(ptr(pos), C.c_uint64(len(pos)), ptr(neg), C.c_uint64(len(neg)), C.c_uint64(posN), C.c_uint64(negN),
                               C.byref(n_rows), C.byref(occ), ptr(cols["tp"]), ptr(cols["fp"]), ptr(cols["fdr"]), ptr(cols["rec"]), ptr(p))
    assert rc == 0
    out = {k: v[:n_rows.value] for k, v in cols.items()}
    out.update(n_rows=n_rows.value, occ_mult=np.float32(occ.value), p=p[:len(pos)])
    return out


def device_handle(ctx, pos, neg, posN, negN, pieces=1):
    """The scores through add_scores (in `pieces` calls per list: the buffers grow), statistics run."""
    f = bm.FdrMops(ctx)
    for negative, a in ((False, pos), (True, neg)):
        a = np.ascontiguousarray(a, np.float32)
        cuts = [len(a) * k // pieces for k in range(pieces + 1)]
        for b, e in zip(cuts[:-1], cuts[1:]):
            f.add_scores(negative, a[b:e])
    f.statistics(posN, negN, True)
    return f


def check(ctx, host, pos, neg, posN, negN, pieces=1, tail=None):
    """Every output of the device against the host's; rows fetched whole and again in three uneven pieces (tail: only the
    last `tail` rows and p-values are fetched)."""
    hp = host_rows(host, pos, neg, posN, negN)
    f = device_handle(ctx, pos, neg, posN, negN, pieces)
    try:
        info = f.info()
        assert info["n_pos"] == len(pos) and info["n_neg"] == len(neg)
        assert info["n_rows"] == hp["n_rows"], (info["n_rows"], hp["n_rows"])
        assert same_bits([info["occ_mult"]], [hp["occ_mult"]]), (info["occ_mult"], hp["occ_mult"])
        n = info["n_rows"]
        first = 0 if tail is None else max(0, n - tail)
        whole = f.rows(first, n)
        for k in ("tp", "fp", "fdr", "rec"):
            assert same_bits(whole[k], hp[k][first:]), (k, len(pos), len(neg))
        a, b = first + (n - first) // 3 + (1 if n - first > 3 else 0), n - min(5, (n - first) // 2)
        parts = [f.rows(first, a), f.rows(a, b), f.rows(b, n)]
        for k in ("tp", "fp", "fdr", "rec"):
            assert same_bits(np.concatenate([q[k] for q in parts]), whole[k]), k
        only = f.rows(first, n, columns=("rec",))                    # the other columns NULL
        assert list(only) == ["rec"] and same_bits(only["rec"], whole["rec"])
        pfirst = 0 if tail is None else max(0, len(pos) - tail)
        p = f.pvalues(pfirst, len(pos))
        assert same_bits(p, hp["p"][pfirst:]), (len(pos), len(neg))
        m = pfirst + (len(pos) - pfirst) // 4
        assert same_bits(np.concatenate([f.pvalues(pfirst, m), f.pvalues(m, len(pos))]), p)
    finally:
        f.close()
    return hp


# ------------------------------------------------------------------ the reference's own scores
def test_reference_scores(gpu_ctx, host):
    g = dict(np.load(os.path.join(gu.GOLDEN_DIR, "eval_small.npz")))
    hp = check(gpu_ctx, host, g["fdr_pos_all"], g["fdr_neg_all"], 120, 240)
    assert hp["n_rows"] > 0 and len(hp["p"]) == len(g["fdr_pos_all"])


# ------------------------------------------------------------------ device == host, length by length
def synthetic(n_pos, n_neg, seed, shift=1.0):
    rs = np.random.RandomState(seed)
    return (rs.normal(shift, 1.0, n_pos)).astype(np.float32), rs.normal(0.0, 1.0, n_neg).astype(np.float32)


def lengths():
    global SPT, SPB
    SPT, SPB = bm.fdr_geometry()
    out = [(1, 1), (0, 70), (70, 0), (63, 64), (64, 65), (65, 63), (64, 0), (0, 65)]
    for g in (SPT, SPB):                                    # the walk's steps: n_pos + n_neg one below, at and above a granule
        for d in (-1, 0, 1):
            out.append(((g + d) // 3, (g + d) - (g + d) // 3))
            out.append((g + d, g + 1 - d))                   # and each list itself around it
    out.append((2 * SPB + 1, 3 * SPB - 1))
    return out


def test_device_equals_host_across_granularities(gpu_ctx, host):
    for n_pos, n_neg in lengths():
        pos, neg = synthetic(n_pos, n_neg, 7 + n_pos)
        # sequence counts as the CLI passes them: windows / 11, never zero; idx_max starts there, not at the window count
        check(gpu_ctx, host, pos, neg, max(1, n_pos // 11), max(1, n_neg // 11), pieces=2)
        check(gpu_ctx, host, pos, neg, n_pos + 1, n_neg + 3)                    # idx_max's initial value beyond the walk: every row


def test_device_equals_host_many_blocks(gpu_ctx, host):
    """3 M + 5 M scores: some 2 000 blocks, so that the scan of the block maxima runs two of them per thread."""
    pos, neg = synthetic(3_000_017, 5_000_003, 99)
    hp = check(gpu_ctx, host, pos, neg, 3_000_017 // 181, 5_000_003 // 181, pieces=3)
    assert hp["n_rows"] > 4 * SPB                           # the peak lies millions of steps in (the positives sit one sigma higher)
    assert (3_000_017 + 5_000_003) // SPB > 1024


# ------------------------------------------------------------------ regimes
def test_long_ties(gpu_ctx, host):
    pos, neg = synthetic(5000, 9000, 3)
    q = lambda a: (np.round(a * 2) / 2).clip(-1.5, 2.0).astype(np.float32)     # eight values
    assert len(np.unique(np.concatenate([q(pos), q(neg)]))) == 8
    check(gpu_ctx, host, q(pos), q(neg), 5000, 9000)
    check(gpu_ctx, host, q(pos), q(neg), 50, 90)


def test_all_scores_equal(gpu_ctx, host):
    check(gpu_ctx, host, np.full(700, 1.25, np.float32), np.full(1300, 1.25, np.float32), 700, 1300)


def test_one_list_exhausted_first(gpu_ctx, host):
    pos, neg = synthetic(SPB + 300, 2 * SPB + 77, 5)
    check(gpu_ctx, host, pos + np.float32(100), neg, SPB + 300, 2 * SPB + 77)  # every positive above every negative
    check(gpu_ctx, host, pos - np.float32(100), neg, SPB + 300, 2 * SPB + 77)  # and the reverse


def test_signed_zero_pair(gpu_ctx, host):
    """+0 / -0 compare equal: the tie goes to the negative whichever list holds which zero."""
    for pz, nz in ((0.0, -0.0), (-0.0, 0.0)):
        pos = np.array([1.0, pz, -1.0], np.float32)
        neg = np.array([0.5, nz, -2.0], np.float32)
        hp = check(gpu_ctx, host, pos, neg, 3, 3)
        # taken: P 1, N .5, N 0, P 0, P -1, N -2
        assert hp["n_rows"] == 4 and np.array_equal(hp["tp"], np.array([1, 0, -1, 0], np.float32))


def test_return_to_the_peak(gpu_ctx, host):
    """mFold = 2, order P N N P: tp = 1, 0.5, 0, 1 -- the last step EQUALS the running maximum, idx_max = 3."""
    hp = check(gpu_ctx, host, np.array([4.0, 1.0], np.float32), np.array([3.0, 2.0], np.float32), 1, 2)
    assert hp["n_rows"] == 3 and np.array_equal(hp["tp"], np.array([1.0, 0.5, 0.0], np.float32))


def test_peak_at_the_last_step(gpu_ctx, host):
    """N N P P with mFold = 1: tp = -1, -2, -1, 0 -- the last step returns to the initial maximum 0."""
    hp = check(gpu_ctx, host, np.array([1.0, 0.5], np.float32), np.array([3.0, 2.0], np.float32), 5, 5)
    assert hp["n_rows"] == 3
    # ... and across blocks: every negative first, then the positives climb back to exactly 0 at the very last step
    n = SPB + 5
    hp = check(gpu_ctx, host, np.linspace(-2, -1, n).astype(np.float32), np.linspace(1, 2, n).astype(np.float32), n, n)
    assert hp["n_rows"] == 2 * n - 1


def test_no_positive_score(gpu_ctx, host):
    hp = check(gpu_ctx, host, np.zeros(0, np.float32), synthetic(0, 500, 1)[1], 40, 80)
    assert hp["occ_mult"] == 0 and hp["n_rows"] == 120 and np.all(np.isinf(hp["rec"])) and np.all(hp["rec"] < 0)


def test_mfold_not_representable(gpu_ctx, host):
    pos, neg = synthetic(100 * 23, 515 * 23, 17)
    check(gpu_ctx, host, pos, neg, 103, 517)


def test_beyond_2_pow_24(gpu_ctx, host):
    """2^24 + 5000 positives: (float)ip rounds in the last rows (and ties the running maximum there, which is what makes
    these rows exist).  Only the last 10 000 rows and p-values are fetched."""
    n_pos, n_neg = (1 << 24) + 5000, 1 << 20
    pos, neg = synthetic(n_pos, n_neg, 2024, shift=3.0)
    # mFold = 128, positives three sigma up: tp = ip - in / 128 peaks where 16 * 128 * phi(x - 3) = phi(x), x = -1.04 -- all but
    # some 450 positives (ip > 2^24) and 85 % of the negatives lie above it
    hp = check(gpu_ctx, host, pos, neg, 1000, 128000, tail=10000)
    assert hp["n_rows"] > (1 << 24) + (1 << 19)


# ------------------------------------------------------------------ scores of resident sets
@pytest.mark.parametrize("ss", [False, True], ids=["both_strands", "single_strand"])
def test_resident_sets(ss, gpu_ctx, host):
    """Two folds with their own models over one resident set (complementary masks) plus a negative set through add_set,
    against the same scores downloaded by logodds() and fed through add_scores."""
    W, K, N = 8, 1, 40
    rs = np.random.RandomState(12)
    lens = rs.randint(30, 91, size=N)
    lens[3] = W if ss else 30                                # single strand: a sequence with exactly one window
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes = rs.randint(1, 5, size=int(off[-1])).astype(np.uint8)
    packed = bm.PackedSeqs.from_codes(codes, off, ss, seed=42)
    pos = bm.SeqSet(gpu_ctx, packed)
    ncodes, noff = synth.make_sequences(60, 50, synth.make_pwm(W, 4), 8, 0.0, 0.0, 15)
    neg = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_codes(ncodes, noff, True, seed=42))
    vbg = packed.bg_model(2, np.array([1, 10, 10], np.float32))
    models = [synth.bamm_from_pwm((0.7 * synth.make_pwm(W, s) + 0.075).astype(np.float32), K) for s in (5, 6)]
    masks = [(np.arange(N) % 2 == f).astype(np.uint8) for f in (0, 1)]
    moff = np.concatenate([[0], np.cumsum(pos.lengths.astype(np.int64) - W + 1)])
    assert (pos.lengths.min() == W) == ss
    a, b = bm.FdrMops(gpu_ctx), bm.FdrMops(gpu_ctx)
    try:
        for v, mk in zip(models, masks):
            a.add_set(False, pos, K, W, 2, v, vbg, mask=mk)
            a.add_set(True, neg, K, W, 2, v, vbg)
            pm, _, _ = bm.logodds(gpu_ctx, pos, K, W, 2, v, vbg, mask=mk)
            nm, _, _ = bm.logodds(gpu_ctx, neg, K, W, 2, v, vbg)
            b.add_scores(False, np.concatenate([pm[moff[n]:moff[n + 1]] for n in range(N) if mk[n]]))
            b.add_scores(True, nm)
        a.statistics(N, 120, True)
        b.statistics(N, 120, True)
        ia, ib = a.info(), b.info()
        assert ia["n_pos"] == ib["n_pos"] == int(moff[-1]) and ia["n_neg"] == ib["n_neg"] and ia["n_rows"] == ib["n_rows"]
        assert same_bits([ia["occ_mult"]], [ib["occ_mult"]]) and same_bits([ia["e_tp"]], [ib["e_tp"]])
        ra, rb = a.rows(), b.rows()
        for k in ra:
            assert same_bits(ra[k], rb[k]), k
        assert same_bits(a.pvalues(), b.pvalues())
    finally:
        a.close(); b.close(); pos.close(); neg.close()


# ------------------------------------------------------------------ errors, not crashes
def test_argument_errors(gpu_ctx):
    pwm = synth.make_pwm(8, 3)
    codes, off = synth.make_sequences(20, 30, pwm, 3, 0.5, 0.0, 0)
    packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
    pos = bm.SeqSet(gpu_ctx, packed)
    v, vbg = synth.bamm_from_pwm(pwm, 1), packed.bg_model(2, np.array([1, 10, 10], np.float32))
    f = bm.FdrMops(gpu_ctx)
    try:
        with pytest.raises(bm.abi.BammError, match="no score was added"):
            f.statistics(20, 20)
        with pytest.raises(bm.abi.BammError, match="before bamm_fdr_statistics"):
            f.rows(0, 0)
        with pytest.raises(bm.abi.BammError, match="shorter than the motif"):
            f.add_set(False, pos, 1, 31, 2, synth.bamm_from_pwm(synth.make_pwm(31, 3), 1), vbg)
        other = bm.Context(0)
        try:
            theirs = bm.SeqSet(other, packed)
            with pytest.raises(bm.abi.BammError, match="another context"):
                f.add_set(True, theirs, 1, 8, 2, v, vbg)
            theirs.close()
        finally:
            other.close()
        # the sort's index width: refused from the count alone, before anything is allocated or scored
        lib = gpu_ctx.lib
        f.add_scores(False, np.ones(3, np.float32))
        rc = lib.bamm_fdr_add_scores(f.h, 0, ptr(np.ones(1, np.float32)), C.c_uint64((1 << 32) - 3))
        assert rc != 0 and b"2^32 - 1" in lib.bamm_last_error()
        f.add_set(True, pos, 1, 8, 2, v, vbg)
        f.statistics(20, 20, False)
        info = f.info()
        assert info["n_pos"] == 3 and info["n_neg"] == 20 * 23
        with pytest.raises(bm.abi.BammError, match="no more scores"):
            f.add_scores(True, np.ones(2, np.float32))
        with pytest.raises(bm.abi.BammError, match="no more scores"):
            f.add_set(True, pos, 1, 8, 2, v, vbg)
        with pytest.raises(bm.abi.BammError, match="outside the"):
            f.rows(0, info["n_rows"] + 1)
        with pytest.raises(bm.abi.BammError, match="outside the"):
            f.rows(2, 1)
        with pytest.raises(bm.abi.BammError, match="without with_pvalues"):
            f.pvalues(0, 1)
    finally:
        f.close(); pos.close()
    g = bm.FdrMops(gpu_ctx)
    try:
        g.add_scores(False, np.ones(3, np.float32))
        g.statistics(3, 3, True)
        with pytest.raises(bm.abi.BammError, match="outside the"):
            g.pvalues(0, 4)
        assert len(g.pvalues(0, 3)) == 3
    finally:
        g.close()
