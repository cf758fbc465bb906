"""bamm_occurrences (csrc/occ.hip, csrc/occurrences.cpp): ScoreSeqSet::calcPvalues and the cut of ScoreSeqSet::write on the
device -- the negatives' scores sorted there, every positive window ranked there, only candidates on the host -- against
the reference's own vectors (tests/golden/eval_small.npz, ScoreSeqSet.cpp:70-126,245-291) and against the host path
(bamm_logodds + host/fdr.cpp::mops_pvalues, pinned to the reference by tests/test_eval_cpu.py).  p and e must be the
same bits: the device decides only which windows the host's own formula gets to see."""
import ctypes as C
import os

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import build, synth
from tests import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    build.build_host()
    h = C.CDLL(build.HOST_LIB)
    h.bh_last_error.restype = C.c_char_p
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_path(host, ctx, pos, neg, K, W, bg_order, v, vbg):
    """Every window's p and e the way the CLI's --hostPvalues path computes them, FPl and the scalars restated in numpy."""
    pm, _, _ = bm.logodds(ctx, pos, K, W, bg_order, v, vbg)
    nm, _, _ = bm.logodds(ctx, neg, K, W, bg_order, v, vbg)
    pm, nm = np.ascontiguousarray(pm), np.ascontiguousarray(nm)
    p, e = np.zeros(len(pm), np.float32), np.zeros(len(pm), np.float32)
    assert host.bh_mops_pvalues(ptr(pm), C.c_uint64(len(pm)), ptr(nm), C.c_uint64(len(nm)), C.c_uint64(pos.n_seqs), ptr(p), ptr(e)) == 0
    ns = np.sort(nm)
    fp = (len(ns) - np.searchsorted(ns, pm, side="right")).astype(np.uint64)
    n_top = min(100, len(ns) // 10)
    lam = np.float32(0)
    for x in ns[:n_top]:                                      # sequential fp32 sum (ScoreSeqSet.cpp:89-93)
        lam = np.float32(lam + np.float32(x - ns[n_top]))
    with np.errstate(all="ignore"):
        lam = np.float32(lam / np.float32(n_top))
    moff = np.concatenate([[0], np.cumsum(pos.lengths.astype(np.int64) - W + 1)])
    return dict(p=p, e=e, fp=fp, pm=pm, ns=ns, n_top=n_top, s_ntop=ns[n_top], lam=lam, moff=moff)


def check_against(hp, occ, cutoff, fp_floor=0):
    """The device's hit list against the host path's windows with p < cutoff (those with FPl >= fp_floor)."""
    want = np.flatnonzero((hp["p"] < np.float32(cutoff)) & (hp["fp"] >= fp_floor))
    window = hp["moff"][occ.seq.astype(np.int64)] + occ.pos.astype(np.int64)
    keep = occ.fp >= fp_floor
    assert np.array_equal(window[keep], want), (len(window), len(want))
    assert np.array_equal(occ.fp[keep], hp["fp"][want])
    assert np.array_equal(occ.score[keep].view(np.uint32), hp["pm"][want].view(np.uint32))
    assert np.array_equal(occ.p[keep].view(np.uint32), hp["p"][want].view(np.uint32))
    assert np.array_equal(occ.e[keep].view(np.uint32), hp["e"][want].view(np.uint32))
    assert occ.n_neg_scores == len(hp["ns"]) and occ.n_top == hp["n_top"]
    assert np.float32(occ.s_ntop).view(np.uint32) == np.float32(hp["s_ntop"]).view(np.uint32)
    assert np.float32(occ.lambda_).view(np.uint32) == np.float32(hp["lam"]).view(np.uint32)
    assert occ.n_candidates >= occ.n_hits
    assert np.all(np.diff(window) > 0)                        # ascending (sequence, i)


# ------------------------------------------------------------------ the reference's own vectors
def test_reference_occurrences(gpu_ctx, host, tmp_path):
    g = dict(np.load(os.path.join(gu.GOLDEN_DIR, "eval_small.npz")))
    K, W = int(g["K"]), int(g["W"])
    pos = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_codes(g["codes"], g["in_off"], False, seed=42))
    # SeqGenerator's negatives are single strands as long as the positives' stored sequences (2 * 50 + 1 bases, no N)
    neg = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_codes(g["neg_codes"], g["neg_off"], True, seed=None))
    nm, _, _ = bm.logodds(gpu_ctx, neg, K, W, 2, g["occ_v"], g["vbg"])
    assert np.array_equal(nm, g["occ_neg_mops"])
    pv = g["occ_pvalues"]
    assert len(pv) == 11280
    moff = np.concatenate([[0], np.cumsum(pos.lengths.astype(np.int64) - W + 1)])
    codes, off = np.ascontiguousarray(g["codes"], np.uint8), np.ascontiguousarray(g["in_off"], np.uint64)
    for cutoff, n_want in ((0.02, 274), (1e-4, 0), (0.5, 5530)):
        occ = bm.occurrences(gpu_ctx, pos, neg, K, W, 2, g["occ_v"], g["vbg"], cutoff)
        want = np.flatnonzero(pv < np.float32(cutoff))
        assert len(want) == n_want
        window = moff[occ.seq.astype(np.int64)] + occ.pos.astype(np.int64)
        assert np.array_equal(window, want)
        assert np.array_equal(occ.p, pv[want])
        assert np.array_equal(occ.e, pv[want] * np.float32(120))
        assert np.array_equal(occ.score, g["occ_pos_mops"][want])
        assert occ.n_neg_scores == 22560 and occ.n_top == 100
        # S_ntop and lambda as ScoreSeqSet.cpp:85-93 computes them from the reference's own scores (sequential fp32 sum)
        ns = np.sort(g["occ_neg_mops"])
        lam = np.float32(0)
        for x in ns[:100]:
            lam = np.float32(lam + np.float32(x - ns[100]))
        lam = np.float32(lam / np.float32(100))
        assert np.float32(occ.s_ntop) == ns[100] == np.float32(-11.000789)
        assert np.float32(occ.lambda_) == lam and abs(float(lam) + 0.7554123) < 1e-6
        assert occ.n_candidates >= n_want + 20               # the 20 windows with FPl < 10 go to the host, which drops them (p ~ 2e7)
        assert host.bh_occurrence_hits(str(tmp_path).encode(), b"d", ptr(codes), ptr(off), C.c_uint64(120), 0, W, C.c_uint64(occ.n_hits),
                                       ptr(occ.seq), ptr(occ.pos), ptr(occ.p), ptr(occ.e)) == 0, host.bh_last_error()
        mine = open(tmp_path / "d.occurrence", "rb").read()
        if cutoff == 0.02:
            assert mine == g["occ_file"].tobytes()
        if cutoff == 1e-4:
            assert occ.n_hits == 0 and mine == b"seq\tlength\tstrand\tstart..end\tpattern\tp-value\te-value\n"
        ev = (pv * np.float32(120)).astype(np.float32)
        assert host.bh_occurrence(str(tmp_path).encode(), b"w", ptr(codes), ptr(off), C.c_uint64(120), 0, W, ptr(np.ascontiguousarray(pv)),
                                  ptr(ev), C.c_float(cutoff)) == 0
        assert mine == open(tmp_path / "w.occurrence", "rb").read()
    pos.close(); neg.close()


# ------------------------------------------------------------------ device path == host path, shape by shape
SHAPES = [
    dict(name="k0_w6_ties", N=400, L0=40, W=6, K=0, m=2, big=False),
    dict(name="k2_w20_2000_m1", N=2000, L0=200, W=20, K=2, m=1, big=False),
    dict(name="k2_w20_2000_m3", N=2000, L0=200, W=20, K=2, m=3, big=False),
    dict(name="k2_w20_50000_m1", N=50000, L0=200, W=20, K=2, m=1, big=True),
    dict(name="k2_w20_50000_m3", N=50000, L0=200, W=20, K=2, m=3, big=True),
    dict(name="single_strand", N=500, L0=100, W=12, K=2, m=2, ss=True, big=False),
    dict(name="n_rich", N=300, L0=80, W=10, K=1, m=2, n_frac=0.10, ragged=20, big=False),
    dict(name="beyond_8192_positions", N=6, L0=4200, W=16, K=2, m=2, ragged=150, own_negatives=True, big=False),
    dict(name="table_beyond_lds", N=120, L0=80, W=8, K=6, m=2, big=False),
    dict(name="few_negatives", N=8, L0=50, W=8, K=1, m=1, ss=True, big=False),
    dict(name="planted_strong_motif", N=2000, L0=100, W=10, K=1, m=1, plant_frac=1.0, sharp=8, exact_model=True, big=False),
]


def make_shape(ctx, s):
    W, K = s["W"], s["K"]
    pwm = synth.make_pwm(W, 5, sharp=s.get("sharp", 3))
    codes, off = synth.make_sequences(s["N"], s["L0"], pwm, 23, s.get("plant_frac", 0.5), s.get("n_frac", 0.0), s.get("ragged", 0))
    packed = bm.PackedSeqs.from_codes(codes, off, s.get("ss", False), seed=42)
    pos = bm.SeqSet(ctx, packed)
    if s.get("own_negatives"):                                # the device sampler takes positives up to 8 192 positions
        ncodes, noff = synth.make_sequences(s["N"] * s["m"], s["L0"], pwm, 77, 0.0, 0.0, s.get("ragged", 0))
        neg = bm.SeqSet(ctx, bm.PackedSeqs.from_codes(ncodes, noff, True, seed=42))
    else:
        _, neg = bm.sample_negatives(ctx, pos, 2, s["m"])
    vbg = packed.bg_model(2, np.array([1, 10, 10], np.float32))
    model = pwm if s.get("exact_model") else (0.7 * pwm + 0.3 * 0.25).astype(np.float32)
    return pos, neg, synth.bamm_from_pwm(model, K), vbg


@pytest.mark.parametrize("s", SHAPES, ids=[s["name"] for s in SHAPES])
def test_device_equals_host(s, gpu_ctx, host):
    pos, neg, v, vbg = make_shape(gpu_ctx, s)
    hp = host_path(host, gpu_ctx, pos, neg, s["K"], s["W"], 2, v, vbg)
    if s["name"] == "few_negatives":
        assert len(hp["ns"]) < 1000 and hp["n_top"] < 100
    if s["name"] == "beyond_8192_positions":
        assert pos.lengths.max() > 8192
    if s["name"] == "planted_strong_motif":
        assert int((hp["fp"] < 10).sum()) > 40               # the consensus alone is planted some 80 times (product of the column maxima x N)
    if s["name"] == "k0_w6_ties":
        assert len(np.unique(hp["ns"])) < len(hp["ns"]) // 4
    for cutoff in (1e-4, 1e-2) + (() if s["big"] else (1.5,)):   # 1.5: every window with p <= 1 is a hit, the list outgrows its first size
        occ = bm.occurrences(gpu_ctx, pos, neg, s["K"], s["W"], 2, v, vbg, cutoff)
        check_against(hp, occ, cutoff)
    pos.close(); neg.close()


# ------------------------------------------------------------------ the sort on awkward keys
def test_sorted_negatives_adversarial(gpu_ctx, host):
    """k = 0 with uniform columns next to sharp ones and exact zeros in the model: scores on both sides of zero over many
    binades, thousands of exact ties.  Every rank (fp), S_ntop and lambda come from the sorted array."""
    W, K = 6, 0
    cols = np.array([[0.25, 0.25, 0.25, 0.25], [0.97, 0.01, 0.01, 0.01], [0.0, 0.5, 0.5, 0.0], [0.25, 0.25, 0.25, 0.25],
                     [0.001, 0.001, 0.997, 0.001], [0.4, 0.1, 0.1, 0.4]], np.float32).T.copy()
    codes, off = synth.make_sequences(3000, 60, synth.make_pwm(W, 9), 31, 0.3, 0.01, 20)
    packed = bm.PackedSeqs.from_codes(codes, off, False, seed=42)
    pos = bm.SeqSet(gpu_ctx, packed)
    _, neg = bm.sample_negatives(gpu_ctx, pos, 2, 3)
    v = synth.bamm_from_pwm(cols, K)
    vbg = packed.bg_model(2, np.array([1, 10, 10], np.float32))
    hp = host_path(host, gpu_ctx, pos, neg, K, W, 2, v, vbg)
    ns = hp["ns"]
    assert ns.min() < -8 and ns.max() > 1 and len(np.unique(ns)) < len(ns) // 20
    assert len(np.unique(np.frexp(np.abs(ns[ns != 0]))[1])) >= 5           # binades
    # so few distinct scores that the lowest nTop + 1 negatives tie (lambda = 0): windows above every negative (FPl = 0) are
    # then the corner the reference leaves undefined (test_flat_low_tail_corner) and stay out of the comparison
    floor = 1 if abs(float(hp["lam"])) <= 1e-5 else 0
    for cutoff in (1e-4, 1e-2, 1.5):
        check_against(hp, bm.occurrences(gpu_ctx, pos, neg, K, W, 2, v, vbg, cutoff), cutoff, fp_floor=floor)
    pos.close(); neg.close()


# ------------------------------------------------------------------ the corner the reference leaves undefined
def test_flat_low_tail_corner(gpu_ctx, host):
    """FPl = 0 with |lambda| <= 1e-5 reads one past the sorted negatives in the reference (ScoreSeqSet.cpp:120); the device
    path takes +infinity there (include/bamm_em.h).  A model with one informative column over a flat background: three
    distinct scores, the lowest shared by a quarter of the negatives (lambda = 0), the highest by every window with FPl = 0.
    The call returns, and both paths agree on every window with FPl > 0."""
    W, K = 5, 0
    cols = np.full((4, W), 0.25, np.float32)
    cols[:, 2] = [0.25, 0.25, 0.4, 0.1]
    codes, off = synth.make_sequences(500, 50, synth.make_pwm(W, 9), 41, 0.0, 0.0, 0)
    packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
    pos = bm.SeqSet(gpu_ctx, packed)
    _, neg = bm.sample_negatives(gpu_ctx, pos, 2, 2)
    v = synth.bamm_from_pwm(cols, K)
    vbg = np.full(bm.bg_size(2), 0.25, np.float32)
    hp = host_path(host, gpu_ctx, pos, neg, K, W, 2, v, vbg)
    assert len(np.unique(hp["ns"])) == 3 and hp["lam"] == 0 and int((hp["fp"] == 0).sum()) > 100
    occ = bm.occurrences(gpu_ctx, pos, neg, K, W, 2, v, vbg, 1.5)
    assert int((occ.fp == 0).sum()) == int((hp["fp"] == 0).sum()) and np.all(occ.p[occ.fp == 0] == 0)
    check_against(hp, occ, 1.5, fp_floor=1)
    pos.close(); neg.close()


# ------------------------------------------------------------------ errors, not crashes
def test_argument_errors(gpu_ctx):
    pwm = synth.make_pwm(8, 3)
    codes, off = synth.make_sequences(20, 30, pwm, 3, 0.5, 0.0, 0)
    packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
    pos = bm.SeqSet(gpu_ctx, packed)
    empty = bm.SeqSet(gpu_ctx, bm.PackedSeqs.from_kmers(np.zeros(0, np.uint64), np.zeros(1, np.uint64)))
    v, vbg = synth.bamm_from_pwm(pwm, 1), packed.bg_model(2, np.array([1, 10, 10], np.float32))
    with pytest.raises(bm.abi.BammError, match="negative set is empty"):
        bm.occurrences(gpu_ctx, pos, empty, 1, 8, 2, v, vbg, 1e-4)
    with pytest.raises(bm.abi.BammError, match="shorter than the motif"):
        bm.occurrences(gpu_ctx, pos, pos, 1, 31, 2, synth.bamm_from_pwm(synth.make_pwm(31, 3), 1), vbg, 1e-4)
    other = bm.Context(0)
    try:
        theirs = bm.SeqSet(other, packed)
        with pytest.raises(bm.abi.BammError, match="another context"):
            bm.occurrences(gpu_ctx, pos, theirs, 1, 8, 2, v, vbg, 1e-4)
        theirs.close()
    finally:
        other.close()
    occ = bm.occurrences(gpu_ctx, empty, pos, 1, 8, 2, v, vbg, 1e-4)      # no positives: an empty list, the scalars still there
    assert occ.n_hits == 0 and occ.n_neg_scores == 20 * 23
    pos.close(); empty.close()
