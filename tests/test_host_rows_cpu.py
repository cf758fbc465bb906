"""The host library's row writers and sampler at their edges (host/row_text.h, host/fdr.cpp, host/neg_sampler.h).

.positions, .occurrence and .logOddsZoops share one window row -- header, shown length, strand, start..end, the window's
bases as forward strand + N + reverse complement -- and .mops.stats / .mops.pvalues have one writer, fed whole or in
chunks.  The expected text is restated here in Python (`'%.3g' % float(np.float32(x))` for the numbers), not read from
the code under test."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import build
from tests import golden_util as gu

W = 3
# forward lengths 3 (= W), 4 and 7; a 0 (N) and a 5 (outside the alphabet: N on both strands)
SEQS = [[1, 2, 3], [4, 0, 2, 1], [3, 5, 1, 1, 2, 4, 3]]
VALUES = [0, 1e-5, 0.000123456, 0.5, 0.9995, 12345.678, 1e-40, 3.4e38]
SAMPLER_GOLDEN = os.path.join(gu.GOLDEN_DIR, "host_sampler_edges.npz")
SAMPLER_POSITIVES = [[1, 2, 3], [4, 4, 1], [2, 3, 1, 1, 4, 2, 3, 3], [3, 1, 4, 2, 2]]     # lengths 3, 3, 8, 5
SAMPLER_CASES = list(itertools.product((1, 2, 3), (0, 3), (0, 1)))                         # m_fold, keep_stride, generic


@pytest.fixture(scope="module")
def host(lib):
    build.build_host()
    H = C.CDLL(build.HOST_LIB)
    H.bh_last_error.restype = C.c_char_p
    return H


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def flat(seqs):
    codes = np.array([x for s in seqs for x in s], np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return codes, off


def full_text(seq, revcomp):
    """Sequence::getSequence(): the forward strand, and behind it an N and the reverse complement."""
    fwd = "".join("NACGT"[x] if x <= 4 else "N" for x in seq)
    rev = "".join("NTGCA"[x] if x <= 4 else "N" for x in reversed(seq))
    return fwd + "N" + rev if revcomp else fwd


def fmt3(x):
    return "%.3g" % float(np.float32(x))


def window_row(header, seq, i, revcomp, shown):
    text = full_text(seq, revcomp)
    assert i + W <= len(text)
    return "%s\t%d\t%s\t%d..%d\t%s" % (header, shown, "+" if i < shown else "-", i + 1, i + W, text[i:i + W])


def windows(ss):
    """(sequence, window start) of every window of SEQS."""
    return [(n, i) for n, s in enumerate(SEQS) for i in range((len(s) if ss else 2 * len(s) + 1) - W + 1)]


def values(n):
    return np.array([VALUES[k % len(VALUES)] for k in range(n)], np.float32)


POSITIONS_HEAD = "seq\tlength\tstrand\tstart..end\tpattern\n"
OCCURRENCE_HEAD = "seq\tlength\tstrand\tstart..end\tpattern\tp-value\te-value\n"
ZOOPS_HEAD = "seq\tlength\tstrand\tstart..end\tpattern\tzoops_score\n"


def write_positions(host, d, base, ss, r, cutoff):
    codes, off = flat(SEQS)
    hd = (C.c_char_p * len(SEQS))(*[b">s%d x" % n for n in range(len(SEQS))])
    assert host.bh_positions(str(d).encode(), base, hd, ptr(codes), ptr(off), C.c_uint64(len(SEQS)), ss, W, ptr(r),
                             C.c_float(cutoff)) == 0, host.bh_last_error()
    return open(d / (base.decode() + ".positions")).read()


def write_positions_hits(host, d, base, ss, hits):
    codes, off = flat(SEQS)
    hd = (C.c_char_p * len(SEQS))(*[b">s%d x" % n for n in range(len(SEQS))])
    seq, pos = np.array([h[0] for h in hits], np.uint64), np.array([h[1] for h in hits], np.uint32)
    assert host.bh_positions_hits(str(d).encode(), base, hd, ptr(codes), ptr(off), C.c_uint64(len(SEQS)), ss, W, C.c_uint64(len(hits)),
                                  ptr(seq), ptr(pos)) == 0, host.bh_last_error()
    return open(d / (base.decode() + ".positions")).read()


def write_occurrence(host, d, base, ss, p, e, cutoff):
    codes, off = flat(SEQS)
    assert host.bh_occurrence(str(d).encode(), base, ptr(codes), ptr(off), C.c_uint64(len(SEQS)), ss, W, ptr(p), ptr(e),
                              C.c_float(cutoff)) == 0, host.bh_last_error()
    return open(d / (base.decode() + ".occurrence")).read()


def write_occurrence_hits(host, d, base, ss, hits, p, e):
    codes, off = flat(SEQS)
    seq, pos = np.array([h[0] for h in hits], np.uint64), np.array([h[1] for h in hits], np.uint32)
    assert host.bh_occurrence_hits(str(d).encode(), base, ptr(codes), ptr(off), C.c_uint64(len(SEQS)), ss, W, C.c_uint64(len(hits)),
                                   ptr(seq), ptr(pos), ptr(p), ptr(e)) == 0, host.bh_last_error()
    return open(d / (base.decode() + ".occurrence")).read()


def write_logodds_zoops(host, d, base, seqs, revcomp, ss, z, score):
    codes, off = flat(seqs)
    z = np.array(z, np.uint64)
    assert host.bh_logodds_zoops(str(d).encode(), base, b"seq", 1, ptr(codes), ptr(off), C.c_uint64(len(seqs)), revcomp, ss, W,
                                 ptr(score), ptr(z)) == 0, host.bh_last_error()
    return open(d / (base.decode() + ".logOddsZoops")).read()


def dense_r(ss, keep):
    """EM's r layout: per sequence L floats, window start i at L - W - i; 1 where keep(window number), else 0."""
    r, k = [], 0
    for s in SEQS:
        L = len(s) if ss else 2 * len(s) + 1
        row = np.zeros(L, np.float32)
        for i in range(L - W + 1):
            row[L - W - i] = 1.0 if keep(k) else 0.0
            k += 1
        r.append(row)
    return np.concatenate(r)


@pytest.mark.parametrize("ss", [1, 0])
def test_every_window_through_the_three_writers(ss, host, tmp_path):
    """ss = 0: the last forward window, the windows across the junction N, the first reverse window and the last
    window i = L - W of every sequence; the numbers run through zero, %g's exponent forms, a rounding carry, a
    denormal and the largest floats."""
    win = windows(ss)
    assert len(win) == (8 if ss else 25)
    rev = not ss
    # .positions and .occurrence show the forward length whatever the strands
    want = POSITIONS_HEAD + "".join(window_row(">s%d x" % n, SEQS[n], i, rev, len(SEQS[n])) + "\n" for n, i in win)
    assert write_positions(host, tmp_path, b"all", ss, dense_r(ss, lambda k: True), 0.5) == want
    p, e = values(len(win)), values(len(win) + 3)[3:]
    want = OCCURRENCE_HEAD + "".join(window_row("seq%d" % n, SEQS[n], i, rev, len(SEQS[n])) + "\t%s\t%s\n" % (fmt3(p[k]), fmt3(e[k]))
                                     for k, (n, i) in enumerate(win))
    assert write_occurrence(host, tmp_path, b"all", ss, p, e, np.inf) == want
    # .logOddsZoops has one row per sequence (its best window): every window as the best one of a copy of its sequence
    score = values(len(win) + 5)[5:]
    want = ZOOPS_HEAD + "".join(window_row("seq%d" % k, SEQS[n], i, rev, len(SEQS[n])) + "\t%s\n" % fmt3(score[k])
                                for k, (n, i) in enumerate(win))
    got = write_logodds_zoops(host, tmp_path, b"all", [SEQS[n] for n, _ in win], int(rev), ss, [i for _, i in win], score)
    assert got == want


@pytest.mark.parametrize("ss", [1, 0])
def test_dense_and_list_forms_write_the_same_bytes(ss, host, tmp_path):
    win = windows(ss)
    hits = win[::2]                                             # the cut-off keeps every second window
    dense = write_positions(host, tmp_path, b"dense", ss, dense_r(ss, lambda k: k % 2 == 0), 0.5)
    assert dense.count("\n") == 1 + len(hits)
    assert write_positions_hits(host, tmp_path, b"hits", ss, hits) == dense
    p = np.array([0.01 if k % 2 == 0 else 0.5 for k in range(len(win))], np.float32)
    e = values(len(win))
    dense = write_occurrence(host, tmp_path, b"dense", ss, p, e, 0.1)
    assert dense.count("\n") == 1 + len(hits)
    assert write_occurrence_hits(host, tmp_path, b"hits", ss, hits, np.ascontiguousarray(p[::2]), np.ascontiguousarray(e[::2])) == dense
    # no hit: the header line alone
    none = np.zeros(1, np.float32)
    assert write_positions_hits(host, tmp_path, b"none", ss, []) == POSITIONS_HEAD
    assert write_occurrence_hits(host, tmp_path, b"none", ss, [], none, none) == OCCURRENCE_HEAD


def test_negatives_keep_the_halved_length_column(host, tmp_path):
    """ScoreSeqSet.cpp:293-331 halves the length column whenever --ss is absent, also for the sampled negatives, which
    carry one strand: the column shows (L0 - 1) // 2, the strand sign is taken against that, the pattern is forward."""
    seqs = [SEQS[1], SEQS[1], SEQS[2], SEQS[2], SEQS[2]]
    z = [0, 1, 0, 3, 4]                                         # below, at and above (7 - 1) // 2 = 3; (4 - 1) // 2 = 1
    score = values(len(seqs))
    want = ZOOPS_HEAD
    for k, (s, i) in enumerate(zip(seqs, z)):
        shown = (len(s) - 1) // 2
        want += window_row("seq%d" % k, s, i, False, shown) + "\t%s\n" % fmt3(score[k])
    assert [row.split("\t")[2] for row in want.split("\n")[1:-1]] == ["+", "-", "+", "-", "-"]
    assert write_logodds_zoops(host, tmp_path, b"neg", seqs, 0, 0, z, score) == want


def test_mops_files_whole_and_in_chunks(host, tmp_path):
    """The ranking ties once (3.0: the negative goes first), climbs to a new peak of 4 behind the tie, leaves it and
    returns to it at step 13, for the last time: 13 rows.  Written through the range fetchers at several chunk sizes ==
    written from the result."""
    pos = np.array([9, 8, 7, 5.5, 4.5, 3.5, 3.0, 2.8, 2.4, 0.001], np.float32)
    neg = np.array([6, 5, 4, 3.0, 2.5, 2.0, 0.5, 0.1, 0.05, 0.01], np.float32)
    n = len(pos) + len(neg)
    tp, fp, fdr, rec = (np.zeros(n, np.float32) for _ in range(4))
    p = np.zeros(len(pos), np.float32)
    n_rows, occ = C.c_uint64(), C.c_float()
    assert host.bh_fdr_mops_rows(ptr(pos), C.c_uint64(len(pos)), ptr(neg), C.c_uint64(len(neg)), C.c_uint64(10), C.c_uint64(10),
                                 C.byref(n_rows), C.byref(occ), ptr(tp), ptr(fp), ptr(fdr), ptr(rec), ptr(p)) == 0
    n_rows = n_rows.value
    assert n_rows == 13 and list(tp[:14]) == [1, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 4, 3, 4]
    d = str(tmp_path).encode()
    assert host.bh_fdr_stats(ptr(pos), C.c_uint64(0), ptr(neg), C.c_uint64(0), ptr(pos), C.c_uint64(len(pos)), ptr(neg), C.c_uint64(len(neg)),
                             C.c_uint64(10), C.c_uint64(10), C.c_float(0.3), 1, 0, 1, d, b"whole") == 0, host.bh_last_error()
    stats, pvalues = (open(tmp_path / ("whole.mops." + x), "rb").read() for x in ("stats", "pvalues"))
    assert stats.count(b"\n") == 1 + n_rows and pvalues.count(b"\n") == len(pos)
    for chunk in (1, 5, n_rows, 100):
        base = b"c%d" % chunk
        assert host.bh_fdr_mops_chunked(ptr(tp), ptr(fp), ptr(fdr), ptr(rec), C.c_uint64(n_rows), ptr(p), C.c_uint64(len(p)), occ,
                                        C.c_uint64(chunk), d, base) == 0, host.bh_last_error()
        assert open(tmp_path / (base.decode() + ".mops.stats"), "rb").read() == stats
        assert open(tmp_path / (base.decode() + ".mops.pvalues"), "rb").read() == pvalues
    assert host.bh_fdr_mops_chunked(ptr(tp), ptr(fp), ptr(fdr), ptr(rec), C.c_uint64(0), ptr(p), C.c_uint64(0), occ, C.c_uint64(5), d,
                                    b"empty") == 0, host.bh_last_error()
    assert open(tmp_path / "empty.mops.stats", "rb").read() == stats.split(b"\n")[0] + b"\n"
    assert open(tmp_path / "empty.mops.pvalues", "rb").read() == b""


def sample_edges(host):
    """{case name: codes / offsets of the negatives} of SAMPLER_CASES on SAMPLER_POSITIVES."""
    codes, off = flat(SAMPLER_POSITIVES)
    packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)        # one strand: the lengths as listed
    out = {}
    for m_fold, stride, generic in SAMPLER_CASES:
        n, m = C.c_uint64(), C.c_uint64()
        args = (packed._p, 2, C.c_uint64(m_fold), generic, C.c_uint64(stride), C.byref(n), C.byref(m))
        assert host.bh_sample_negatives_strided(*args, None, None) == 0, host.bh_last_error()
        ncodes, noff = np.zeros(m.value, np.uint8), np.zeros(n.value + 1, np.uint64)
        assert host.bh_sample_negatives_strided(*args, ptr(ncodes), ptr(noff)) == 0
        name = "f%d_k%d_g%d" % (m_fold, stride, generic)
        out[name + "_codes"], out[name + "_off"] = ncodes, noff
    return out


def record_sampler_edges():
    H = C.CDLL(build.HOST_LIB)
    H.bh_last_error.restype = C.c_char_p
    np.savez_compressed(SAMPLER_GOLDEN, **sample_edges(H))


@pytest.mark.parametrize("threads", [1, 3])
def test_sampler_edges_are_pinned(threads, host):
    """One negative per positive (draw_many hands over to draw), two and three (the interleaved loop), all of them or
    every third, sequence-specific and generic tables, on positives of lengths 3, 3, 8 and 5: the arrays recorded from
    the build in front of the commit that folded the two loops' copies into first_bases / next_base, by

        python -c "from tests.test_host_rows_cpu import record_sampler_edges as r; r()"
    """
    g = dict(np.load(SAMPLER_GOLDEN))
    gomp = C.CDLL("libgomp.so.1")                              # bh_set_threads also sets the process's OpenMP thread count,
    before = gomp.omp_get_max_threads()                        # on which the sums of later tests' fp32 oracle depend: left as found
    host.bh_set_threads(threads)
    try:
        got = sample_edges(host)
    finally:
        host.bh_auto_threads()
        gomp.omp_set_num_threads(before)
    assert sorted(got) == sorted(g) and len(g) == 2 * len(SAMPLER_CASES)
    for name in g:
        assert np.array_equal(got[name], g[name]), name
    assert len(g["f3_k0_g0_off"]) == 13 and len(g["f3_k3_g0_off"]) == 5 and len(g["f1_k3_g1_off"]) == 2
    assert list(np.diff(g["f2_k0_g1_off"].astype(np.int64))) == [3, 3, 3, 3, 8, 8, 5, 5]
