"""bamm_kmer_counts_gapped (csrc/kmer_count.hip, k_kmer_counts_gapped) against the numpy oracle of tests/gapped_ref.py and
against its host twin: exact integers, every comparison is array_equal, all gaps 0 .. 16 - w in one call.  The shapes are the
smallest at which the kernel can go wrong: record lengths around the largest span and around the word and dword edges of
the 2-bit stream (with both strands the separator lands at every phase of a word, and inside a gap), unknown bases at those
edges and in pairs around the spans, records beyond BAMM_MAX_SEQ_POSITIONS cut into segments down to a single word (a window
of span 16 then lies entirely in the overlap), a set that piles its adds onto a few cells under a low flush threshold, and
other launch geometries.  Every set is packed on the host and uploaded."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi, em
from tests import gapped_ref, kmer_ref

pytestmark = pytest.mark.gpu

WS = (6, 8)
MAX_POS = 8192                                               # BAMM_MAX_SEQ_POSITIONS
S_MAX = 16
STRANDS = pytest.mark.parametrize("single_strand", [False, True], ids=["ds", "ss"])


def lengths_for(w: int):
    """Around the smallest span, around the largest (16 - 1, 16, 16 + 1: the word edge as well) and around the later edges."""
    return [w - 1, w, w + 1, 15, 16, 17, 31, 32, 33, 47, 48, 49]


def rnd_records(rs, lengths):
    return [rs.randint(1, 5, size=int(n)).astype(np.uint8) for n in lengths]


def length_set(w: int):
    rs = np.random.RandomState(1100 + w)
    return rnd_records(rs, [L for L in lengths_for(w) for _ in range(64)])


def unknown_set(w: int):
    """The same lengths, 64 records each: record r of a length carries pattern r mod 37 -- one unknown at 0, 1, 15, 16 or
    L - 1, or a pair at distance 1, S - 1, S or S + 1 for a span S of w, w + 1, w + 4 or 16, starting at position 3 or 14
    (positions beyond the record are dropped)."""
    rs = np.random.RandomState(1200 + w)
    dists = sorted({1} | {S + d for S in (w, w + 1, w + 4, S_MAX) for d in (-1, 0, 1)})
    pairs = [(a, a + d) for d in dists for a in (3, 14)]
    recs = []
    for L in lengths_for(w):
        for r, rec in enumerate(rnd_records(rs, [L] * 64)):
            p = r % (5 + len(pairs))
            at = [[0], [1], [15], [16], [L - 1]][p] if p < 5 else pairs[p - 5]
            for z in at:
                if 0 <= z < L:
                    rec[z] = 0
            recs.append(rec)
    return recs


def long_set(w: int, seg: int):
    """Two records beyond BAMM_MAX_SEQ_POSITIONS, 8 193 and 20 011 positions, with unknowns on a cut, S - 1 before it and
    just behind it for the spans w, w + 3 and 16, at several cuts of `seg` positions (and of the default 8192)."""
    rs = np.random.RandomState(1400 + w)
    recs = rnd_records(rs, [8193, 20011])
    for rec in recs:
        for cut in (seg, 2 * seg, 5 * seg, 17 * seg, 40 * seg, MAX_POS, 2 * MAX_POS):
            for z in [cut, cut + 1] + [cut - d for S in (w, w + 3, S_MAX) for d in (S - 1, S)]:
                if 0 <= z < len(rec) and rs.random_sample() < 0.6:
                    rec[z] = 0
    return recs


def flush_set():
    return [kmer_ref.codes_of("ACGTTGCAAGGCTTACGCGTAACCGGTTACGTACGTAAAA")] * 4096


def device_tables(ctx, codes, off, w, lo, hi, single_strand):
    packed = bm.PackedSeqs.from_codes(codes, off, single_strand)
    seqs = bm.SeqSet(ctx, packed)
    try:
        return em.kmer_counts_gapped(ctx, seqs, w, lo, hi)
    finally:
        seqs.close(); packed.free()


def check(ctx, recs, w, single_strand, want=None):
    """Device tables of all gaps == oracle == host twin; returns the tables."""
    codes, off = kmer_ref.concat(recs)
    G = S_MAX - w
    if want is None:
        want = gapped_ref.gapped_counts_ref(codes, off, w, 0, G, single_strand)
    got, totals = device_tables(ctx, codes, off, w, 0, G, single_strand)
    host, host_totals = em.kmer_counts_gapped_host(codes, off, w, 0, G, single_strand)
    assert got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(host, want)
    assert np.array_equal(totals, want.sum(axis=1)) and np.array_equal(host_totals, totals)
    return got


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_record_lengths(gpu_ctx, w, single_strand):
    got = check(gpu_ctx, length_set(w), w, single_strand)
    assert (got.sum(axis=1) > 0).all()                        # every span up to 16 has windows in these records


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_unknowns(gpu_ctx, w, single_strand):
    check(gpu_ctx, unknown_set(w), w, single_strand)


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_long_records(gpu_ctx, w, single_strand):
    recs = long_set(w, 64)
    codes, off = kmer_ref.concat(recs)
    want = gapped_ref.gapped_counts_ref(codes, off, w, 0, S_MAX - w, single_strand)
    try:
        for seg in (0, 16, 64, 1008):                       # the default cut, and short segments: at 16 a segment is one word
            gpu_ctx.set_tuning(kmer_segment_positions=seg)
            check(gpu_ctx, recs, w, single_strand, want)
    finally:
        gpu_ctx.set_tuning(kmer_segment_positions=0)


@pytest.mark.parametrize("w", WS)
def test_flush_rule(gpu_ctx, w):
    """4 096 copies of one 40-base record: a few cells of every gap's table take every add.  Nothing wraps, nothing is lost
    between flushes, whether the workgroups flush once at the end or after every few hundred windows."""
    recs = flush_set()
    codes, off = kmer_ref.concat(recs[:1])
    want = gapped_ref.gapped_counts_ref(codes, off, w, 0, S_MAX - w, False) * np.uint64(4096)
    try:
        for threshold in (0, 300, 1):
            gpu_ctx.set_tuning(kmer_flush_windows=threshold)
            got = check(gpu_ctx, recs, w, False, want)
        assert (got.max(axis=1) >= 4096).all()
    finally:
        gpu_ctx.set_tuning(kmer_flush_windows=0)


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_mixed_set_and_launch_geometry(gpu_ctx, w, single_strand):
    recs = length_set(w)[::4] + unknown_set(w)[::3] + long_set(w, 64)[:1] + flush_set()[:512]
    codes, off = kmer_ref.concat(recs)
    want = gapped_ref.gapped_counts_ref(codes, off, w, 0, S_MAX - w, single_strand)
    try:
        gpu_ctx.set_tuning(kmer_segment_positions=2048)
        tables = []
        for blocks in (0, 1, 3):
            gpu_ctx.set_launch(blocks=blocks)
            tables.append(check(gpu_ctx, recs, w, single_strand, want))
        assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], tables[2])
    finally:
        gpu_ctx.set_launch(0, 0)
        gpu_ctx.set_tuning(kmer_segment_positions=0)


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_consistency_with_the_contiguous_call_and_single_gaps(gpu_ctx, w, single_strand):
    """Gap 0 of the gapped call is bamm_kmer_counts' table, and a call for one gap (or a range that starts above 0) gives the
    slices of the call for all of them."""
    recs = unknown_set(w)[::2] + long_set(w, 64)[:1]
    codes, off = kmer_ref.concat(recs)
    G = S_MAX - w
    packed = bm.PackedSeqs.from_codes(codes, off, single_strand)
    seqs = bm.SeqSet(gpu_ctx, packed)
    try:
        whole, totals = em.kmer_counts_gapped(gpu_ctx, seqs, w, 0, G)
        flat, flat_total = em.kmer_counts(gpu_ctx, seqs, w)
        assert np.array_equal(whole[0], flat) and int(totals[0]) == flat_total
        assert np.array_equal(flat, kmer_ref.counts_ref(codes, off, w, single_strand))
        for g in (0, 1, 4, G):
            one, one_total = em.kmer_counts_gapped(gpu_ctx, seqs, w, g, g)
            assert one.shape == (1, 4 ** w)
            assert np.array_equal(one[0], whole[g]) and int(one_total[0]) == int(totals[g])
        part, part_totals = em.kmer_counts_gapped(gpu_ctx, seqs, w, 3, G - 1)
        assert np.array_equal(part, whole[3:G]) and np.array_equal(part_totals, totals[3:G])
        seven, seven_total = em.kmer_counts_gapped(gpu_ctx, seqs, 7, 0, 0)       # the odd width passes with gap 0 alone
        assert np.array_equal(seven[0], em.kmer_counts(gpu_ctx, seqs, 7)[0])
    finally:
        seqs.close(); packed.free()


def test_empty_set_and_records_without_windows(gpu_ctx):
    got, totals = device_tables(gpu_ctx, np.zeros(0, np.uint8), np.zeros(1, np.uint64), 6, 0, 10, False)
    assert got.shape == (11, 4096) and not got.any() and not totals.any()
    codes, off = kmer_ref.concat([np.zeros(20, np.uint8), kmer_ref.codes_of("ACGTA"), np.zeros(0, np.uint8)])
    got, totals = device_tables(gpu_ctx, codes, off, 8, 0, 8, False)
    assert not got.any() and not totals.any()


def test_refusals(gpu_ctx):
    recs = length_set(6)[:8]
    codes, off = kmer_ref.concat(recs)
    packed = bm.PackedSeqs.from_codes(codes, off, True)
    from_kmers = bm.PackedSeqs.from_kmers(packed.unpack_y(10).astype(np.uint64), packed.offsets())
    no_list = bm.SeqSet(gpu_ctx, from_kmers)
    with_list = bm.SeqSet(gpu_ctx, packed)
    try:
        with pytest.raises(abi.BammError) as e:
            em.kmer_counts_gapped(gpu_ctx, no_list, 8, 0, 4)
        assert e.value.code == abi.ERR_UNSUPPORTED and "kmer_" in str(e.value)
        for w, lo, hi in ((7, 0, 1), (7, 2, 2), (6, 0, 11), (8, 0, 9), (8, 9, 9), (6, 3, 2), (5, 0, 0), (9, 0, 0)):
            with pytest.raises(abi.BammError) as e:
                em.kmer_counts_gapped(gpu_ctx, with_list, w, lo, hi)
            assert e.value.code == abi.ERR_ARG, (w, lo, hi)
        other = bm.Context(0)                                 # a set of another context
        try:
            with pytest.raises(abi.BammError) as e:
                em.kmer_counts_gapped(other, with_list, 8, 0, 4)
            assert e.value.code == abi.ERR_ARG
        finally:
            other.close()
    finally:
        no_list.close(); with_list.close(); from_kmers.free(); packed.free()
