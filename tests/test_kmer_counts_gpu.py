"""bamm_kmer_counts (csrc/kmer_count.hip) against the numpy oracle of tests/kmer_ref.py and against its host twin: exact
integers, every comparison is array_equal.  The shapes are the smallest at which the kernel can go wrong: record lengths
around the word and dword edges of the 2-bit stream (with both strands the separator lands at every phase of a word),
unknown bases at those edges and in pairs around the window's width, the boundaries of every length class, records beyond
BAMM_MAX_SEQ_POSITIONS cut into short segments with unknowns on the cuts, a set that piles its adds onto a few cells
under a low flush threshold, and all of it at once under other launch geometries."""
import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi, em
from tests import em_classes, kmer_ref

pytestmark = pytest.mark.gpu

WS = (6, 7, 8)
MAX_POS = 8192                                               # BAMM_MAX_SEQ_POSITIONS


def lengths_for(w: int):
    return [w, 15, 16, 17, 31, 32, 33, 47, 48, 49]


def rnd_records(rs, lengths):
    return [rs.randint(1, 5, size=int(n)).astype(np.uint8) for n in lengths]


def length_set(w: int):
    rs = np.random.RandomState(100 + w)
    return rnd_records(rs, [L for L in lengths_for(w) for _ in range(64)])


def unknown_set(w: int):
    """The same lengths, 64 records each: record r of a length carries pattern r mod 13 -- one unknown at 0, 1, 15, 16 or
    L - 1, or a pair at distance 1, w - 1, w or w + 1 starting at position 3 or 14 (positions beyond the record are dropped)."""
    rs = np.random.RandomState(200 + w)
    recs = []
    for L in lengths_for(w):
        for r, rec in enumerate(rnd_records(rs, [L] * 64)):
            p = r % 13
            at = [[0], [1], [15], [16], [L - 1]][p] if p < 5 else [(3, 14)[(p - 5) % 2], (3, 14)[(p - 5) % 2] + (1, w - 1, w, w + 1)[(p - 5) // 2]]
            for z in at:
                if 0 <= z < L:
                    rec[z] = 0
            recs.append(rec)
    return recs


def class_set(M: int):
    """Single-stranded records just under, on and just over the boundary of the class of M positions per lane, a few unknowns in each."""
    rs = np.random.RandomState(300 + M)
    boundary = em_classes.edge_lengths(M, 8)[1]              # the class's longest record
    recs = rnd_records(rs, [boundary - 1, boundary, boundary + 1])
    for rec in recs:
        rec[rs.randint(0, len(rec), size=3)] = 0
    return recs


def long_set(w: int, seg: int):
    """Two records beyond BAMM_MAX_SEQ_POSITIONS, 8193 and about 20 000 positions, with unknowns on a cut, w - 1 before it and
    just behind it, at several cuts of `seg` positions (and of the default 8192)."""
    rs = np.random.RandomState(400 + w)
    recs = rnd_records(rs, [8193, 20011])
    for rec in recs:
        for cut in (seg, 2 * seg, 5 * seg, 17 * seg, MAX_POS, 2 * MAX_POS):
            for z in (cut, cut - (w - 1), cut + 1, cut - w):
                if 0 <= z < len(rec) and rs.random_sample() < 0.7:
                    rec[z] = 0
    return recs


def flush_set():
    return [kmer_ref.codes_of("ACGTTGCAAGGCTTACGCGTAACCGGTTACGTACGTAAAA")] * 4096


def check(ctx, recs, w, single_strand, want=None):
    """Device table == oracle == host twin; returns the table."""
    codes, off = kmer_ref.concat(recs)
    if want is None:
        want = kmer_ref.counts_ref(codes, off, w, single_strand)
    packed = bm.PackedSeqs.from_codes(codes, off, single_strand)
    seqs = bm.SeqSet(ctx, packed)
    try:
        got, total = em.kmer_counts(ctx, seqs, w)
    finally:
        seqs.close(); packed.free()
    host, host_total = em.kmer_counts_host(codes, off, w, single_strand)
    assert np.array_equal(got, want)
    assert np.array_equal(host, want)
    assert total == host_total == int(want.sum())
    return got


STRANDS = pytest.mark.parametrize("single_strand", [False, True], ids=["ds", "ss"])


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_record_lengths(gpu_ctx, w, single_strand):
    check(gpu_ctx, length_set(w), w, single_strand)


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_unknowns(gpu_ctx, w, single_strand):
    check(gpu_ctx, unknown_set(w), w, single_strand)


@pytest.mark.parametrize("M", em_classes.M_CLASSES)
def test_length_classes(gpu_ctx, M):
    recs = class_set(M)
    for w in WS:
        check(gpu_ctx, recs, w, True)
    check(gpu_ctx, recs[:2] + [recs[2][: len(recs[2]) // 2]], 7, False)     # both strands: 2 L + 1 positions straddle later classes


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_long_records(gpu_ctx, w, single_strand):
    recs = long_set(w, 64)
    codes, off = kmer_ref.concat(recs)
    want = kmer_ref.counts_ref(codes, off, w, single_strand)
    try:
        for seg in (0, 64, 1008, 16):                       # the default cut, and short segments: many edges
            gpu_ctx.set_tuning(kmer_segment_positions=seg)
            check(gpu_ctx, recs, w, single_strand, want)
    finally:
        gpu_ctx.set_tuning(kmer_segment_positions=0)


@pytest.mark.parametrize("w", WS)
def test_flush_rule(gpu_ctx, w):
    """4 096 copies of one 40-base record: a few cells take every add.  Nothing wraps, nothing is lost between flushes,
    whether the workgroups flush once at the end or after every few hundred windows."""
    recs = flush_set()
    codes, off = kmer_ref.concat(recs[:1])
    one = kmer_ref.counts_ref(codes, off, w, False)
    want = one * np.uint64(4096)
    try:
        for threshold in (0, 300, 1):
            gpu_ctx.set_tuning(kmer_flush_windows=threshold)
            got = check(gpu_ctx, recs, w, False, want)
        assert got.max() >= 4096
    finally:
        gpu_ctx.set_tuning(kmer_flush_windows=0)


@STRANDS
@pytest.mark.parametrize("w", WS)
def test_mixed_set_and_launch_geometry(gpu_ctx, w, single_strand):
    recs = length_set(w)[::4] + unknown_set(w)[::3] + class_set(8) + class_set(em_classes.M_CLASSES[-1]) + long_set(w, 64)[:1] + flush_set()[:512]
    codes, off = kmer_ref.concat(recs)
    want = kmer_ref.counts_ref(codes, off, w, single_strand)
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
def test_uploaded_range_of_a_host_packed_set(gpu_ctx, single_strand):
    """bamm_seqs_upload of records [begin, end) of a set bamm_pack_codes made: the list of unknown positions travels with the
    packed set and is cut with it."""
    recs = unknown_set(7)
    codes, off = kmer_ref.concat(recs)
    packed = bm.PackedSeqs.from_codes(codes, off, single_strand)
    try:
        for begin, end in ((0, len(recs)), (37, 411), (5, 5)):
            seqs = bm.SeqSet(gpu_ctx, packed, begin, end)
            try:
                got, total = em.kmer_counts(gpu_ctx, seqs, 7)
            finally:
                seqs.close()
            c2, o2 = kmer_ref.concat(recs[begin:end])
            want = kmer_ref.counts_ref(c2, o2, 7, single_strand)
            assert np.array_equal(got, want) and total == int(want.sum())
    finally:
        packed.free()


def test_refusals(gpu_ctx):
    recs = length_set(6)[:8]
    codes, off = kmer_ref.concat(recs)
    packed = bm.PackedSeqs.from_codes(codes, off, True)
    from_kmers = bm.PackedSeqs.from_kmers(packed.unpack_y(10).astype(np.uint64), packed.offsets())
    seqs = bm.SeqSet(gpu_ctx, from_kmers)
    with_list = bm.SeqSet(gpu_ctx, packed)
    try:
        with pytest.raises(abi.BammError) as e:
            em.kmer_counts(gpu_ctx, seqs, 8)
        assert e.value.code == abi.ERR_UNSUPPORTED and "kmer_" in str(e.value)
        dev_packed, dev_set = bm.SeqSet.from_codes(gpu_ctx, codes, off, True)      # packed on the device: no list either
        try:
            with pytest.raises(abi.BammError) as e:
                em.kmer_counts(gpu_ctx, dev_set, 8)
            assert e.value.code == abi.ERR_UNSUPPORTED
        finally:
            dev_set.close(); dev_packed.free()
        for w in (5, 9, 0):
            with pytest.raises(abi.BammError) as e:
                em.kmer_counts(gpu_ctx, with_list, w)
            assert e.value.code == abi.ERR_ARG
    finally:
        seqs.close(); with_list.close(); from_kmers.free(); packed.free()
