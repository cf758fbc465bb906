"""The host half of --seedGaps without a GPU: the host dyad counter against the numpy oracle (tests/gapped_ref.py), the
cross-gap ranking (host/seeder.cpp, kmer_seeds_gapped) against its restatement and on a scripted table, the seed file through
the existing MEME reader, the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi, build, em
from tests import gapped_ref, kmer_ref
from tests.kmer_ref import codes_of, kmer_of

WS = (6, 8)
vp = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host(lib):
    build.build_host()
    H = C.CDLL(build.HOST_LIB)
    H.bh_last_error.restype = C.c_char_p
    return H


def edge_records(w: int):
    """The records the host counter can go wrong on, for every span S = w .. 16 at once."""
    rs = np.random.RandomState(700 + w)
    rnd = lambda n: rs.randint(1, 5, size=n).astype(np.uint8)
    h = w // 2
    recs = [np.zeros(19, np.uint8), np.zeros(0, np.uint8)]                              # all unknown, empty
    r = rnd(40); r[0] = 0; r[-1] = 0; recs.append(r)                                    # unknowns at the first and last position
    for S in range(w, 17):
        recs += [rnd(S - 1), rnd(S), rnd(S + 1)]                                        # shorter than, exactly, one above the span
        for d in (S - 1, S, S + 1):                                                     # two unknowns fewer than / exactly / more than S apart
            r = rnd(60); r[12] = 0; r[12 + d] = 0; recs.append(r)
        if S > w:
            r = rnd(S); r[h] = 0; recs.append(r)                                        # exactly S, its only unknown in the gap: no window
            r = rnd(S); r[S - h - 1] = 0; recs.append(r)                                # ... at the gap's last position
    recs.append(codes_of("ACGTTCGT" if w == 6 else "ACGTTTACGT"))                       # reverse-palindromic dyad at gap 2
    recs += [rnd(int(n)) for n in rs.randint(w, 120, size=40)]
    r = rnd(500); r[rs.random_sample(500) < 0.03] = 0; recs.append(r)
    return kmer_ref.concat(recs)


@pytest.mark.parametrize("single_strand", [False, True], ids=["ds", "ss"])
@pytest.mark.parametrize("w", WS)
def test_host_counter_matches_oracle(lib, w, single_strand):
    codes, off = edge_records(w)
    G = 16 - w
    want = gapped_ref.gapped_counts_ref(codes, off, w, 0, G, single_strand)
    for threads in (1, 5):
        lib.bamm_set_host_threads(threads)
        try:
            got, totals = em.kmer_counts_gapped_host(codes, off, w, 0, G, single_strand)
        finally:
            lib.bamm_set_host_threads(0)
        assert got.shape == (G + 1, 4 ** w)
        assert np.array_equal(got, want)
        assert np.array_equal(totals, want.sum(axis=1))
    assert (want.sum(axis=1) > 0).all()
    # gap 0 is the contiguous table, and a range that starts above 0 is a slice of the whole
    assert np.array_equal(got[0], em.kmer_counts_host(codes, off, w, single_strand)[0])
    part, part_totals = em.kmer_counts_gapped_host(codes, off, w, 2, 5, single_strand)
    assert np.array_equal(part, want[2:6]) and np.array_equal(part_totals, want[2:6].sum(axis=1))
    if not single_strand:                                     # both strands: every gap's table is its own reverse complement
        rc = kmer_ref.revcomp(np.arange(4 ** w), w)
        for g in range(G + 1):
            assert np.array_equal(want[g], want[g][rc])


def test_gap_zero_at_seven_is_the_contiguous_table(lib):
    codes, off = edge_records(6)
    got, totals = em.kmer_counts_gapped_host(codes, off, 7, 0, 0)
    want, total = em.kmer_counts_host(codes, off, 7)
    assert np.array_equal(got[0], want) and int(totals[0]) == total
    assert np.array_equal(want, kmer_ref.counts_ref(codes, off, 7, False))


def test_unknown_in_the_gap_is_not_counted(lib):
    """ACG nn CGT: a window whose only unknown base lies between its halves adds nothing, at the gap it spans; the gaps whose
    windows avoid it still count."""
    codes, off = kmer_ref.concat([codes_of("ACGNTCGT")])
    got, totals = em.kmer_counts_gapped_host(codes, off, 6, 0, 2, True)
    assert totals.tolist() == [0, 0, 0]
    codes, off = kmer_ref.concat([codes_of("ACGATCGT")])
    got, totals = em.kmer_counts_gapped_host(codes, off, 6, 0, 2, True)
    assert totals.tolist() == [3, 2, 1] and got[2, kmer_of("ACGCGT")] == 1


def test_palindromic_dyad_counts_twice(lib):
    codes, off = kmer_ref.concat([codes_of("ACGTTCGT")])      # ACG nn CGT is its own reverse complement
    got, totals = em.kmer_counts_gapped_host(codes, off, 6, 2, 2, False)
    assert got[0, kmer_of("ACGCGT")] == 2 and int(totals[0]) == 2
    got, totals = em.kmer_counts_gapped_host(codes, off, 6, 2, 2, True)
    assert got[0, kmer_of("ACGCGT")] == 1 and int(totals[0]) == 1


@pytest.mark.parametrize("w,lo,hi", [(7, 0, 1), (7, 1, 1), (6, 0, 11), (8, 0, 9), (8, 9, 9), (6, 3, 2), (8, 1, 0), (5, 0, 0), (9, 0, 0)])
def test_host_counter_refusals(lib, w, lo, hi):
    codes, off = kmer_ref.concat([codes_of("ACGTACGTACGTACGTACGT")])
    with pytest.raises(abi.BammError) as e:
        em.kmer_counts_gapped_host(codes, off, w, lo, hi)
    assert e.value.code == abi.ERR_ARG


def test_empty_set_gives_zeroed_tables(lib):
    got, totals = em.kmer_counts_gapped_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 6, 0, 3)
    assert got.shape == (4, 4096) and not got.any() and not totals.any()


# ---- ranking ------------------------------------------------------------------------------------------------------------
def random_bg(K: int, seed: int) -> np.ndarray:
    """Conditional probabilities of every order up to K, each context's four summing to 1 (flat [k][y])."""
    rs = np.random.RandomState(seed)
    parts = []
    for k in range(K + 1):
        v = rs.randint(1, 50, size=(4 ** k, 4)).astype(np.float64)
        parts.append((v / v.sum(axis=1, keepdims=True)).ravel())
    return np.concatenate(parts).astype(np.float32)


def same_seeds(got, want):
    (k, g, z, p), (rk, rg, rz, rp) = got, want
    assert np.array_equal(k, rk) and np.array_equal(g, rg) and np.array_equal(z, rz)
    assert len(p) == len(rp)
    for a, b in zip(p, rp):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("Kbg", [0, 1, 2, 4])
@pytest.mark.parametrize("w", WS)
def test_ranking_against_restatement(host, w, Kbg):
    """Tables counted from records with a planted dyad, a background of every order the expectation can take: the same
    w-mers, gaps, z and PWM bits as the numpy restatement, over all gaps and over a range that starts above 0."""
    rs = np.random.RandomState(87 + w)
    recs = [rs.randint(1, 5, size=60).astype(np.uint8) for _ in range(300)]
    h = w // 2
    for r in recs[::2]:
        r[20:20 + h] = codes_of("TGAC"[:h])
        r[23 + h:23 + w] = codes_of("GCAT"[:h])               # the halves 3 apart
    codes, off = kmer_ref.concat(recs)
    vbg = random_bg(Kbg, 5 + Kbg)
    for single_strand in (False, True):
        for lo, hi in ((0, 16 - w), (2, 4)):
            counts, totals = em.kmer_counts_gapped_host(codes, off, w, lo, hi, single_strand)
            got = em.kmer_seeds_gapped(counts, totals, vbg, Kbg, w, lo, hi, max_seeds=4, single_strand=single_strand)
            same_seeds(got, gapped_ref.gapped_seeds_ref(counts, totals, vbg, Kbg, w, lo, hi, 4, single_strand))
            assert len(got[0]) == 4
            for y, g, p in zip(got[0], got[1], got[3]):
                assert p.shape == (4, w + g) and (p[:, h:h + g] == np.float32(0.25)).all()
                assert np.allclose(p.sum(axis=0), 1.0, atol=1e-6)


def test_gap_zero_alone_is_kmer_seeds(host):
    rs = np.random.RandomState(9)
    recs = [rs.randint(1, 5, size=60).astype(np.uint8) for _ in range(200)]
    for r in recs[::2]:
        r[10:18] = codes_of("TGACTCAT")
    codes, off = kmer_ref.concat(recs)
    vbg = random_bg(2, 3)
    for w in (6, 7, 8):
        counts, totals = em.kmer_counts_gapped_host(codes, off, w, 0, 0)
        k, g, z, p = em.kmer_seeds_gapped(counts, totals, vbg, 2, w, 0, 0, max_seeds=4)
        k0, z0, p0 = em.kmer_seeds(counts[0], int(totals[0]), vbg, 2, w, max_seeds=4)
        assert np.array_equal(k, k0) and np.array_equal(z, z0) and not g.any()
        assert np.array_equal(np.array(p).view(np.uint32), p0.view(np.uint32))


@pytest.mark.parametrize("single_strand", [True, False], ids=["ss", "ds"])
def test_cross_gap_rule_on_a_scripted_table(host, single_strand):
    """Every cell at 100; a planted cell at gap 3; at gap 4 a cell with the plant's left half (a shifted copy, as a dyad leaves
    at the neighbouring gaps) above every unrelated cell; unrelated cells at gaps 3 and 4.  The copy is skipped, the unrelated
    ones are taken in order of z."""
    w, lo, hi = 8, 2, 5
    t = np.full((hi - lo + 1, 4 ** w), 100, np.uint64)
    plant, copy_l, copy_r = kmer_of("TGACGCAT"), kmer_of("TGACCCCA"), kmer_of("AAGAGCAT")
    other3, other4 = kmer_of("GGAAGGAA"), kmer_of("CCTTTTGG")

    def put(g, y, c):
        t[g - lo, y] = c
        if not single_strand:
            t[g - lo, int(kmer_ref.revcomp(y, w))] = c
    put(3, plant, 900); put(4, copy_l, 800); put(2, copy_r, 700); put(4, other4, 600); put(3, other3, 500)
    totals = t.sum(axis=1)
    vbg = np.full(4, 0.25, np.float32)
    k, g, z, p = em.kmer_seeds_gapped(t, totals, vbg, 0, w, lo, hi, max_seeds=10, single_strand=single_strand)
    canon = (lambda y: y) if single_strand else (lambda y: min(y, int(kmer_ref.revcomp(y, w))))
    if single_strand:
        assert list(zip(k.tolist(), g.tolist())) == [(plant, 3), (other4, 4), (other3, 3)]
    else:
        assert [(canon(int(y)), int(gg)) for y, gg in zip(k, g)] == [(canon(plant), 3), (canon(other4), 4), (canon(other3), 3)]
        assert len(k) == 3
    assert z[0] > z[1] > z[2] > 0
    same_seeds((k, g, z, p), gapped_ref.gapped_seeds_ref(t, totals, vbg, 0, w, lo, hi, 10, single_strand))
    # the copies do rank above the unrelated cells: at their own gaps alone they come first
    k4, g4, _, _ = em.kmer_seeds_gapped(t[2:3], totals[2:3], vbg, 0, w, 4, 4, max_seeds=1, single_strand=single_strand)
    assert canon(int(k4[0])) == canon(copy_l) and int(g4[0]) == 4


def test_planted_dyad_ranks_first_on_the_host(host):
    """The premise of tests/test_cli_seed_gaps_gpu.py's planted run, without the command line or a GPU: on planted_dyad_set()
    with the set's own order-2 background the host twin and the ranking put TGAC nnnn GCAT, or its reverse complement, first
    at gap 4, more than 3 x above the second seed -- the cross-gap rule having removed the shifted copies."""
    codes, off = gapped_ref.planted_dyad_set()
    counts, totals = em.kmer_counts_gapped_host(codes, off, 8, 0, 6)
    vbg = bm.PackedSeqs.from_codes(codes, off, False, seed=42).bg_model(2, np.array([1, 10, 10], np.float32))
    y = kmer_of(gapped_ref.LEFT + gapped_ref.RIGHT)
    for kmers, gaps, z, _ in (gapped_ref.gapped_seeds_ref(counts, totals, vbg, 2, 8, 0, 6, 4, False),
                              em.kmer_seeds_gapped(counts, totals, vbg, 2, 8, 0, 6, 4)):
        print("planted dyad: seeds", [gapped_ref.dyad_string(int(k), 8, int(g)) for k, g in zip(kmers, gaps)], "z", z.tolist())
        assert int(kmers[0]) in (y, int(kmer_ref.revcomp(y, 8))) and int(gaps[0]) == gapped_ref.PLANT_GAP
        assert z[0] > 3 * z[1]


# ---- seed file -----------------------------------------------------------------------------------------------------------
def read_motif(host, path, i, width):
    got = np.zeros((4, width), np.float32)
    nm, wo = C.c_uint32(0), C.c_uint32(0)
    assert host.bh_read_meme_pwm(str(path).encode(), C.c_uint32(i), C.byref(nm), C.byref(wo), vp(got), C.c_uint64(got.size)) == 0, host.bh_last_error()
    assert wo.value == width
    return nm.value, got


def test_meme_round_trip_with_gaps(host, tmp_path):
    """A dyad is written with its gap as n's, at width w + g, ' gap= g' behind the z-score; it comes back through load_seeds'
    MEME reader at that width with the floats it was given and gap columns of exactly 0.25."""
    w, max_gap = 8, 5
    gaps = np.array([4, 0, 5], np.uint32)
    rs = np.random.RandomState(4)
    pwm = np.zeros((3, 4 * (w + max_gap)), np.float32)
    mats = []
    for i, g in enumerate(gaps):
        m = rs.randint(1, 1000, size=(4, w + g)).astype(np.float64)
        m = (m / m.sum(axis=0, keepdims=True)).astype(np.float32)
        m[:, 4:4 + g] = 0.25
        mats.append(m)
        pwm[i, : m.size] = m.ravel()
    mats[0][:, 0] = np.float32([1 / 3, 1 / 7, np.nextafter(np.float32(0.5), np.float32(0)), 1 - 1 / 3 - 1 / 7 - 0.5])
    pwm[0, : mats[0].size] = mats[0].ravel()
    kmer = np.array([kmer_of("TGACGCAT"), kmer_of("TTTTGGGG"), kmer_of("ACGTACGT")], np.uint32)
    count = np.array([12, 2 ** 40 + 1, 7], np.uint64)
    z = np.array([1.5, 1e-3, 123456.789], np.float64)
    path = tmp_path / "x_seeds.meme"
    assert host.bh_kmer_seeds_write_gapped(str(path).encode(), C.c_uint32(w), C.c_uint32(max_gap), C.c_uint32(3), vp(kmer), vp(gaps), vp(count), vp(z), vp(pwm)) == 0, host.bh_last_error()
    text = open(path).read()
    assert "MOTIF TGACnnnnGCAT count= 12 z= 1.5 gap= 4\nletter-probability matrix: alength= 4 w= 12 nsites= 12\n" in text
    assert "MOTIF TTTTGGGG count= 1099511627777 z= 0.001\nletter-probability matrix: alength= 4 w= 8 " in text
    assert "MOTIF ACGTnnnnnACGT count= 7" in text and text.count("gap=") == 2
    for i, g in enumerate(gaps):
        n, got = read_motif(host, path, i, w + int(g))
        assert n == 3 and np.array_equal(got.view(np.uint32), mats[i].view(np.uint32))
        assert (got[:, 4:4 + int(g)] == np.float32(0.25)).all()


def test_seed_file_of_contiguous_seeds_keeps_its_bytes(host, tmp_path):
    w, n = 8, 3
    rs = np.random.RandomState(3)
    pwm = rs.randint(1, 1000, size=(n, 4, w)).astype(np.float64)
    pwm = np.ascontiguousarray((pwm / pwm.sum(axis=1, keepdims=True)).astype(np.float32))
    kmer = np.array([kmer_of("ACGTACGT"), kmer_of("TTTTGGGG"), 0], np.uint32)
    count = np.array([12, 2 ** 40 + 1, 0], np.uint64)
    z = np.array([1.5, 1e-3, 123456.789], np.float64)
    a, b = tmp_path / "a.meme", tmp_path / "b.meme"
    assert host.bh_kmer_seeds_write(str(a).encode(), C.c_uint32(w), C.c_uint32(n), vp(kmer), vp(count), vp(z), vp(pwm)) == 0
    assert host.bh_kmer_seeds_write_gapped(str(b).encode(), C.c_uint32(w), C.c_uint32(0), C.c_uint32(n), vp(kmer), vp(np.zeros(n, np.uint32)), vp(count), vp(z), vp(pwm)) == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    assert b"gap=" not in open(a, "rb").read()


# ---- command line --------------------------------------------------------------------------------------------------------
FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example", "JunD.fasta")


def run_cli(*args):
    return subprocess.run([build.CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


def test_cli_refusals(host, tmp_path):
    out = tmp_path / "o"
    for args in (("--seedGaps", 4), ("--seedGaps", 4, "--PWMFile", "x"), ("--seedKmers", 7, "--seedGaps", 2), ("--seedKmers", 7, "--seedGaps", 0)):
        p = run_cli(out, FASTA, *args)
        assert p.returncode == 1 and "Error: --seedGaps needs --seedKmers 6 or 8." in p.stderr, args
    for args in (("--seedKmers", 8, "--seedGaps", 9), ("--seedKmers", 6, "--seedGaps", 11), ("--seedKmers", 8, "--seedGaps", 2, 9), ("--seedKmers", 8, "--seedGaps", 9, 12)):
        p = run_cli(out, FASTA, *args)
        assert p.returncode == 1 and "Error: --seedGaps: w + gap may not exceed 16." in p.stderr, args
    p = run_cli(out, FASTA, "--seedKmers", 8, "--seedGaps", 5, 2)
    assert p.returncode == 1 and "--seedGaps" in p.stderr
    p = run_cli(out, FASTA, "--seedKmers", 8, "--seedGaps")
    assert p.returncode == 1 and "--seedGaps" in p.stderr
    assert not os.path.exists(out / "JunD_seeds.meme")


def test_cli_seed_file_on_the_host(host, tmp_path):
    """Without a GPU stage the driver counts on the host: OUTDIR/<base>_seeds.meme holds the seeds the Python entry points give
    for the same records and the background model the driver learns, each at its own width, and the initial models are
    written from it."""
    out = tmp_path / "o"
    p = run_cli(out, FASTA, "--seedKmers", 8, "--seedGaps", 6, "--maxPWM", 3, "--timing")
    assert p.returncode == 0, p.stderr
    assert "dyad counts on the host (--seedKmers --seedGaps, gaps 0..6)" in p.stderr and "rank dyads (gaps 0..6)" in p.stderr
    n, nc = C.c_uint64(0), C.c_uint64(0)
    assert host.bh_read_fasta(FASTA.encode(), C.byref(n), C.byref(nc), None, None, None) == 0
    codes, off = np.zeros(nc.value, np.uint8), np.zeros(n.value + 1, np.uint64)
    assert host.bh_read_fasta(FASTA.encode(), C.byref(n), C.byref(nc), vp(codes), vp(off), None) == 0
    counts, totals = em.kmer_counts_gapped_host(codes, off, 8, 0, 6)
    vbg = bm.PackedSeqs.from_codes(codes, off, False, seed=42).bg_model(2, np.array([1, 10, 10], np.float32))
    kmers, gaps, z, pwms = em.kmer_seeds_gapped(counts, totals, vbg, 2, 8, 0, 6, max_seeds=3)
    assert len(kmers) == 3
    names = [l.split()[1] for l in open(out / "JunD_seeds.meme").read().split("\n") if l.startswith("MOTIF ")]
    assert names == [gapped_ref.dyad_string(int(k), 8, int(g)) for k, g in zip(kmers, gaps)]
    for i in range(3):
        nm, got = read_motif(host, out / "JunD_seeds.meme", i, 8 + int(gaps[i]))
        assert nm == 3 and np.array_equal(got.view(np.uint32), pwms[i].view(np.uint32))
    assert all(os.path.exists(out / f"JunD_motif_{i}.ihbcp") for i in (1, 2, 3))
    assert not os.path.exists(out / "JunD_motif_4.ihbcp")


def test_cli_gap_zero_writes_the_contiguous_seed_file(host, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    assert run_cli(a, FASTA, "--seedKmers", 8, "--maxPWM", 3).returncode == 0
    assert run_cli(b, FASTA, "--seedKmers", 8, "--seedGaps", 0, "--maxPWM", 3).returncode == 0
    assert open(a / "JunD_seeds.meme", "rb").read() == open(b / "JunD_seeds.meme", "rb").read()
