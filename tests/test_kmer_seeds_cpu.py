"""The host half of the de novo seeder without a GPU: the host w-mer counter against the numpy oracle (tests/kmer_ref.py),
the ranking (host/seeder.cpp) on a scripted table, the seed file through the existing MEME reader, the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import abi, build, em
from tests import kmer_ref
from tests.kmer_ref import codes_of, kmer_of

WS = (6, 7, 8)


@pytest.fixture(scope="module")
def host(lib):
    build.build_host()
    H = C.CDLL(build.HOST_LIB)
    H.bh_last_error.restype = C.c_char_p
    return H


def edge_records(w: int):
    """The records the host counter can go wrong on, for windows of w."""
    rs = np.random.RandomState(600 + w)
    rnd = lambda n: rs.randint(1, 5, size=n).astype(np.uint8)
    recs = [rnd(w - 1), rnd(w), np.zeros(w + 3, np.uint8), np.zeros(0, np.uint8)]     # shorter than w, exactly w, all unknown, empty
    r = rnd(30); r[0] = 0; r[-1] = 0; recs.append(r)                                   # unknowns at the first and last position
    for d in (1, w - 1, w, w + 1):                                                     # two unknowns fewer than / exactly / more than w apart
        r = rnd(40); r[12] = 0; r[12 + d] = 0; recs.append(r)
    r = rnd(w); r[w // 2] = 0; recs.append(r)                                          # exactly w with an unknown: no window
    recs.append(codes_of("ACGCGT"))                                                    # reverse-palindromic 6-mer
    recs.append(codes_of("TTACGCGTAA"))                                                # ... inside a record, and the palindromic 8-mer TACGCGTA
    recs += [rnd(int(n)) for n in rs.randint(w, 120, size=40)]
    r = rnd(500); r[rs.random_sample(500) < 0.03] = 0; recs.append(r)
    return kmer_ref.concat(recs)


@pytest.mark.parametrize("single_strand", [False, True], ids=["ds", "ss"])
@pytest.mark.parametrize("w", WS)
def test_host_counter_matches_oracle(lib, w, single_strand):
    codes, off = edge_records(w)
    want = kmer_ref.counts_ref(codes, off, w, single_strand)
    for threads in (1, 5):
        lib.bamm_set_host_threads(threads)
        try:
            got, total = em.kmer_counts_host(codes, off, w, single_strand)
        finally:
            lib.bamm_set_host_threads(0)
        assert np.array_equal(got, want)
        assert total == int(want.sum())
    if not single_strand:                                     # both strands: the table is its own reverse complement
        assert np.array_equal(want, want[kmer_ref.revcomp(np.arange(4 ** w), w)])


def test_palindrome_counts_twice(lib):
    codes, off = kmer_ref.concat([codes_of("ACGCGT")])
    got, total = em.kmer_counts_host(codes, off, 6, False)
    assert got[kmer_of("ACGCGT")] == 2 and total == 2
    got, total = em.kmer_counts_host(codes, off, 6, True)
    assert got[kmer_of("ACGCGT")] == 1 and total == 1


@pytest.mark.parametrize("w", [0, 5, 9, 11])
def test_host_counter_refuses_other_widths(lib, w):
    codes, off = kmer_ref.concat([codes_of("ACGTACGTACGT")])
    with pytest.raises(abi.BammError) as e:
        em.kmer_counts_host(codes, off, w)
    assert e.value.code == abi.ERR_ARG


# ---- ranking ------------------------------------------------------------------------------------------------------------
def random_bg(K: int, seed: int) -> np.ndarray:
    """Conditional probabilities of every order up to K, each context's four summing to 1 (flat [k][y])."""
    rs = np.random.RandomState(seed)
    parts = []
    for k in range(K + 1):
        v = rs.randint(1, 50, size=(4 ** k, 4)).astype(np.float64)
        parts.append((v / v.sum(axis=1, keepdims=True)).ravel())
    return np.concatenate(parts).astype(np.float32)


def scripted_table(w: int, single_strand: bool):
    """Every cell at 100; a planted w-mer far above it with its neighbours raised; a pair of cells with equal counts (a tie in z
    under the uniform background); both strands: every raise mirrored onto the reverse complement."""
    t = np.full(4 ** w, 100, np.uint64)
    plant, tie_a, tie_b = kmer_of("ACGTTGCA"[:w] if w < 8 else "ACGTTGAC"), kmer_of("GGGGGGAC"[:w]), kmer_of("TTCTTTCC"[:w])

    def put(y, c):
        t[y] = c
        if not single_strand:
            t[int(kmer_ref.revcomp(y, w))] = c
    for j in range(w):
        for b in range(4):
            put((plant & ~(3 << (2 * j))) | (b << (2 * j)), 300 + 7 * j + b)
    put(plant, 900)
    put(tie_a, 500)
    put(tie_b, 500)
    return t, plant, tie_a, tie_b


@pytest.mark.parametrize("w", WS)
def test_ranking_uniform_background_ss(host, w):
    counts, plant, tie_a, tie_b = scripted_table(w, True)
    vbg = np.full(4, 0.25, np.float32)
    kmers, z, pwm = em.kmer_seeds(counts, int(counts.sum()), vbg, 0, w, max_seeds=10, single_strand=True)
    # the plant, then the tie in ascending cell order; the plant's neighbours (z > 0) are within Hamming distance 1 of it, and the
    # cells at 100 lie below their expectation: the walk ends at the first z <= 0, short of max_seeds
    assert [int(k) for k in kmers] == [plant] + sorted([tie_a, tie_b])
    assert z[1] == z[2] and z[0] > z[1] > 0
    rk, rz, rp = kmer_ref.seeds_ref(counts, int(counts.sum()), vbg, 0, w, 10, True)
    assert np.array_equal(kmers, rk) and np.array_equal(z, rz)
    assert np.array_equal(pwm.view(np.uint32), rp.view(np.uint32))
    # the plant's own column counts, written out: column j holds 900 + the raised neighbours of the other columns at the plant's
    # base and one raised neighbour at each other base
    col_sum = lambda j: 900 + sum(300 + 7 * jj + b for jj in range(w) for b in range(4) if b != (plant >> (2 * jj)) & 3)
    for j in range(w):
        bit = w - 1 - j
        own = (plant >> (2 * bit)) & 3
        n_own = col_sum(j) - sum(300 + 7 * bit + b for b in range(4) if b != own)
        assert pwm[0][own, j] == np.float32((n_own + 1.0) / (col_sum(j) + 4.0))
        for b in range(4):
            if b != own:
                assert pwm[0][b, j] == np.float32((300 + 7 * bit + b + 1.0) / (col_sum(j) + 4.0))
    assert em.kmer_seeds(counts, int(counts.sum()), vbg, 0, w, max_seeds=2, single_strand=True)[0].tolist() == [plant, min(tie_a, tie_b)]


@pytest.mark.parametrize("w", WS)
def test_ranking_both_strands_takes_one_of_a_pair(host, w):
    counts, plant, tie_a, tie_b = scripted_table(w, False)
    vbg = np.full(4, 0.25, np.float32)
    kmers, z, pwm = em.kmer_seeds(counts, int(counts.sum()), vbg, 0, w, max_seeds=10, single_strand=False)
    rc = lambda y: int(kmer_ref.revcomp(y, w))
    # of a w-mer and its reverse complement (equal counts, equal z) the smaller cell is taken and the other one skipped
    assert [int(k) for k in kmers] == [min(plant, rc(plant))] + sorted([min(tie_a, rc(tie_a)), min(tie_b, rc(tie_b))])
    rk, rz, rp = kmer_ref.seeds_ref(counts, int(counts.sum()), vbg, 0, w, 10, False)
    assert np.array_equal(kmers, rk) and np.array_equal(z, rz)
    assert np.array_equal(pwm.view(np.uint32), rp.view(np.uint32))
    # single-stranded ranking of the same table takes both members of each pair
    ss = em.kmer_seeds(counts, int(counts.sum()), vbg, 0, w, max_seeds=10, single_strand=True)[0]
    assert len(ss) == 6 and {plant, rc(plant)} <= set(int(k) for k in ss)


@pytest.mark.parametrize("Kbg", [0, 1, 2, 4])
@pytest.mark.parametrize("w", WS)
def test_ranking_against_restatement(host, w, Kbg):
    """A table counted from records, a background of every order the expectation can take: the same w-mers, the same z and
    PWM bits as the numpy restatement."""
    rs = np.random.RandomState(77 + w)
    recs = [rs.randint(1, 5, size=60).astype(np.uint8) for _ in range(300)]
    site = codes_of("TGACTCAT"[:w])
    for r in recs[::2]:
        r[20:20 + w] = site
    codes, off = kmer_ref.concat(recs)
    vbg = random_bg(Kbg, 5 + Kbg)
    for single_strand in (False, True):
        counts, total = em.kmer_counts_host(codes, off, w, single_strand)
        kmers, z, pwm = em.kmer_seeds(counts, total, vbg, Kbg, w, max_seeds=4, single_strand=single_strand)
        rk, rz, rp = kmer_ref.seeds_ref(counts, total, vbg, Kbg, w, 4, single_strand)
        assert len(kmers) == 4
        assert np.array_equal(kmers, rk) and np.array_equal(z, rz)
        assert np.array_equal(pwm.view(np.uint32), rp.view(np.uint32))
        assert np.allclose(pwm.sum(axis=1), 1.0, atol=1e-6)


def test_planted_consensus_ranks_first_on_the_host(host):
    """The premise of tests/test_cli_seed_kmers_gpu.py's planted-motif run, without the command line or a GPU: on
    kmer_ref.planted_set() the host twin and the ranking put the consensus, or its reverse complement, first by a wide margin."""
    codes, off = kmer_ref.planted_set()
    counts, total = em.kmer_counts_host(codes, off, 8)
    vbg = bm.PackedSeqs.from_codes(codes, off, False, seed=42).bg_model(2, np.array([1, 10, 10], np.float32))
    y = kmer_of(kmer_ref.CONSENSUS)
    for kmers, z, _ in (kmer_ref.seeds_ref(counts, total, vbg, 2, 8, 4, False), em.kmer_seeds(counts, total, vbg, 2, 8, 4)):
        assert int(kmers[0]) in (y, int(kmer_ref.revcomp(y, 8)))
        assert z[0] > 3 * z[1]


# ---- seed file -----------------------------------------------------------------------------------------------------------
def test_meme_round_trip(host, tmp_path):
    """What kmer_seeds_write prints comes back through load_seeds' MEME reader as the floats it was given: thirds, sevenths and
    the neighbours of 1 need all nine digits."""
    w, n = 8, 3
    rs = np.random.RandomState(3)
    pwm = rs.randint(1, 1000, size=(n, 4, w)).astype(np.float64)
    pwm = (pwm / pwm.sum(axis=1, keepdims=True)).astype(np.float32)
    pwm[0, :, 0] = np.float32([1 / 3, 1 / 7, np.nextafter(np.float32(0.5), np.float32(0)), 1 - 1 / 3 - 1 / 7 - 0.5])
    kmer = np.array([kmer_of("ACGTACGT"), kmer_of("TTTTGGGG"), 0], np.uint32)
    count = np.array([12, 2 ** 40 + 1, 0], np.uint64)
    z = np.array([1.5, 1e-3, 123456.789], np.float64)
    path = str(tmp_path / "x_seeds.meme")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert host.bh_kmer_seeds_write(path.encode(), C.c_uint32(w), C.c_uint32(n), vp(kmer), vp(count), vp(z), vp(np.ascontiguousarray(pwm))) == 0, host.bh_last_error()
    text = open(path).read()
    assert text.count("letter-probability matrix") == n
    assert "MOTIF ACGTACGT count= 12 z= 1.5" in text and "MOTIF TTTTGGGG count= 1099511627777" in text
    for i in range(n):
        got = np.zeros((4, w), np.float32)
        nm, wo = C.c_uint32(0), C.c_uint32(0)
        assert host.bh_read_meme_pwm(path.encode(), C.c_uint32(i), C.byref(nm), C.byref(wo), vp(got), C.c_uint64(got.size)) == 0, host.bh_last_error()
        assert nm.value == n and wo.value == w
        assert np.array_equal(got.view(np.uint32), pwm[i].view(np.uint32))


# ---- command line --------------------------------------------------------------------------------------------------------
FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example", "JunD.fasta")


def run_cli(host, *args):
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=120)


def test_cli_refuses_a_second_initial_model(host, tmp_path):
    for flag in ("--PWMFile", "--BaMMFile", "--bindingSiteFile"):
        p = run_cli(host, str(tmp_path / "o"), FASTA, "--seedKmers", "8", flag, "x")
        assert p.returncode == 1
        assert "--seedKmers cannot be combined with " + flag in p.stderr


@pytest.mark.parametrize("w", ["5", "9", "0", "-1"])
def test_cli_refuses_other_widths(host, tmp_path, w):
    p = run_cli(host, str(tmp_path / "o"), FASTA, "--seedKmers", w)
    assert p.returncode == 1 and "--seedKmers takes a width from 6 to 8" in p.stderr


def test_cli_without_a_model_still_exits(host, tmp_path):
    p = run_cli(host, str(tmp_path / "o"), FASTA, "--EM")
    assert p.returncode == 1 and "Error: No initial model is provided." in p.stderr
    p = run_cli(host, str(tmp_path / "o"), FASTA, "--hostSeedCounts")      # the helper flag alone names no model
    assert p.returncode == 1 and "Error: No initial model is provided." in p.stderr


def test_cli_seed_file_on_the_host(host, tmp_path):
    """Without a GPU stage the driver counts on the host: OUTDIR/<base>_seeds.meme holds the seeds the Python entry points give
    for the same records and the background model the driver learns, and the initial models are written from it."""
    out = str(tmp_path / "o")
    p = run_cli(host, out, FASTA, "--seedKmers", "8", "--maxPWM", "3", "--timing")
    assert p.returncode == 0, p.stderr
    assert "w-mer counts on the host" in p.stderr and "rank w-mers" in p.stderr
    n, nc = C.c_uint64(0), C.c_uint64(0)
    assert host.bh_read_fasta(FASTA.encode(), C.byref(n), C.byref(nc), None, None, None) == 0
    codes, off = np.zeros(nc.value, np.uint8), np.zeros(n.value + 1, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert host.bh_read_fasta(FASTA.encode(), C.byref(n), C.byref(nc), vp(codes), vp(off), None) == 0
    counts, total = em.kmer_counts_host(codes, off, 8)
    assert np.array_equal(counts, kmer_ref.counts_ref(codes, off, 8, False))
    vbg = bm.PackedSeqs.from_codes(codes, off, False, seed=42).bg_model(2, np.array([1, 10, 10], np.float32))
    kmers, z, pwm = em.kmer_seeds(counts, total, vbg, 2, 8, max_seeds=3)
    assert len(kmers) == 3
    for i in range(3):
        got = np.zeros((4, 8), np.float32)
        nm, wo = C.c_uint32(0), C.c_uint32(0)
        assert host.bh_read_meme_pwm(os.path.join(out, "JunD_seeds.meme").encode(), C.c_uint32(i), C.byref(nm), C.byref(wo), vp(got), C.c_uint64(32)) == 0
        assert nm.value == 3 and wo.value == 8
        assert np.array_equal(got.view(np.uint32), pwm[i].view(np.uint32))
    assert all(os.path.exists(os.path.join(out, f"JunD_motif_{i}.ihbcp")) for i in (1, 2, 3))
    assert not os.path.exists(os.path.join(out, "JunD_motif_4.ihbcp"))
