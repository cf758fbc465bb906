"""`BaMMmotif OUT FASTA --seedKmers 8 --seedGaps 6 --EM`: a planted dyad TGAC nnnn GCAT, which no contiguous 8-mer sees, is
named first and refined.  The seeds go through OUTDIR/<base>_seeds.meme at their own widths and the existing --PWMFile path, so
a second run on that file writes the same models byte for byte; --hostSeedCounts writes the same seed file; --seedGaps 0 writes
the seed file of --seedKmers alone."""
import os
import subprocess

import pytest

from bammmotif2_amd import build
from tests import gapped_ref

pytestmark = pytest.mark.gpu

FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example", "JunD.fasta")
MODEL_FILES = ["planted_motif_1.ihbcp", "planted_motif_1.ihbp", "planted.hbcp", "planted.hbp"]


def run(*args):
    build.build_host()
    r = subprocess.run([build.CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    return r


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_planted_dyad_is_named_first_and_round_trips(tmp_path):
    """gapped_ref.planted_dyad_set(): tests/test_kmer_gapped_cpu.py checks the premise (host twin + numpy ranking) without a GPU."""
    codes, off = gapped_ref.planted_dyad_set()
    fasta = tmp_path / "planted.fasta"
    gapped_ref.write_fasta(fasta, codes, off)
    out1, out2, out3 = tmp_path / "o1", tmp_path / "o2", tmp_path / "o3"
    r = run(out1, fasta, "--seedKmers", 8, "--seedGaps", 6, "--EM", "--maxPWM", 1, "--timing")
    assert "dyad counts on the device (--seedKmers --seedGaps, gaps 0..6)" in r.stderr and "rank dyads (gaps 0..6)" in r.stderr
    seeds = out1 / "planted_seeds.meme"
    lines = open(seeds).read().split("\n")
    motif = [l for l in lines if l.startswith("MOTIF ")]
    assert len(motif) == 1 and motif[0].split()[1] in (gapped_ref.DYAD, gapped_ref.DYAD_RC) and motif[0].endswith(" gap= 4")
    assert any(l.startswith("letter-probability matrix: alength= 4 w= 12 ") for l in lines)
    assert os.path.exists(out1 / "planted_motif_1.ihbcp") and not os.path.exists(out1 / "planted_motif_2.ihbcp")
    # the seed file is an ordinary --PWMFile: the same models byte for byte
    run(out2, fasta, "--PWMFile", seeds, "--EM", "--maxPWM", 1)
    for f in MODEL_FILES:
        assert read(out1 / f) == read(out2 / f), f
    # the counts from the host twin: the same seed file, byte for byte
    r = run(out3, fasta, "--seedKmers", 8, "--seedGaps", 6, "--EM", "--maxPWM", 1, "--hostSeedCounts", "--timing")
    assert "dyad counts on the host" in r.stderr
    assert read(out3 / "planted_seeds.meme") == read(seeds)
    for f in MODEL_FILES:
        assert read(out1 / f) == read(out3 / f), f


def test_gap_zero_writes_the_seed_file_of_seed_kmers_alone(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    run(a, FASTA, "--seedKmers", 8, "--EM", "--maxPWM", 2, "--maxEMIterations", 1)
    r = run(b, FASTA, "--seedKmers", 8, "--seedGaps", 0, "--EM", "--maxPWM", 2, "--maxEMIterations", 1, "--timing")
    assert "dyad counts on the device" in r.stderr
    assert read(a / "JunD_seeds.meme") == read(b / "JunD_seeds.meme")
    assert b"gap=" not in read(b / "JunD_seeds.meme")
