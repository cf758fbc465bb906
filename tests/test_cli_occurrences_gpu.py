"""`BaMMmotif ... --scoreSeqset` with the window p-values on the device (the default: bamm_occurrences) against --hostPvalues
(every window's score downloaded, host/fdr.cpp::mops_pvalues, the path the reference's goldens pin in test_cli_gpu.py): every
output file byte for byte."""
import random
import subprocess

import pytest

from bammmotif2_amd import build
from tests.test_host_io_cpu import FASTA, MEME

pytestmark = pytest.mark.gpu


def run_both(tmp_path, fasta, flags):
    build.build_host()
    outs = []
    for extra in ([], ["--hostPvalues"]):
        out = tmp_path / ("dev" if not extra else "host")
        r = subprocess.run([build.CLI, str(out), str(fasta), "--PWMFile", MEME, "--maxPWM", "1", "--timing"] + flags + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        assert "--scoreSeqset: score + p-values + .occurrence" in r.stderr
        outs.append({p.name: p.read_bytes() for p in sorted(out.iterdir())})
    assert outs[0].keys() == outs[1].keys()
    for name in outs[0]:
        assert outs[0][name] == outs[1][name], name
    return outs[0]


def test_cli_travis_line_device_and_host_pvalues_write_the_same_files(tmp_path, gpu_ctx):
    """The reference's CI line (.travis.yml:21) on JunD."""
    files = run_both(tmp_path, FASTA, ["--EM", "-k", "0", "--FDR", "--scoreSeqset"])
    assert "JunD_motif_1.occurrence" in files and files["JunD_motif_1.occurrence"].count(b"\n") > 1


def test_cli_save_logodds_device_and_host_pvalues_write_the_same_files(tmp_path, gpu_ctx):
    """--EM --FDR --scoreSeqset --saveLogOdds -m 2 on 20 000 x 200 bp (-m is parsed with --FDR only, Global.cpp:303-307): the
    .occurrence file and both .logOddsZoops listings (whose maxima the device path still asks the scorer for, without the
    window scores)."""
    rnd = random.Random(11)
    motif = "TGACTCATCGGA"
    fa = tmp_path / "syn.fasta"
    with open(fa, "w") as f:
        for i in range(20000):
            s = "".join(rnd.choices("ACGT", k=200))
            if i % 3 == 0:
                k = rnd.randint(0, 200 - len(motif))
                s = s[:k] + motif + s[k + len(motif):]
            f.write(f">s{i}\n{s}\n")
    files = run_both(tmp_path, fa, ["--EM", "--FDR", "--scoreSeqset", "--saveLogOdds", "-m", "2"])
    assert "syn_motif_1.occurrence" in files and "syn_motif_1.logOddsZoops" in files and "syn.negSet.logOddsZoops" in files
    assert files["syn_motif_1.occurrence"].count(b"\n") > 100


def test_cli_plain_score_line_device_and_host_pvalues_write_the_same_files(tmp_path, gpu_ctx):
    """--EM --scoreSeqset --saveLogOdds without --FDR: the negatives are sampled for the scoring stage alone."""
    files = run_both(tmp_path, FASTA, ["--EM", "--scoreSeqset", "--saveLogOdds"])
    assert "JunD_motif_1.occurrence" in files and "JunD_motif_1.logOddsZoops" in files and "JunD.negSet.logOddsZoops" in files
