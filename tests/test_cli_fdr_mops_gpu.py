"""`BaMMmotif ... --FDR --mops` with the MOPS statistics on the device (the default on one context: bamm_fdr) against
--hostFdr (every window's score downloaded, host/fdr.cpp::fdr_statistics, the path tests/test_eval_cpu.py pins to the
reference's files): every output file byte for byte."""
import random
import subprocess

import pytest

from bammmotif2_amd import build
from tests.test_host_io_cpu import MEME

pytestmark = pytest.mark.gpu


def test_cli_device_and_host_fdr_write_the_same_files(tmp_path, gpu_ctx):
    rnd = random.Random(5)
    motif = "TGACTCATCGGA"
    fa = tmp_path / "syn.fasta"
    with open(fa, "w") as f:
        for i in range(200):
            s = "".join(rnd.choices("ACGT", k=rnd.randint(60, 140)))
            if i % 2 == 0:
                k = rnd.randint(0, len(s) - len(motif))
                s = s[:k] + motif + s[k + len(motif):]
            f.write(f">s{i}\n{s}\n")
    build.build_host()
    outs, errs = [], []
    for extra in ([], ["--hostFdr"]):
        out = tmp_path / ("dev" if not extra else "host")
        r = subprocess.run([build.CLI, str(out), str(fa), "--PWMFile", MEME, "--maxPWM", "1", "--timing", "--EM", "--FDR", "--mops",
                            "--savePRs", "--savePvalues", "-n", "4", "-m", "3"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        outs.append({p.name: p.read_bytes() for p in sorted(out.iterdir())})
        errs.append(r.stderr)
    assert "MOPS statistics on the device" in errs[0] and "MOPS statistics on the device" not in errs[1]
    assert outs[0].keys() == outs[1].keys()
    for ext in (".mops.stats", ".mops.pvalues", ".zoops.stats", ".zoops.pvalues"):
        name = "syn_motif_1" + ext
        assert name in outs[0], sorted(outs[0])
        assert outs[0][name] == outs[1][name], name
    # .bmscore is what the reference's R scripts derive from the .stats files (R/evaluateBaMM.R); the binary writes none,
    # so both runs must agree on that as on every file they do write (the model, the background, the negatives' files)
    assert outs[0].get("syn_motif_1.bmscore") == outs[1].get("syn_motif_1.bmscore")
    for name in outs[0]:
        assert outs[0][name] == outs[1][name], name
    assert outs[0]["syn_motif_1.mops.stats"].count(b"\n") > 100 and outs[0]["syn_motif_1.mops.pvalues"].count(b"\n") > 1000
