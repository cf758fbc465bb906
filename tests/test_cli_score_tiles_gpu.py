"""`BaMMmotif ... --scoreSeqset` on a FASTA with one record of 20 kb among 50 of 200 bp: the long record is scored tile by
tile (csrc/scorer.hip, the one score_chain k_score runs too) by default and window by window with BAMM_NO_SCORE_TILES=1 in the environment -- the driver's
switch for comparing the program with itself.  Every output file, the .occurrence listing first, byte for byte."""
import os
import random
import subprocess

import pytest

from bammmotif2_amd import build
from tests.test_host_io_cpu import MEME

pytestmark = pytest.mark.gpu


def test_cli_occurrences_with_and_without_the_tiles(tmp_path, gpu_ctx):
    build.build_host()
    rnd = random.Random(5)
    motif = "TGACTCATCGGA"
    fa = tmp_path / "mixed.fasta"
    with open(fa, "w") as f:
        for i, n in enumerate([200] * 25 + [20000] + [200] * 25):
            s = "".join(rnd.choices("ACGT", k=n))
            for _ in range(max(1, n // 600) if i % 2 == 0 else 0):
                k = rnd.randint(0, n - len(motif))
                s = s[:k] + motif + s[k + len(motif):]
            f.write(f">s{i}\n{s}\n")
    outs = []
    for name, env in (("tiles", {}), ("windows", {"BAMM_NO_SCORE_TILES": "1"})):
        out = tmp_path / name
        r = subprocess.run([build.CLI, str(out), str(fa), "--PWMFile", MEME, "--maxPWM", "1", "--EM", "--scoreSeqset"],
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        outs.append({p.name: p.read_bytes() for p in sorted(out.iterdir())})
    assert "mixed_motif_1.occurrence" in outs[0] and outs[0]["mixed_motif_1.occurrence"].count(b"\n") > 1
    assert outs[0]["mixed_motif_1.occurrence"] == outs[1]["mixed_motif_1.occurrence"]
    assert outs[0].keys() == outs[1].keys()
    for name in outs[0]:
        assert outs[0][name] == outs[1][name], name
