"""`BaMMmotif ... -k 5 --EM --scoreSeqset --FDR --mops` at W = 12, a log-odds table of 196 KiB: the driver turns
"score_slices" on for its contexts, so every scoring call behind --scoreSeqset and the folds of --FDR takes the table a
slice of columns per launch (csrc/scorer.hip), the record of 20 kb tile by tile; with BAMM_NO_SCORE_SLICES=1 in the
environment it keeps the window-by-window scorer.  Every output file byte for byte."""
import os
import random
import subprocess

import numpy as np
import pytest

import bammmotif2_amd as bm
from bammmotif2_amd import build, synth

pytestmark = pytest.mark.gpu

K, W = 5, 12


def write_bamm(path, v):
    """the .ihbcp layout (Motif.cpp:515-547): per motif position one line per order, a blank line behind them"""
    with open(path, "w") as f:
        for j in range(W):
            for k in range(K + 1):
                f.write(" ".join("%.3e" % x for x in v[bm.v_offset(k, W) + np.arange(4 ** (k + 1)) * W + j]) + " \n")
            f.write("\n")


def test_cli_outputs_with_and_without_the_slices(tmp_path, gpu_ctx):
    build.build_host()
    assert bm.score_slice_geometry(K, W) == (6, 2)
    pwm = synth.make_pwm(W, 3)
    motif = "".join("ACGT"[i] for i in np.argmax(pwm, axis=0))   # [4][W]: the consensus, planted below
    seed = tmp_path / "seed.ihbcp"
    write_bamm(seed, synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K))
    rnd = random.Random(5)
    fa = tmp_path / "mixed.fasta"
    with open(fa, "w") as f:
        for i, n in enumerate([200] * 30 + [20000] + [200] * 30):
            s = "".join(rnd.choices("ACGT", k=n))
            for _ in range(max(1, n // 600) if i % 2 == 0 else 0):
                k = rnd.randint(0, n - W)
                s = s[:k] + motif + s[k + W:]
            f.write(f">s{i}\n{s}\n")
    outs = []
    for name, env in (("slices", {}), ("windows", {"BAMM_NO_SCORE_SLICES": "1"})):
        out = tmp_path / name
        r = subprocess.run([build.CLI, str(out), str(fa), "--BaMMFile", str(seed), "-k", str(K), "--EM", "--scoreSeqset", "--FDR", "--mops"],
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        outs.append({p.name: p.read_bytes() for p in sorted(out.iterdir())})
    assert "mixed_motif_1.occurrence" in outs[0] and outs[0]["mixed_motif_1.occurrence"].count(b"\n") > 1
    assert any(n.endswith(".mops.stats") for n in outs[0]), sorted(outs[0])
    assert outs[0].keys() == outs[1].keys()
    for name in outs[0]:
        assert outs[0][name] == outs[1][name], name
