"""`BaMMmotif ... --scoreSeqset` and `--FDR` on a FASTA whose records run from 300 to 34 000 bases (both strands: up to 68 001
positions), some with N: the negative set comes from the device (csrc/negs.hip, the long records segment by segment) by
default and from the host sampler with --hostSampler.  Every output file byte for byte, and the default run says where it
sampled."""
import random
import subprocess

import pytest

from bammmotif2_amd import build
from tests.test_host_io_cpu import MEME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    rnd = random.Random(23)
    fa = tmp_path_factory.mktemp("negs_long") / "long.fasta"
    with open(fa, "w") as f:
        for i, L in enumerate([300, 5000, 9000, 120, 34000, 2500, 800, 12000, 4097, 450]):
            s = "".join(rnd.choice("ACGT") for _ in range(L))
            if i % 3 == 0:
                k = rnd.randint(5, L - 5)
                s = s[:k] + "N" + s[k + 1:]
            f.write(f">rec{i}\n")
            for a in range(0, L, 80):
                f.write(s[a:a + 80] + "\n")
    return fa


@pytest.mark.parametrize("flags", [["--scoreSeqset"], ["--FDR", "-n", "5", "-m", "2"]], ids=["score", "fdr"])
def test_cli_long_records_device_sampler_and_host_sampler_write_the_same_files(flags, fasta, tmp_path, gpu_ctx):
    build.build_host()
    outs = []
    for extra in ([], ["--hostSampler"]):
        out = tmp_path / ("dev" if not extra else "host")
        r = subprocess.run([build.CLI, str(out), str(fasta), "--PWMFile", MEME, "--EM", "-k", "1", "--maxPWM", "1", "--maxEMIterations", "3",
                            "--timing"] + flags + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        assert ("sample (device" in r.stderr) == (not extra), r.stderr[-1500:]
        outs.append({p.name: p.read_bytes() for p in sorted(out.iterdir())})
    assert outs[0].keys() == outs[1].keys() and len(outs[0]) >= 1
    for name in outs[0]:
        assert outs[0][name] == outs[1][name], name
