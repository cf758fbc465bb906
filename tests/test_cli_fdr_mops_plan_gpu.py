"""`BaMMmotif ... --FDR --mops -n 5` under a plan over several contexts (--deviceList 0,0 and 0,0,0: fold f on slot f mod N):
the window scores stay on the device there too -- one bamm_fdr handle per slot, sealed by the slot's thread, absorbed and
merged by the handle that computes the statistics -- and every output file is, byte for byte, what the same command writes
with --hostFdr (the scores downloaded, host/fdr.cpp) and what it writes on one slot.  One process per run."""
import random
import re
import subprocess

import pytest

from bammmotif2_amd import build
from tests.test_host_io_cpu import MEME

pytestmark = pytest.mark.gpu

RUN_SECONDS = 120                                            # a run takes about a second; a hung one ends here


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    """The fixture of tests/test_cli_fdr_mops_gpu.py: 200 sequences of 60..140 bases, every second one with the motif."""
    rnd = random.Random(5)
    motif = "TGACTCATCGGA"
    fa = tmp_path_factory.mktemp("plan") / "syn.fasta"
    with open(fa, "w") as f:
        for i in range(200):
            s = "".join(rnd.choices("ACGT", k=rnd.randint(60, 140)))
            if i % 2 == 0:
                k = rnd.randint(0, len(s) - len(motif))
                s = s[:k] + motif + s[k + len(motif):]
            f.write(f">s{i}\n{s}\n")
    return fa


def run(fasta, out, extra):
    r = subprocess.run([build.CLI, str(out), str(fasta), "--PWMFile", MEME, "--maxPWM", "1", "--timing", "--EM", "--FDR", "--mops",
                        "--savePRs", "--savePvalues", "-n", "5", "-m", "3"] + extra, capture_output=True, text=True, timeout=RUN_SECONDS)
    assert r.returncode == 0, r.stderr + r.stdout[-2000:]
    return {p.name: p.read_bytes() for p in sorted(out.iterdir())}, r.stderr


@pytest.fixture(scope="module")
def one_slot(fasta, tmp_path_factory, gpu_ctx):
    build.build_host()
    return run(fasta, tmp_path_factory.mktemp("one_slot"), [])


@pytest.mark.parametrize("device_list", ["0,0", "0,0,0"])
def test_plan_over_several_contexts_keeps_the_scores_on_the_device(device_list, fasta, one_slot, tmp_path, gpu_ctx):
    slots = device_list.count(",") + 1
    dev, dev_err = run(fasta, tmp_path / "dev", ["--deviceList", device_list])
    host, host_err = run(fasta, tmp_path / "host", ["--deviceList", device_list, "--hostFdr"])
    single, single_err = one_slot
    for name in ("syn_motif_1.mops.stats", "syn_motif_1.mops.pvalues", "syn_motif_1.zoops.stats", "syn_motif_1.zoops.pvalues"):
        assert name in dev, sorted(dev)
    assert dev["syn_motif_1.mops.stats"].count(b"\n") > 100 and dev["syn_motif_1.mops.pvalues"].count(b"\n") > 1000
    for other, what in ((host, "--hostFdr"), (single, "one slot")):
        assert dev.keys() == other.keys(), what
        for name in dev:
            assert dev[name] == other[name], (name, what)
    # the path each run took, in its own words
    m = re.search(r"MOPS window scores: device, (\d+) runs from (\d+) slots: seal \S+ s.*absorb \S+ s, merge \S+ s", dev_err)
    assert m, dev_err
    assert int(m.group(2)) == slots and int(m.group(1)) == slots
    assert "MOPS statistics on the device" in dev_err
    assert "MOPS window scores: host" in host_err and "MOPS statistics on the device" not in host_err
    assert re.search(r"MOPS window scores: device, 1 runs from 1 slots", single_err), single_err
