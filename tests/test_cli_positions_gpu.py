"""`BaMMmotif ... --EM --saveBaMMs`: the .positions file from the sites the device lists (the default: bamm_em_sites) against
--hostPositions (every responsibility downloaded and scanned on the host, the path the reference's goldens pin in
test_cli_gpu.py): byte for byte, with .counts and the model file unchanged."""
import subprocess

import pytest

from bammmotif2_amd import build
from tests.test_host_io_cpu import FASTA, MEME

pytestmark = pytest.mark.gpu


def run_both(tmp_path, flags):
    build.build_host()
    outs = []
    for extra in ([], ["--hostPositions"]):
        out = tmp_path / ("dev" if not extra else "host")
        r = subprocess.run([build.CLI, str(out), FASTA, "--PWMFile", MEME, "--maxPWM", "1", "--EM", "--saveBaMMs", "--timing"] + flags + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        assert "Unknown option(s)" not in r.stderr
        assert ("dense r" in r.stderr) == bool(extra) and (" sites, " in r.stderr) == (not extra)    # which path wrote the file
        outs.append({p.name: p.read_bytes() for p in sorted(out.iterdir())})
    assert outs[0].keys() == outs[1].keys()
    for name in ("JunD_motif_1.positions", "JunD_motif_1.counts", "JunD_motif_1.ihbcp"):
        assert name in outs[0] and outs[0][name] == outs[1][name], name
    rows = outs[0]["JunD_motif_1.positions"].split(b"\n")
    assert rows[0] == b"seq\tlength\tstrand\tstart..end\tpattern" and len(rows) > 10
    return outs[0]


@pytest.mark.parametrize("flags", [["-k", "0"], ["-k", "2"], ["-k", "2", "--ss"], ["-k", "2", "--advanceEM"],
                                   ["-k", "2", "--deviceList", "0,0"]],
                         ids=["k0", "k2", "ss", "advanceEM", "two_slots"])
def test_cli_device_and_host_positions_write_the_same_files(flags, tmp_path, gpu_ctx):
    files = run_both(tmp_path, flags)
    strands = {row.split(b"\t")[2] for row in files["JunD_motif_1.positions"].split(b"\n")[1:] if row}
    assert strands == {b"+"} if "--ss" in flags else b"+" in strands


def test_cli_knows_host_positions(tmp_path, gpu_ctx):
    """--hostPositions alone is a known option (an unknown one prints the help and exits with 1)."""
    build.build_host()
    r = subprocess.run([build.CLI, str(tmp_path / "o"), FASTA, "--PWMFile", MEME, "--maxPWM", "1", "--hostPositions"],
                       capture_output=True, text=True)
    assert "Unknown option(s)" not in r.stderr and r.returncode == 0, r.stderr
    r = subprocess.run([build.CLI, str(tmp_path / "o2"), FASTA, "--PWMFile", MEME, "--maxPWM", "1", "--hostPositionz"],
                       capture_output=True, text=True)
    assert "Unknown option(s)" in r.stderr and r.returncode == 1
