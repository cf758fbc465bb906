"""numpy restatements for the w-mer counter and the de novo seeder (helper; not collected by pytest).

counts_ref is the oracle of bamm_kmer_counts / bamm_kmer_counts_host: per record, slide a window of w codes, skip the windows
that hold a 0, add 1 to the window's cell and -- both strands -- 1 to its reverse complement's.  Exact integers, no tolerance.
seeds_ref restates host/seeder.cpp's ranking in float64, operation for operation.
"""
from __future__ import annotations

import numpy as np


def kmer_of(text: str) -> int:
    y = 0
    for ch in text:
        y = y * 4 + "ACGT".index(ch)
    return y


def codes_of(text: str) -> np.ndarray:
    return np.array([" ACGT".index(ch) if ch in "ACGT" else 0 for ch in text], np.uint8)


def revcomp(y, w: int):
    y = np.asarray(y, np.int64)
    rc = np.zeros_like(y)
    for _ in range(w):
        rc = rc * 4 + (3 - (y & 3))
        y = y >> 2
    return rc


def counts_ref(codes, off, w: int, single_strand: bool) -> np.ndarray:
    counts = np.zeros(4 ** w, np.uint64)
    pw = 4 ** np.arange(w - 1, -1, -1, dtype=np.int64)
    off = np.asarray(off, np.int64)
    for n in range(len(off) - 1):
        c = np.asarray(codes[off[n]:off[n + 1]], np.int64)
        if len(c) < w:
            continue
        win = np.lib.stride_tricks.sliding_window_view(c, w)
        win = win[(win != 0).all(axis=1)]
        np.add.at(counts, ((win - 1) * pw).sum(axis=1), 1)
        if not single_strand:
            np.add.at(counts, ((4 - win)[:, ::-1] * pw).sum(axis=1), 1)
    return counts


def concat(records):
    """(codes, off) of a list of code arrays."""
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    codes = np.concatenate([np.asarray(r, np.uint8) for r in records]) if records else np.zeros(0, np.uint8)
    return np.ascontiguousarray(codes, np.uint8), off


def bg_offset(k: int) -> int:
    return (4 ** (k + 1) - 4) // 3


def z_scores(counts, n_windows: int, vbg, Kbg: int, w: int, single_strand: bool) -> np.ndarray:
    y = np.arange(4 ** w, dtype=np.int64)
    P = np.ones(4 ** w, np.float64)
    for i in range(w):                                        # oldest base first
        k = min(i, Kbg)
        ctx = (y >> (2 * (w - 1 - i))) & (4 ** (k + 1) - 1)
        P = P * np.asarray(vbg, np.float32)[bg_offset(k) + ctx].astype(np.float64)
    E = np.float64(n_windows) * P if single_strand else np.float64(n_windows) * ((P + P[revcomp(y, w)]) * 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (np.asarray(counts).astype(np.float64) - E) / np.sqrt(E)
    return np.where(E > 0, z, 0.0)


def hamming(a: int, b: int, w: int) -> int:
    x = a ^ b
    return sum(1 for i in range(w) if (x >> (2 * i)) & 3)


def seed_pwm(counts, y: int, w: int) -> np.ndarray:
    pwm = np.zeros((4, w), np.float32)
    counts = [int(c) for c in counts]
    for j in range(w):
        sh = 2 * (w - 1 - j)
        n = [0, 0, 0, 0]
        members = [y] + [(y & ~(3 << s2)) | (b << s2) for s2 in range(0, 2 * w, 2) for b in range(4) if b != (y >> s2) & 3]
        assert len(members) == 3 * w + 1
        for m in members:
            n[(m >> sh) & 3] += counts[m]
        total = np.float64(sum(n)) + 4.0
        for b in range(4):
            pwm[b, j] = np.float32((np.float64(n[b]) + 1.0) / total)
    return pwm


def seeds_ref(counts, n_windows: int, vbg, Kbg: int, w: int, max_seeds: int = 4, single_strand: bool = False):
    """(w-mers, z, PWMs [n][4][w]) as host/seeder.cpp selects them."""
    z = z_scores(counts, n_windows, vbg, Kbg, w, single_strand)
    order = np.lexsort((np.arange(4 ** w), -z))               # descending z, ties to the smaller cell
    taken = []
    for y in (int(v) for v in order):
        if len(taken) >= max_seeds or not z[y] > 0:
            break
        rc = int(revcomp(y, w))
        if any(hamming(y, t, w) <= 1 or (not single_strand and hamming(rc, t, w) <= 1) for t in taken):
            continue
        taken.append(y)
    return (np.array(taken, np.uint32), np.array([z[t] for t in taken], np.float64),
            np.array([seed_pwm(counts, t, w) for t in taken], np.float32).reshape(len(taken), 4, w))


# ---- planted motif (tests/test_kmer_seeds_cpu.py checks the premise on the host, tests/test_cli_seed_kmers_gpu.py runs the driver) ----
CONSENSUS = "TGACGCAT"                                       # not its own reverse complement
PLANT_SEED = 11


def planted_set():
    """2 000 records of 100 bases, the consensus (each base with probability 0.97) planted in 60 % of them."""
    from bammmotif2_amd import synth
    pwm = np.full((4, 8), 0.01, np.float32)
    for j, ch in enumerate(CONSENSUS):
        pwm["ACGT".index(ch), j] = 0.97
    return synth.make_sequences(2000, 100, pwm, PLANT_SEED, plant_frac=0.6)
