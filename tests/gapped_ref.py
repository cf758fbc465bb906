"""numpy restatements for the dyad counter and the cross-gap ranking (helper; not collected by pytest).

gapped_counts_ref is the oracle of bamm_kmer_counts_gapped / bamm_kmer_counts_gapped_host: per record and gap, slide a window
of S = w + g codes, drop the windows that hold a 0 anywhere (gap positions included), take the 2 h informative columns, add 1
to the cell and -- both strands -- 1 to its reverse complement's.  Exact integers, no tolerance.
gapped_seeds_ref restates host/seeder.cpp's kmer_seeds_gapped in float64, operation for operation.
"""
from __future__ import annotations

import numpy as np

from tests import kmer_ref
from tests.kmer_ref import bg_offset, hamming, revcomp, seed_pwm


def gapped_counts_ref(codes, off, w: int, gap_lo: int, gap_hi: int, single_strand: bool) -> np.ndarray:
    """counts [n_gaps, 4^w]."""
    h = w // 2
    counts = np.zeros((gap_hi - gap_lo + 1, 4 ** w), np.uint64)
    pw = 4 ** np.arange(w - 1, -1, -1, dtype=np.int64)
    off = np.asarray(off, np.int64)
    for g in range(gap_lo, gap_hi + 1):
        S = w + g
        cols = np.r_[np.arange(h), np.arange(S - (w - h), S)]
        table = counts[g - gap_lo]
        for n in range(len(off) - 1):
            c = np.asarray(codes[off[n]:off[n + 1]], np.int64)
            if len(c) < S:
                continue
            win = np.lib.stride_tricks.sliding_window_view(c, S)
            win = win[(win != 0).all(axis=1)][:, cols]
            np.add.at(table, ((win - 1) * pw).sum(axis=1), 1)
            if not single_strand:
                np.add.at(table, ((4 - win)[:, ::-1] * pw).sum(axis=1), 1)
    return counts


def dyad_string(y: int, w: int, g: int) -> str:
    s = "".join("ACGT"[(y >> (2 * (w - 1 - i))) & 3] for i in range(w))
    return s[: w // 2] + "n" * g + s[w // 2:] if g else s


def window_p(vbg, Kbg: int, w: int) -> np.ndarray:
    """P(y) of every w-mer: the product, oldest base first, of the conditionals at order min(i, Kbg)."""
    y = np.arange(4 ** w, dtype=np.int64)
    P = np.ones(4 ** w, np.float64)
    for i in range(w):
        k = min(i, Kbg)
        ctx = (y >> (2 * (w - 1 - i))) & (4 ** (k + 1) - 1)
        P = P * np.asarray(vbg, np.float32)[bg_offset(k) + ctx].astype(np.float64)
    return P


def gapped_z(counts, n_windows, vbg, Kbg: int, w: int, gap_lo: int, gap_hi: int, single_strand: bool) -> np.ndarray:
    h = w // 2
    y = np.arange(4 ** w, dtype=np.int64)
    rc = revcomp(y, w)
    z = np.zeros((gap_hi - gap_lo + 1, 4 ** w), np.float64)
    for g in range(gap_lo, gap_hi + 1):
        if g == 0:
            P = window_p(vbg, Kbg, w)
        else:
            ph = window_p(vbg, Kbg, h)
            P = ph[y >> (2 * h)] * ph[y & (4 ** h - 1)]
        nw = np.float64(int(n_windows[g - gap_lo]))
        E = nw * P if single_strand else nw * ((P + P[rc]) * 0.5)
        with np.errstate(divide="ignore", invalid="ignore"):
            zz = (np.asarray(counts[g - gap_lo]).astype(np.float64) - E) / np.sqrt(E)
        z[g - gap_lo] = np.where(E > 0, zz, 0.0)
    return z


def gapped_pwm(table, y: int, w: int, g: int) -> np.ndarray:
    """[4][w + g]: the contiguous seed's columns (kmer_ref.seed_pwm on the gap's table) around g columns of 0.25."""
    h = w // 2
    inner = seed_pwm(table, y, w)
    pwm = np.full((4, w + g), 0.25, np.float32)
    pwm[:, :h] = inner[:, :h]
    pwm[:, h + g:] = inner[:, h:]
    return pwm


def gapped_seeds_ref(counts, n_windows, vbg, Kbg: int, w: int, gap_lo: int, gap_hi: int, max_seeds: int = 4, single_strand: bool = False):
    """(w-mers, gaps, z, list of PWMs [4][w + gap]) as host/seeder.cpp's kmer_seeds_gapped selects them."""
    counts = np.asarray(counts).reshape(gap_hi - gap_lo + 1, 4 ** w)
    h, cells = w // 2, 4 ** w
    z = gapped_z(counts, n_windows, vbg, Kbg, w, gap_lo, gap_hi, single_strand).reshape(-1)
    order = np.lexsort((np.arange(len(z)), -z))               # descending z, ties to the smaller gap, then the smaller cell
    left, right = (lambda v: v >> (2 * h)), (lambda v: v & (4 ** h - 1))
    shares = lambda a, b: left(a) == left(b) or right(a) == right(b)
    taken = []
    for i in (int(v) for v in order):
        if len(taken) >= max_seeds or not z[i] > 0:
            break
        g, y = gap_lo + i // cells, i % cells
        rc = int(revcomp(y, w))
        skip = False
        for (ty, tg, _) in taken:
            if tg == g:
                skip = skip or hamming(y, ty, w) <= 1 or (not single_strand and hamming(rc, ty, w) <= 1)
            else:
                skip = skip or shares(y, ty) or (not single_strand and shares(rc, ty))
        if skip:
            continue
        taken.append((y, g, z[i]))
    return (np.array([t[0] for t in taken], np.uint32), np.array([t[1] for t in taken], np.uint32),
            np.array([t[2] for t in taken], np.float64), [gapped_pwm(counts[g - gap_lo], y, w, g) for (y, g, _) in taken])


# ---- planted dyad (tests/test_kmer_gapped_cpu.py checks the premise on the host, tests/test_cli_seed_gaps_gpu.py runs the driver) ----
LEFT, RIGHT, PLANT_GAP = "TGAC", "GCAT", 4
DYAD = LEFT + "n" * PLANT_GAP + RIGHT
DYAD_RC = "ATGC" + "n" * PLANT_GAP + "GTCA"
PLANT_SEED = 13


def planted_dyad_set():
    """2 000 records of 100 bases; TGAC nnnn GCAT (each informative base with probability 0.97, the four between them
    uniform) planted in 60 % of them."""
    from bammmotif2_amd import synth
    pwm = np.full((4, 12), 0.25, np.float32)
    for j, ch in list(enumerate(LEFT)) + [(8 + j, ch) for j, ch in enumerate(RIGHT)]:
        pwm[:, j] = 0.01
        pwm["ACGT".index(ch), j] = 0.97
    return synth.make_sequences(2000, 100, pwm, PLANT_SEED, plant_frac=0.6)


def write_fasta(path, codes, off):
    with open(path, "w") as fh:
        for n in range(len(off) - 1):
            fh.write(f">s{n}\n" + "".join(" ACGT"[c] for c in codes[int(off[n]):int(off[n + 1])]) + "\n")


concat, codes_of, kmer_of = kmer_ref.concat, kmer_ref.codes_of, kmer_ref.kmer_of
